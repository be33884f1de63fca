"""The cases the p1s_ntt tests share (tests/test_p1ntt_emu.py on the CPU, tests/test_gpu_p1s_ntt.py on the device): tests/golden/p1ntt.json,
made by tests/golden/gen_p1ntt.py from the oracle's point arithmetic and frntt_cases.ntt.  Nothing here comes from the code under test."""
import functools
import json
import os

import frntt_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
R = fc.R
INVERSE, BITREV = 1, 2
FLAGS = (0, INVERSE, BITREV, INVERSE | BITREV)
ROW = 96                                              # a blst_p1_affine image; all zero: infinity
# the generator G as such an image (Montgomery form, R = 2^384): the one-row table the larger tests multiply
G1X = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
G1Y = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
G_IMAGE = b"".join((c * (1 << 384) % P).to_bytes(48, "little") for c in (G1X, G1Y))


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "p1ntt.json")) as f:
        return json.load(f)


def cases():
    """-> [(name, n, k, flags, input images, expected images)] over every case and every flag value it is stored for"""
    out = []
    for c in fixture()["cases"]:
        for f in sorted(c["out"], key=int):
            out.append((c["name"], c["n"], c["k"], int(f), bytes.fromhex(c["in"]), bytes.fromhex(c["out"][f])))
    return out


def case(name):
    return [c for c in fixture()["cases"] if c["name"] == name][0]


def scalars(c):
    return [[int(a, 16) for a in v] for v in c["scalars"]]


def rows(b):
    return [b[i:i + ROW] for i in range(0, len(b), ROW)]


def expected_scalars(vectors, flags):
    """the scalars of the expected outputs: frntt_cases.ntt of each vector under the same flags"""
    return [fc.ntt(list(v), bool(flags & INVERSE), bool(flags & BITREV)) for v in vectors]


def twiddle_multiplications(n, k, flags):
    """the butterflies of a call that multiply by a twiddle: all but those whose twiddle is 1 (n - 1 of a vector's (n / 2) log2 n); the
    inverse folds 1 / n into the stage at the top bit, where the butterfly with twiddle 1 then multiplies by 1 / n like the others"""
    m = n.bit_length() - 1
    return k * (n // 2 * m - (n - 1) + (1 if flags & INVERSE and m else 0))
