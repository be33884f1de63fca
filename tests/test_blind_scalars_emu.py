"""CPU side of the chosen-blinding-scalar tests (tests/blind_scalars.py): the family census, and the COMPILED 64-bit multiplication -
curve.hpp jac_mul_u64_w4_body<fp>, the fallback of k_pkmul and the body csrc/combsets.hpp restates - on every family scalar under the
bounds-tracked CPU build.  Its digit rule is a carry chain (a digit above 8 borrows from the next one, so +8 stays +8), not the assembly loop's
bias: the same families reach its carries, its carry digit 16 and its zero digits.  The generated assembly blocks run the named subset in
tests/test_asm_loops.py; the device runs everything in tests/test_gpu_blind_scalars.py."""
import ctypes
import random

import bls12381_py as o
import blind_scalars as bs
from util import buf, g1_jac_to_affine


def test_census_holds_and_names_are_usable():
    """the module asserted its census on import; what the tests index it by is there"""
    assert len(bs.ALL) == len(bs.SCALARS) == len(bs.NAMES) and 4 * 64 < len(bs.ALL) < 6 * 64
    assert {f for f in bs.FAMILIES} == {"single_digit", "equal_nibbles", "all_minus_8", "edges", "random"}
    assert len(bs.FAMILIES["single_digit"]) == 240 and len(bs.FAMILIES["equal_nibbles"]) == 15 and len(bs.FAMILIES["random"]) == 32
    assert [v for _, v in bs.FAMILIES["edges"]] == [1, 2, 7, 8, 9, 15, 16, 17, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**64 - 8]
    assert bs.rotated(17)[0] == bs.ALL[17] and bs.rotated(17)[-1] == bs.ALL[16] and sorted(bs.rotated(17)) == sorted(bs.ALL)
    for r in (1, 8, 2**64 - 1, 0x7777777777777778):
        assert sum(d * 16**j for j, d in enumerate(bs.digits(r))) == r
    assert bs.unsigned_digits(2**64 - 1, 8) == [255] * 8 and bs.unsigned_digits(1, 4) == [1] + [0] * 15


def test_compiled_multiplication_on_every_family_scalar(emu):
    rng = random.Random(20261019)
    keys = [o.g1_mul(o.G1_GEN, rng.randrange(1, o.R)) for _ in range(2)]
    for key in keys:
        image = o.g1_to_blst_affine(key)
        for name, r in bs.ALL:
            out = buf(144)
            emu.emu_g1_mul_u64_w4(image, ctypes.c_uint64(r), out)
            assert g1_jac_to_affine(out.raw) == o.g1_mul(key, r), name
