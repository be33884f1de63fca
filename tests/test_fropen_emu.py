"""The openings over Fr executed on the CPU (tests/host_emu/fropen.cpp: the lane bodies of csrc/fropen.hpp, phase by phase with 256 emulated
lanes as the kernels walk them) against Python integers mod r (tests/fropen_cases.py): both forms at every size where the chunking changes,
chosen z and images, the domain in both orders, z in the domain, and the two formulas of the evaluation form against the coefficient route
through an interpolation.  The device half is tests/test_gpu_fr_open.py."""
import ctypes
import os
import random
import subprocess

import pytest

import fropen_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
R = fc.R
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_fropen.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libfropen.so"))
    cp = ctypes.c_char_p
    L.emu_fropen_coef.argtypes = [cp, SZ, cp, SZ, cp, cp, cp]
    L.emu_fropen_eval.argtypes = [cp, SZ, cp, SZ, cp, cp, cp, cp, ctypes.POINTER(SZ)]
    L.emu_fr_ops.argtypes = [cp, cp, cp, cp, cp, ctypes.POINTER(ctypes.c_int)]
    L.emu_fr_ops.restype = None
    L.emu_fr_pow.argtypes = [cp, ctypes.c_uint64, cp]
    L.emu_fr_pow.restype = None
    return L


def run(lib, polys, zs, xs=None):
    k, n = len(polys), len(polys[0])
    ys, q, st = ctypes.create_string_buffer(32 * k), ctypes.create_string_buffer(32 * k * n), ctypes.create_string_buffer(k)
    if xs is None:
        r = lib.emu_fropen_coef(fc.pack(polys), n, fc.pack([zs]), k, ys, q, st)
    else:
        invs = SZ()
        r = lib.emu_fropen_eval(fc.pack(polys), n, fc.pack([zs]), k, fc.pack([xs]), ys, q, st, ctypes.byref(invs))
        assert invs.value == k                        # one inversion per polynomial
    return ys.raw, q.raw, st.raw, r


def test_fr_additions_against_python_integers(lib):
    rng = random.Random(1)
    values = [0, 1, 2, R - 1, R, R + 1, R + 5, 2 * R - 1, 2 * R, 2 * R + 1, (1 << 256) - 1, (1 << 255)] + [rng.getrandbits(256) for _ in range(50)]
    bufs = [ctypes.create_string_buffer(32) for _ in range(4)]
    red = ctypes.c_int()
    for v in values:
        lib.emu_fr_ops(fc.le(v), *bufs, ctypes.byref(red))
        got = [int.from_bytes(b.raw, "little") for b in bufs]
        assert got == [-v % R, v * v % R, v % R, v % R] and bool(red.value) == (v >= R), hex(v)
    out = ctypes.create_string_buffer(32)
    for v in values[:12]:
        for e in (0, 1, 2, 3, 16, 255, 256, 4097, (1 << 64) - 1):
            lib.emu_fr_pow(fc.le(v), e, out)
            assert int.from_bytes(out.raw, "little") == pow(v, e, R), (hex(v), e)


@pytest.mark.parametrize("n", fc.N_BOTH)
def test_coefficient_form(lib, n):
    polys, zs = fc.random_call(n, n, 3, [random.Random(n).randrange(R), 0, 1])
    assert run(lib, polys, zs) == fc.expected(polys, zs)
    y, q = fc.coef_open(polys[0], zs[0])              # the quotient's own meaning: p = q (X - z) + y, slot n - 1 empty
    assert q[n - 1] == 0 and all((q[i - 1] - z_q) % R == polys[0][i] for i, z_q in ((i, zs[0] * q[i]) for i in range(1, n)))
    assert fc.evaluate(polys[0], zs[0]) == y


@pytest.mark.parametrize("n", fc.N_EVAL)
@pytest.mark.parametrize("bit_reversed", [False, True])
def test_evaluation_form(lib, n, bit_reversed):
    xs = fc.domain(n, bit_reversed)
    rng = random.Random(n)
    pool = [rng.randrange(R), xs[0], xs[n - 1], xs[n // 2], rng.randrange(R), 0]
    polys, zs = fc.random_call(100 + n, n, len(pool), pool)
    got, want = run(lib, polys, zs, xs), fc.expected(polys, zs, xs)
    assert got == want
    assert [b & fc.IN_DOMAIN for b in got[2]] == [0, 1, 1, 1, 0, 0]


def chosen(n):
    rng = random.Random(7 * n)
    rows = [[0] * n, [R - 1] * n, [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]]
    rows[2][n // 2] = (1 << 256) - 1
    rows[3][n - 1] = R
    return rows


@pytest.mark.parametrize("n", [3, 257])
def test_chosen_points_and_images_coefficient_form(lib, n):
    for z in (0, 1, R - 1, R + 5):
        polys = chosen(n)
        got, want = run(lib, polys, [z] * 4), fc.expected(polys, [z] * 4)
        assert got == want
        assert want[2] == bytes([2 if z >= R else 0] * 2 + [2, 2]) and want[3] == (4 if z >= R else 2)
        assert all(v < R for v in fc.images(got[0]) + fc.images(got[1]))


@pytest.mark.parametrize("n", [2, 512])
def test_chosen_points_and_images_evaluation_form(lib, n):
    xs = fc.domain(n)
    assert xs[0] == 1 and R - 1 in xs                  # z = 1 and z = r - 1 lie in every domain from n = 2 on
    for z in (0, 1, R - 1, R + 5, R + 1):
        polys = chosen(n)
        got, want = run(lib, polys, [z] * 4, xs), fc.expected(polys, [z] * 4, xs)
        assert got == want
        assert all(b & fc.IN_DOMAIN == int(z % R in (1, R - 1)) for b in got[2]) and all(v < R for v in fc.images(got[0]) + fc.images(got[1]))


@pytest.mark.parametrize("n", [8, 256])
def test_evaluation_quotient_is_the_coefficient_quotient_evaluated(lib, n):
    xs = fc.domain(n, True)
    random.Random(3).shuffle(xs)                      # the caller's order is any order
    rng = random.Random(n)
    f = [rng.randrange(R) for _ in range(n)]
    c = fc.interpolate(f, xs)
    assert [fc.evaluate(c, x) for x in xs[:4]] == f[:4]
    for z in (rng.randrange(R), xs[0], xs[n - 1], xs[5]):
        y, q = fc.coef_open(c, z)
        ys, quot, st, _ = run(lib, [f], [z], xs)
        assert fc.images(ys) == [y] and fc.images(quot) == [fc.evaluate(q, x) for x in xs], z in xs
        assert st == bytes([int(z in xs)])
