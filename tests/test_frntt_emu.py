"""The transforms over Fr executed on the CPU (tests/host_emu/frntt.cpp: the lane bodies of csrc/frntt.hpp, phase by phase with 256 emulated
lanes as the kernels walk them, in the order the host call launches them) against Python integers mod r (tests/frntt_cases.py): the root
constant, the twiddle table, tile-only sizes, forced tiles that need two and three passes, every flag combination, coset shifts, images that
are not canonical, and inverse of forward.  The device half is tests/test_gpu_fr_ntt.py."""
import ctypes
import os
import subprocess

import pytest

import fropen_cases as fo
import frntt_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
R = fc.R
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_frntt.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libfrntt.so"))
    cp = ctypes.c_char_p
    L.emu_frntt.argtypes = [cp, SZ, SZ, U32, cp, U32, SZ, cp, cp, ctypes.POINTER(U32)]
    L.emu_frntt_twiddles.argtypes = [SZ, ctypes.c_int, cp]
    L.emu_frntt_twiddles.restype = None
    L.emu_frntt_omega32.argtypes = [U32, cp]
    L.emu_frntt_omega32.restype = None
    L.emu_frntt_domain.argtypes = [SZ, ctypes.c_int, cp]
    L.emu_frntt_domain.restype = None
    L.emu_frntt_rev.argtypes = [ctypes.c_uint64, U32]
    L.emu_frntt_rev.restype = ctypes.c_uint64
    L.frntt_plan_tile.restype = U32
    return L


def run(lib, vectors, flags=0, shift=None, tile=0, vecs=0):
    """-> (output bytes, status bytes, the count), and the passes of one transform"""
    k, n = len(vectors), len(vectors[0])
    out, st, passes = ctypes.create_string_buffer(32 * k * n), ctypes.create_string_buffer(k), U32()
    r = lib.emu_frntt(fc.pack(vectors), n, k, flags, fc.le(shift) if shift is not None else None, tile, vecs, out, st, ctypes.byref(passes))
    return (out.raw, st.raw, r), passes.value


def test_the_helper_itself():
    v = list(fc.random_vectors(1, 1, 64)[0])
    for inverse in (False, True):
        for bitrev in (False, True):
            for shift in (1, 7):
                assert fc.ntt_fast(v, inverse, bitrev, shift) == fc.ntt_definition(v, inverse, bitrev, shift)
    assert fc.ntt_definition([5, 6], shift=3) == [(5 + 18) % R, (5 - 18) % R]
    assert fc.ntt_definition(fc.ntt_definition(v[:8], False, True, 7), True, True, 7) == v[:8]
    assert fc.domain(8) == fo.domain(8) and fc.domain(8, True) == fo.domain(8, True)


def test_the_root_constant(lib):
    out = ctypes.create_string_buffer(32)
    lib.emu_frntt_omega32(0, out)
    assert int.from_bytes(out.raw, "little") == pow(7, (R - 1) >> 32, R)
    lib.emu_frntt_omega32(31, out)
    assert int.from_bytes(out.raw, "little") == R - 1
    lib.emu_frntt_omega32(32, out)
    assert int.from_bytes(out.raw, "little") == 1
    for m in (0, 1, 3, 12, 31, 32):
        for i in {0, 1 % (1 << m), 5 % (1 << m), (1 << m) - 1, (1 << m) // 3}:
            assert lib.emu_frntt_rev(i, m) == fc.rev(i, m), (i, m)


@pytest.mark.parametrize("n", [2, 8, 1024])
def test_the_twiddle_table_entry_by_entry(lib, n):
    for inverse in (0, 1):
        out = ctypes.create_string_buffer(32 * (n // 2))
        lib.emu_frntt_twiddles(n, inverse, out)
        w = pow(fc.omega(n), -1 if inverse else 1, R)
        assert fc.images(out.raw) == [pow(w, j, R) for j in range(n // 2)]


@pytest.mark.parametrize("n", [1, 2, 4096])
def test_the_domain(lib, n):
    for bitrev in (0, 1):
        out = ctypes.create_string_buffer(32 * n)
        lib.emu_frntt_domain(n, bitrev, out)
        assert fc.images(out.raw) == fo.domain(n, bool(bitrev))


@pytest.mark.parametrize("flags", fc.FLAGS)
def test_tile_only_sizes(lib, flags):
    for n in (1, 2, 4, 256, 512, 1 << lib.frntt_plan_tile()):
        vectors = fc.random_vectors(n, 3, n)
        got, passes = run(lib, vectors, flags)
        assert got == fc.expected(vectors, flags) and passes == (1 if n > 1 else 0), n


@pytest.mark.parametrize("flags", fc.FLAGS)
@pytest.mark.parametrize("n,passes", [(4, 1), (8, 2), (16, 2), (64, 3)])
def test_forced_tile_of_four_elements(lib, n, passes, flags):
    for k in (1, 3):
        vectors = fc.random_vectors(100 + n, k, n)
        got, ran = run(lib, vectors, flags, tile=2)
        assert got == fc.expected(vectors, flags) and ran == passes, (n, k)


@pytest.mark.parametrize("flags", fc.FLAGS)
def test_two_passes_at_the_default_tile_and_slices(lib, flags):
    n = 2 << lib.frntt_plan_tile()
    vectors = fc.random_vectors(7, 3, n)
    got, ran = run(lib, vectors, flags, shift=7)
    assert got == fc.expected(vectors, flags, 7) and ran == 2
    assert run(lib, vectors, flags, shift=7, vecs=2)[0] == got


@pytest.mark.parametrize("flags", fc.FLAGS)
@pytest.mark.parametrize("n,tile", [(16, 0), (16, 2), (64, 3)])
def test_shifts(lib, n, tile, flags):
    vectors = fc.random_vectors(200 + n, 2, n)
    results = [run(lib, vectors, flags, s, tile)[0] for s in fc.SHIFTS]
    assert results == [fc.expected(vectors, flags, s) for s in fc.SHIFTS]
    assert results[1] == results[2] and results[2][1:] == (bytes(2), 0)      # r + 7 is 7, and the shift sets no status bit
    assert results[0] == run(lib, vectors, flags, None, tile)[0] != results[1]
    assert lib.emu_frntt(fc.pack(vectors), n, 2, flags, fc.le(R), 0, 0, None, None, None) == -1      # a zero shift


@pytest.mark.parametrize("flags", fc.FLAGS)
@pytest.mark.parametrize("n,tile", [(1, 0), (8, 0), (16, 2)])
def test_images_that_are_not_canonical(lib, n, tile, flags):
    rows = [list(v) for v in fc.random_vectors(300 + n, 5, n)]
    for g, image in enumerate(fc.NON_CANONICAL):
        rows[g + 1][(g * 3) % n] = image
    got, _ = run(lib, rows, flags, 7, tile)
    assert got == fc.expected(rows, flags, 7)
    assert got[1] == bytes([0, 2, 2, 2, 0]) and got[2] == 3 and all(v < R for v in fc.images(got[0]))


@pytest.mark.parametrize("bitrev", [0, fc.BITREV])
@pytest.mark.parametrize("n,tile", [(1, 0), (2, 0), (64, 2), (512, 0), (2048, 0)])
def test_inverse_of_forward_is_the_input_mod_r(lib, n, tile, bitrev):
    rows = [list(v) for v in fc.random_vectors(400 + n, 2, n)]
    rows[1][n - 1] = R + 5
    fwd, _ = run(lib, rows, bitrev, 7, tile)
    back, _ = run(lib, [fc.images(fwd[0])[g * n:(g + 1) * n] for g in range(2)], bitrev | fc.INVERSE, 7, tile)
    assert back[0] == fc.pack([[v % R for v in row] for row in rows]) and fwd[1] == bytes([0, 2]) and back[1] == bytes(2)
