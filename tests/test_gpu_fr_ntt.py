"""Transforms of k vectors over Fr on the device (mi355_bls_fr_ntt_many, host and device form, and mi355_bls_fr_domain) against Python integers
mod r (tests/frntt_cases.py): tile-only sizes and two passes at the default tile with k = 1, 3 and 257, a forced tile of four elements with
two and three passes, forced slices, every flag combination, coset shifts, images that are not canonical, in-place calls, one context
through changing lengths, and the domain in both orders.  The CPU half is tests/test_frntt_emu.py."""
import pytest

import fropen_cases as fo
import frntt_cases as fc

pytestmark = pytest.mark.gpu
R = fc.R
GUARD = 64


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tile():
    """the default tile, in elements, as csrc/plan.hpp has it"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nim-blscurve_amd", "csrc", "plan.hpp")).read()
    return 1 << int(re.search(r"FRNTT_TILE_LOG2 = (\d+)", src).group(1))


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def both_forms(m, cache, vectors, flags=0, shift=None, in_place=False):
    """the host form and the device form (a 0xaa guard band behind the output) -> the one result both gave: (out, status, count)"""
    import torch
    k, n = len(vectors), len(vectors[0])
    vb, sb = fc.pack(vectors), fc.le(shift) if shift is not None else None
    cnt, out, st = m.frNttMany(cache, vb, n, flags, sb)
    d_in = torch.full((32 * k * n + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    d_in[:32 * k * n] = dev(vb)
    d_out = d_in if in_place else torch.full((32 * k * n + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    got = m.frNttMany_device(cache, d_in.data_ptr(), n, k, flags, sb, None if in_place else d_out.data_ptr())
    ho = host(d_out)
    assert ho[32 * k * n:] == b"\xaa" * GUARD
    if not in_place:
        assert host(d_in)[:32 * k * n] == vb                       # the input is left as it was
    assert (got[0], ho[:32 * k * n], got[1]) == (cnt, out, st)
    return out, st, cnt


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 4, 256, 512, "tile", "2 tiles"])
def test_sizes_at_the_default_tile(m, cache, tile, n, k):
    n = {"tile": tile, "2 tiles": 2 * tile}.get(n, n)
    vectors = fc.random_vectors(1000 * k + n, k, n)
    assert both_forms(m, cache, vectors) == fc.expected(vectors)


@pytest.mark.parametrize("n", [2, 16])
def test_many_short_vectors(m, cache, n):
    vectors = fc.random_vectors(n, 257, n)
    for flags in (0, fc.INVERSE | fc.BITREV):
        assert both_forms(m, cache, vectors, flags) == fc.expected(vectors, flags)


def test_one_long_vector(m, cache):
    vectors = fc.random_vectors(65536, 1, 65536)
    assert both_forms(m, cache, vectors) == fc.expected(vectors)


@pytest.mark.parametrize("n", [4, 8, 16, 64])
def test_forced_tile_of_four_elements(m, cache, n):
    vectors = fc.random_vectors(100 + n, 3, n)
    try:
        m.debug_frntt_set_tile(cache, 2)
        for flags in fc.FLAGS:
            assert both_forms(m, cache, vectors, flags) == fc.expected(vectors, flags), flags
    finally:
        m.debug_frntt_set_tile(cache, 0)


def test_forced_slices_give_the_one_slice_bytes(m, cache, tile):
    for n in (8, 2 * tile):
        rows = [list(v) for v in fc.random_vectors(5 + n, 5, n)]
        rows[4][2] = R + 1
        whole = both_forms(m, cache, rows, 0, 7)
        try:
            m.debug_frntt_set_pass(cache, 2)
            assert both_forms(m, cache, rows, 0, 7) == whole == fc.expected(rows, 0, 7)
        finally:
            m.debug_frntt_set_pass(cache, 0)
        assert whole[1] == bytes([0, 0, 0, 0, 2]) and whole[2] == 1


@pytest.mark.parametrize("flags", fc.FLAGS)
@pytest.mark.parametrize("n", [8, "2 tiles"])
def test_flag_combinations(m, cache, tile, n, flags):
    n = 2 * tile if n == "2 tiles" else n
    vectors = fc.random_vectors(7, 3, n)
    assert both_forms(m, cache, vectors, flags) == fc.expected(vectors, flags)


@pytest.mark.parametrize("flags", fc.FLAGS)
def test_shifts(m, cache, flags):
    vectors = fc.random_vectors(216, 2, 16)
    results = [both_forms(m, cache, vectors, flags, s) for s in fc.SHIFTS]
    assert results == [fc.expected(vectors, flags, s) for s in fc.SHIFTS]
    assert results[1] == results[2] and results[2][1:] == (bytes(2), 0)      # r + 7 is 7, and the shift sets no status bit
    assert results[0] == both_forms(m, cache, vectors, flags) != results[1]


@pytest.mark.parametrize("flags", fc.FLAGS)
def test_images_that_are_not_canonical(m, cache, flags):
    for n in (1, 8):
        rows = [list(v) for v in fc.random_vectors(300 + n, 5, n)]
        for g, image in enumerate(fc.NON_CANONICAL):
            rows[g + 1][(g * 3) % n] = image
        got = both_forms(m, cache, rows, flags, 7)
        assert got == fc.expected(rows, flags, 7)
        assert got[1] == bytes([0, 2, 2, 2, 0]) and got[2] == 3 and all(v < R for v in fc.images(got[0]))


@pytest.mark.parametrize("flags", fc.FLAGS)
@pytest.mark.parametrize("n", [8, "2 tiles"])
def test_in_place(m, cache, tile, n, flags):
    n = 2 * tile if n == "2 tiles" else n
    vectors = fc.random_vectors(7, 3, n)
    assert both_forms(m, cache, vectors, flags, 7, in_place=True) == fc.expected(vectors, flags, 7)


def test_one_context_through_changing_lengths(m, cache):
    for n in (8, 16, 8):
        for flags in (0, fc.INVERSE):
            vectors = fc.random_vectors(40 + n, 2, n)
            assert both_forms(m, cache, vectors, flags) == fc.expected(vectors, flags), (n, flags)


@pytest.mark.parametrize("n", [1, 2, 4096])
def test_the_domain_in_both_orders(m, cache, n):
    import torch
    for flags, bitrev in ((0, False), (m.FR_NTT_BITREV, True)):
        want = fo.pack([fo.domain(n, bitrev)])
        assert m.frDomain(cache, n, flags) == want
        d = torch.full((32 * n + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
        m.frDomain_device(cache, n, d.data_ptr(), flags)
        assert host(d) == want + b"\xaa" * GUARD


def test_argument_errors_with_a_context(m, cache):
    """MI355_BLS_ERR_ARG (-3) from the C entry points themselves; nothing is written"""
    import ctypes
    import torch
    L, h = m.lib(), cache._h
    s = bytes(32)
    out, st = ctypes.create_string_buffer(b"\x5a" * 128, 128), ctypes.create_string_buffer(b"\x5a" * 4, 4)
    for case in (dict(vin=None), dict(out=None), dict(n=0), dict(n=3), dict(n=1 << 33), dict(flags=4), dict(flags=0x80000001), dict(shift=s), dict(shift=fc.le(R))):
        a = dict(vin=s * 4, n=4, flags=0, shift=None, out=out)
        a.update(case)
        assert L.mi355_bls_fr_ntt_many(h, a["vin"], a["n"], 1, a["flags"], a["shift"], a["out"], st) == -3, case
    assert L.mi355_bls_fr_ntt_many(h, s * 4, 4, 0, 0, None, out, st) == 0 and out.raw == b"\x5a" * 128 and st.raw == b"\x5a" * 4      # k == 0
    d = torch.zeros(32 * 4 + 8, dtype=torch.uint8, device="cuda")
    P = d.data_ptr()
    call = lambda p, o, n=4, flags=0, shift=None: L.mi355_bls_fr_ntt_many_device(h, p, n, 1, flags, shift, o, st, None)      # noqa: E731
    assert call(P, P) == 0 and call(P + 4, P + 4) == 0                                                   # 4 bytes are enough
    assert call(P + 1, P) == -3 and call(P, P + 2) == -3 and call(None, P) == -3 and call(P, None) == -3
    assert call(P, P, n=0) == -3 and call(P, P, n=6) == -3 and call(P, P, flags=8) == -3 and call(P, P, shift=s) == -3
    assert L.mi355_bls_fr_domain(h, 3, 0, out) == -3 and L.mi355_bls_fr_domain(h, 4, 1, out) == -3 and L.mi355_bls_fr_domain(h, 4, 0, None) == -3
    assert L.mi355_bls_fr_domain_device(h, 4, 0, P + 2, None) == -3 and L.mi355_bls_fr_domain_device(h, 4, 2, P, None) == 0
    assert out.raw == b"\x5a" * 128
