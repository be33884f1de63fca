"""Transforms of k vectors of G1 points on the device (mi355_bls_p1s_ntt_many, host and device form): every case of tests/golden/p1ntt.json
in place and not in place, larger sizes through the defining property - the transform of [a_j]G is [fr_ntt(a)_i]G, both sides made by
p1sLincombMany_device over a one-row table of G - the round trip, many short vectors, forced slices, one context through changing lengths,
a finish over more than TOAFF_DEVICE_LANES elements (neighbours share an inversion), and the argument errors of the C entry points.  The
CPU half is tests/test_p1ntt_emu.py."""
import functools

import pytest

import fk20_levels_cases as lc
import frntt_cases as fc
import p1ntt_cases as pc
from g1_images import multiples_of_g

pytestmark = pytest.mark.gpu
R = pc.R
ROW = pc.ROW
GUARD = 96


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


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def both_forms(m, cache, images, n, flags=0, in_place=False):
    """the host form and the device form (a 0xaa guard band behind the output; the input untouched when not in place) -> the one result"""
    import torch
    size = len(images)
    k = size // (ROW * n)
    out = m.p1sNttMany(cache, images, n, flags)
    d_in = torch.full((size + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    d_in[:size] = dev(images)
    d_out = d_in if in_place else torch.full((size + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    m.p1sNttMany_device(cache, d_in.data_ptr(), n, k, flags, None if in_place else d_out.data_ptr())
    ho = host(d_out)
    assert ho[size:] == b"\xaa" * GUARD
    if not in_place:
        assert host(d_in)[:size] == images                         # the input is left as it was
    assert ho[:size] == out
    return out


@functools.lru_cache(maxsize=None)
def _property_inputs(n, k):
    return fc.random_vectors(7000 + n + k, k, n)


@pytest.mark.parametrize("in_place", [False, True])
def test_every_case_of_the_fixture(m, cache, in_place):
    for name, n, k, flags, images, want in pc.cases():
        got = both_forms(m, cache, images, n, flags, in_place)
        for i, (a, b) in enumerate(zip(pc.rows(got), pc.rows(want))):
            assert a == b, (name, flags, i)


@pytest.mark.parametrize("n,k", [(256, 1), (256, 3), (1024, 1)])
def test_larger_sizes_through_the_defining_property(m, cache, n, k):
    vectors = _property_inputs(n, k)
    images = multiples_of_g(m, cache, [a for v in vectors for a in v])
    for flags in pc.FLAGS:
        want = multiples_of_g(m, cache, [a for v in pc.expected_scalars(vectors, flags) for a in v])
        assert both_forms(m, cache, images, n, flags) == want, flags


def test_round_trip(m, cache):
    n, k = 512, 2
    images = multiples_of_g(m, cache, [a for v in fc.random_vectors(512, k, n) for a in v])
    for br in (0, pc.BITREV):
        there = both_forms(m, cache, images, n, br)
        assert there != images and both_forms(m, cache, there, n, br | pc.INVERSE, in_place=True) == images


@pytest.mark.parametrize("n", [2, 16])
def test_many_short_vectors(m, cache, n):
    k = 257
    vectors = fc.random_vectors(n, k, n)
    images = multiples_of_g(m, cache, [a for v in vectors for a in v])
    for flags in (0, pc.INVERSE | pc.BITREV):
        want = multiples_of_g(m, cache, [a for v in pc.expected_scalars(vectors, flags) for a in v])
        assert both_forms(m, cache, images, n, flags) == want, flags


@pytest.mark.parametrize("flags", [0, pc.INVERSE | pc.BITREV])
def test_finish_with_a_shared_inversion(m, cache, flags):
    """k = 1025 vectors of 64 points, three distinct ones cycled: 65 600 elements, more than TOAFF_DEVICE_LANES, so a lane of
    k_p1ntt_finish inverts once for two neighbours - all finite (a random vector), a finite one beside infinity and infinities alone (a
    constant vector: one output is no infinity), and infinities on the input side (a vector of one entry)"""
    n, k = 64, 1025
    assert k * n > lc.toaff_device_lanes() and k * n <= 2 * lc.toaff_device_lanes()
    vectors = [list(fc.random_vectors(6464, 1, n)[0]), [fc.random_vectors(6465, 1, 1)[0][0]] * n, [0] * 5 + [fc.random_vectors(6466, 1, 1)[0][0]] + [0] * (n - 6)]
    want = pc.expected_scalars(vectors, flags)
    assert all(want[0]) and sum(1 for a in want[1] if a) == 1 and all(want[2])
    rows = lambda scalars: [b"".join(pc.rows(multiples_of_g(m, cache, v))) for v in scalars]      # noqa: E731
    got = both_forms(m, cache, lc.cycled(rows(vectors), k), n, flags)
    expected = lc.cycled(rows(want), k)
    assert got == expected, [i for i, (a, b) in enumerate(zip(pc.rows(got), pc.rows(expected))) if a != b][:8]


def test_forced_slices_give_the_one_slice_bytes(m, cache):
    n, k = 8, 5
    vectors = fc.random_vectors(58, k, n)
    images = multiples_of_g(m, cache, [a for v in vectors for a in v])
    for flags in pc.FLAGS:
        whole = both_forms(m, cache, images, n, flags)
        try:
            m.debug_p1ntt_set_pass(cache, 2)
            assert both_forms(m, cache, images, n, flags) == whole
            assert both_forms(m, cache, images, n, flags, in_place=True) == whole
        finally:
            m.debug_p1ntt_set_pass(cache, 0)
        assert whole == multiples_of_g(m, cache, [a for v in pc.expected_scalars(vectors, flags) for a in v])


def test_one_context_through_changing_lengths(m, cache):
    by = {(name, flags): (images, want) for name, n, k, flags, images, want in pc.cases()}
    for n in (8, 16, 8):
        for flags in (0, pc.INVERSE):
            images, want = by["n%d_k3" % n, flags]
            assert both_forms(m, cache, images, n, flags) == want, (n, flags)


def test_argument_errors_with_a_context(m, cache):
    """MI355_BLS_ERR_ARG (-3) from the C entry points themselves; nothing is written"""
    import ctypes
    import torch
    L, h = m.lib(), cache._h
    p = bytes(ROW)
    out = ctypes.create_string_buffer(b"\x5a" * 4 * ROW, 4 * ROW)
    for case in (dict(pin=None), dict(out=None), dict(n=0), dict(n=3), dict(n=1 << 33), dict(flags=4), dict(flags=0x80000001)):
        a = dict(pin=p * 4, n=4, flags=0, out=out)
        a.update(case)
        assert L.mi355_bls_p1s_ntt_many(h, a["pin"], a["n"], 1, a["flags"], a["out"]) == -3, case
    assert L.mi355_bls_p1s_ntt_many(h, p * 4, 4, 0, 0, out) == 0 and out.raw == b"\x5a" * 4 * ROW                # k == 0
    d = torch.full((ROW * 4 + 8,), 0x5a, dtype=torch.uint8, device="cuda")
    before = host(d)
    P = d.data_ptr()
    call = lambda pi, po, n=4, k=1, flags=0: L.mi355_bls_p1s_ntt_many_device(h, pi, n, k, flags, po, None)      # noqa: E731
    assert call(P + 1, P) == -3 and call(P, P + 2) == -3 and call(None, P) == -3 and call(P, None) == -3
    assert call(P, P, n=0) == -3 and call(P, P, n=6) == -3 and call(P, P, n=(1 << 32) + 1) == -3 and call(P, P, flags=8) == -3
    assert call(P, P, k=0) == 0 and call(None, None, n=3, k=0, flags=9) == 0                                       # k == 0 touches nothing
    assert host(d) == before
    d[:] = 0                                                                                                      # four points at infinity
    assert call(P, P) == 0 and call(P + 4, P + 4) == 0                                                            # aligned to 4 bytes, not to 16
    assert host(d) == bytes(ROW * 4 + 8)
    assert out.raw == b"\x5a" * 4 * ROW


def test_a_busy_context_is_refused(m):
    """a context with a submitted batch that has not been waited for: -3 before anything is launched, the output untouched"""
    import ctypes
    import json
    import os
    import torch
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch.json")))
    case = [c for c in g["cases"] if c["name"] == "n3"][0]
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        L = m.lib()
        recs = dev(bytes.fromhex(case["sets"]))
        d = torch.full((ROW * 4,), 0x5a, dtype=torch.uint8, device="cuda")
        out = ctypes.create_string_buffer(b"\x5a" * 4 * ROW, 4 * ROW)
        c.submit_device(recs.data_ptr(), case["n"], bytes.fromhex(case["rnd"]))
        assert L.mi355_bls_p1s_ntt_many_device(c._h, d.data_ptr(), 4, 1, 0, d.data_ptr(), None) == -3
        assert L.mi355_bls_p1s_ntt_many(c._h, bytes(4 * ROW), 4, 1, 0, out) == -3
        assert b"not been waited for" in L.mi355_bls_last_error()
        assert c.wait() is True
        assert host(d) == out.raw == b"\x5a" * 4 * ROW
        assert L.mi355_bls_p1s_ntt_many(c._h, bytes(4 * ROW), 4, 1, 0, out) == 0 and out.raw == bytes(4 * ROW)
    finally:
        c.close()
