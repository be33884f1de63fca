"""Openings of k polynomials over Fr on the device (mi355_bls_fr_open_many, host and device form) against Python integers mod r
(tests/fropen_cases.py): both forms at every size where the chunking changes with k = 1, 3 and 257, forced passes, chosen points and images,
the domain in both orders with z inside and outside it, the evaluation form against the coefficient form through an interpolation, canonical
outputs, NULL outputs and guard bands, and the C entry points' refusals.  The CPU half is tests/test_fropen_emu.py."""
import ctypes
import random

import pytest

import fropen_cases as fc

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


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def both_forms(m, cache, polys, zs, xs=None):
    """the host form and the device form (0xaa guard bands behind both outputs) -> the one result both gave: (ys, quot, status, count)"""
    import torch
    k, n = len(polys), len(polys[0])
    flags = m.FR_OPEN_EVAL if xs is not None else 0
    pb, zb, db = fc.pack(polys), fc.pack([zs]), fc.pack([xs]) if xs is not None else None
    cnt, ys, quot, st = m.frOpenMany(cache, pb, n, zb, flags, db)
    d_p, d_z, d_d = dev(pb), dev(zb), dev(db) if db else None
    d_y = torch.full((32 * k + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    d_q = torch.full((32 * k * n + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    got = m.frOpenMany_device(cache, d_p.data_ptr(), n, d_z.data_ptr(), k, flags, d_d.data_ptr() if db else None, d_y.data_ptr(), d_q.data_ptr())
    hy, hq = host(d_y), host(d_q)
    assert hy[32 * k:] == b"\xaa" * GUARD and hq[32 * k * n:] == b"\xaa" * GUARD
    assert (got[0], hy[:32 * k], hq[:32 * k * n], got[1]) == (cnt, ys, quot, st)
    return ys, quot, st, cnt


def pool_for(n, xs, seed):
    rng = random.Random(seed)
    if xs is None:
        return [rng.randrange(R), rng.randrange(R), 0]
    return [rng.randrange(R), xs[n // 2], rng.randrange(R)]          # three z: the reference inverts n differences for each, not for each polynomial


@pytest.mark.parametrize("k", [1, 3, 257])
@pytest.mark.parametrize("n", fc.N_BOTH)
def test_coefficient_form_sizes(m, cache, n, k):
    polys, zs = fc.random_call(1000 * k + n, n, k, pool_for(n, None, n))
    assert both_forms(m, cache, polys, zs) == fc.expected(polys, zs)


@pytest.mark.parametrize("k", [1, 3, 257])
@pytest.mark.parametrize("n", fc.N_EVAL)
def test_evaluation_form_sizes(m, cache, n, k):
    xs = fc.domain(n)
    polys, zs = fc.random_call(2000 * k + n, n, k, pool_for(n, xs, n))
    got = both_forms(m, cache, polys, zs, xs)
    assert got == fc.expected(polys, zs, xs)
    assert [b & fc.IN_DOMAIN for b in got[2]] == [int(g % 3 == 1) for g in range(k)]


@pytest.mark.parametrize("ev", [False, True])
def test_forced_passes_give_the_one_pass_bytes(m, cache, ev):
    n, k = 8, 5
    xs = fc.domain(n) if ev else None
    polys, zs = fc.random_call(5, n, k, [3, (xs[3] if ev else 4), R + 9, 11, 12])
    polys[4][2] = R + 1
    whole = both_forms(m, cache, polys, zs, xs)
    try:
        m.debug_fropen_set_pass(cache, 2)
        assert both_forms(m, cache, polys, zs, xs) == whole == fc.expected(polys, zs, xs)
    finally:
        m.debug_fropen_set_pass(cache, 0)
    assert whole[3] == 2 and whole[2] == bytes([0, int(ev), 2, 0, 2])


def chosen(n):
    rng = random.Random(7 * n)
    rows = [[0] * n, [R - 1] * n, [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]]
    rows[2][n // 2] = (1 << 256) - 1
    rows[3][n - 1] = R
    return rows


@pytest.mark.parametrize("n", [3, 257])
def test_chosen_points_and_images_coefficient_form(m, cache, n):
    for z in (0, 1, R - 1, R + 5):
        polys = chosen(n)
        got = both_forms(m, cache, polys, [z] * 4)
        assert got == fc.expected(polys, [z] * 4)
        assert got[2] == bytes([2 if z >= R else 0] * 2 + [2, 2]) and got[3] == (4 if z >= R else 2)      # the count is the return value
        assert all(v < R for v in fc.images(got[0]) + fc.images(got[1]))                                  # canonical
        assert fc.images(got[1])[:n] == [0] * n                                                           # the all-zero polynomial


@pytest.mark.parametrize("n", [2, 512])
def test_chosen_points_and_images_evaluation_form(m, cache, n):
    xs = fc.domain(n)
    for z in (0, 1, R - 1, R + 5, R + 1):                            # 1 and r - 1 lie in every domain from n = 2 on; r + 1 reduces INTO it
        polys = chosen(n)
        got = both_forms(m, cache, polys, [z] * 4, xs)
        assert got == fc.expected(polys, [z] * 4, xs)
        assert all(b & fc.IN_DOMAIN == int(z % R in (1, R - 1)) for b in got[2]) and got[3] == (4 if z >= R else 2)
        assert all(v < R for v in fc.images(got[0]) + fc.images(got[1]))


@pytest.mark.parametrize("bit_reversed", [False, True])
@pytest.mark.parametrize("n", [8, 256, 4096])
def test_domain_orders_and_points_in_the_domain(m, cache, n, bit_reversed):
    xs = fc.domain(n, bit_reversed)
    rng = random.Random(n)
    pool = [rng.randrange(R), xs[0], rng.randrange(R), xs[n - 1], xs[n // 3], rng.randrange(R)]
    polys, zs = fc.random_call(n + 1, n, len(pool), pool)
    got = both_forms(m, cache, polys, zs, xs)
    assert got == fc.expected(polys, zs, xs)
    assert [b & fc.IN_DOMAIN for b in got[2]] == [0, 1, 0, 1, 1, 0]  # exactly the polynomials opened inside the domain, among others that are not


@pytest.mark.parametrize("n", [8, 256])
def test_evaluation_quotient_is_the_coefficient_quotient_evaluated(m, cache, n):
    xs = fc.domain(n, True)
    random.Random(3).shuffle(xs)
    rng = random.Random(n)
    zs = [rng.randrange(R), xs[0], xs[n - 1], xs[5]]
    fs = [[rng.randrange(R) for _ in range(n)] for _ in zs]
    cs = [fc.interpolate(f, xs) for f in fs]
    ys_c, quot_c, _, _ = both_forms(m, cache, cs, zs)                # the coefficient route, on the device too
    ys_e, quot_e, st, _ = both_forms(m, cache, fs, zs, xs)
    assert ys_e == ys_c and st == bytes([0, 1, 1, 1])
    q_c = fc.images(quot_c)
    assert fc.images(quot_e) == [fc.evaluate(q_c[g * n:(g + 1) * n], x) for g in range(len(zs)) for x in xs]


def test_null_outputs_leave_the_others_unchanged(m, cache):
    import torch
    n, k = 16, 3
    for xs in (None, fc.domain(n)):
        flags = m.FR_OPEN_EVAL if xs else 0
        polys, zs = fc.random_call(9, n, k, [5, xs[2] if xs else 6, R + 7])
        want = fc.expected(polys, zs, xs)
        d_p, d_z, d_d = dev(fc.pack(polys)), dev(fc.pack([zs])), dev(fc.pack([xs])) if xs else None
        D = d_d.data_ptr() if xs else None
        d_y = torch.full((32 * k + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
        d_q = torch.full((32 * k * n + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
        assert m.frOpenMany_device(cache, d_p.data_ptr(), n, d_z.data_ptr(), k, flags, D, d_y.data_ptr(), None) == (1, want[2])
        assert host(d_y) == want[0] + b"\xaa" * GUARD and host(d_q) == b"\xaa" * (32 * k * n + GUARD)
        d_y.fill_(0xaa)
        assert m.frOpenMany_device(cache, d_p.data_ptr(), n, d_z.data_ptr(), k, flags, D, None, d_q.data_ptr(), want_status=False) == (1, None)
        assert host(d_q) == want[1] + b"\xaa" * GUARD and host(d_y) == b"\xaa" * (32 * k + GUARD)
        d_q.fill_(0xaa)
        assert m.frOpenMany_device(cache, d_p.data_ptr(), n, d_z.data_ptr(), k, flags, D, None, None) == (1, want[2])      # the status alone
        assert host(d_q) == b"\xaa" * (32 * k * n + GUARD) and host(d_y) == b"\xaa" * (32 * k + GUARD)
        assert m.frOpenMany(cache, fc.pack(polys), n, fc.pack([zs]), flags, fc.pack([xs]) if xs else None, want_quot=False) == (1, want[0], None, want[2])
        assert m.frOpenMany(cache, fc.pack(polys), n, fc.pack([zs]), flags, fc.pack([xs]) if xs else None, want_ys=False) == (1, None, want[1], want[2])


def test_argument_errors_with_a_context(m, cache):
    """MI355_BLS_ERR_ARG (-3) from the C entry points themselves (the Python mirror refuses most of these before the call); nothing is written"""
    import torch
    L, h = m.lib(), cache._h
    s = bytes(32)
    ys, quot, st = (ctypes.create_string_buffer(b"\x5a" * 32 * 4, 32 * 4) for _ in range(3))
    bad = [dict(polys=None), dict(zs=None), dict(n=0), dict(flags=2), dict(flags=0x80000001), dict(dom=s * 4), dict(flags=1), dict(flags=1, dom=s * 3, n=3),
           dict(ys=None, quot=None, st=None), dict(ys=None, quot=None)]
    for case in bad:
        a = dict(polys=s * 4, n=4, zs=s, flags=0, dom=None, ys=ys, quot=quot, st=st)
        a.update(case)
        assert L.mi355_bls_fr_open_many(h, a["polys"], a["n"], a["zs"], 1, a["flags"], a["dom"], a["ys"], a["quot"], a["st"]) == -3, case
    assert ys.raw == quot.raw == st.raw == b"\x5a" * 128
    assert L.mi355_bls_fr_open_many(h, s * 4, 4, s, 0, 0, None, ys, quot, st) == 0 and ys.raw == b"\x5a" * 128                  # k == 0: nothing written
    d_p, d_z, d_o = dev(s * 4 + bytes(4)), dev(s + bytes(4)), torch.zeros(32 * 5 + 4, dtype=torch.uint8, device="cuda")
    P, Z, O = d_p.data_ptr(), d_z.data_ptr(), d_o.data_ptr()
    call = lambda p, z, n=4, flags=0, dom=None, y=O, q=O + 32, stat=st: L.mi355_bls_fr_open_many_device(h, p, n, z, 1, flags, dom, y, q, stat, None)      # noqa: E731
    assert call(P, Z) == 0
    assert call(P + 1, Z) == -3 and call(P, Z + 2) == -3 and call(P, Z, y=O + 1) == -3 and call(P, Z, q=O + 34) == -3      # alignment
    assert call(P + 4, Z + 4) == 0                                                                                          # 4 bytes are enough
    assert call(None, Z) == -3 and call(P, None) == -3 and call(P, Z, n=0) == -3 and call(P, Z, flags=2) == -3
    assert call(P, Z, dom=P) == -3 and call(P, Z, flags=1) == -3 and call(P, Z, n=3, flags=1, dom=P) == -3
    assert call(P, Z, y=None, q=None, stat=None) == -3 and call(P, Z, y=None, q=None) == 0
    assert L.mi355_bls_fr_open_many_device(h, P, 4, Z, 0, 0, None, O, O + 32, st, None) == 0
    assert L.mi355_bls_debug_fropen_set_pass(h, 0) == 0
