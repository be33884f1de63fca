"""GPU parity of the fixed-base table MSM (mi355_bls_p1s_table_* / mi355_bls_p1s_mult_table*): the table's rows byte for byte against the
oracle's affine [2^(w wbits)] P_i, the mult calls against the generic Pippenger call on the same arrays and against the C oracle, exceptional
operands in the buckets and the final sum, table reuse across nbits and contexts, k MSMs over one table, every number of bucket sets the plan
can choose and both sides of its hand-overs, calls cut into passes, resource accounting, and the refusals.  Results are compared as points."""
import ctypes
import random

import pytest

import bls12381_py as o
from test_msm_table_plan import call_plan, windows
from util import g1_jac_to_affine

pytestmark = pytest.mark.gpu
ERR_ARG = -3


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    return m.BatchedBLSVerifierCache.init(max_sets=64)


@pytest.fixture(scope="module")
def base():
    """a few hundred distinct points, repeated by every test (tests/test_gpu_msm.py _bench_points)"""
    import c_oracle as co
    rng = random.Random(1234)
    return [co.sk_to_pk(rng.getrandbits(96) | 1) for _ in range(300)]


@pytest.fixture(scope="module")
def slots():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def points(base, n, first=0):
    return b"".join(base[(first + i) % len(base)] for i in range(n))


def scalars(rng, n, nbits=256):
    return b"".join(rng.getrandbits(nbits).to_bytes(32, "little") for _ in range(n))


def affine(outs):
    assert all(len(b) == 144 for b in outs)
    return [o.g1_to_blst_affine(g1_jac_to_affine(b)) for b in outs]


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def generic(m, cache, pts, sc, nbits):
    dp, ds = on_device(pts), on_device(sc)
    return m.p1s_mult_pippenger_device(cache, dp.data_ptr(), len(pts) // 96, ds.data_ptr(), nbits)


def refused(m, fn, *args):
    with pytest.raises(m.BlsGpuError, match="error %d" % ERR_ARG):
        fn(*args)


# ---- 1. rows
@pytest.fixture(scope="module")
def doublings():
    """[2^t] P for t = 0 .. 256 of seven points, by repeated doubling with the Python oracle (shared by the row tests)"""
    rng = random.Random(5)
    out = []
    for _ in range(7):
        q = o.g1_mul(o.G1_GEN, rng.randrange(1, o.R))
        chain = [q]
        for _ in range(256):
            q = o.g1_add(q, q)
            chain.append(q)
        out.append(chain)
    return out


@pytest.mark.parametrize("n", [5, 65])
def test_rows_equal_the_oracles_multiples(m, cache, doublings, n):
    """5 points, one at infinity; 65: a second wave, partly filled.  Every row byte for byte."""
    which = [i % 7 if i % 4 != 3 else None for i in range(n)]
    pts = b"".join(bytes(96) if b is None else o.g1_to_blst_affine(doublings[b][0]) for b in which)
    for wbits in (5, 16):
        for nbits in (255, 256):
            W = windows(wbits, nbits)
            assert m.p1s_table_sizeof(n, wbits, nbits) == W * n * 128
            tab = m.p1s_table_create(cache, pts, wbits, nbits)
            try:
                got = m.debug_p1s_table_rows(tab, 0, W, 0, n)
                for w in range(W):
                    want = [bytes(96) if b is None else o.g1_to_blst_affine(doublings[b][w * wbits]) for b in which]
                    assert got[w] == want, (wbits, nbits, w)
                # a rectangle inside the table
                sub = m.debug_p1s_table_rows(tab, 1, 2, 1, 3)
                assert sub == [got[1][1:4], got[2][1:4]]
            finally:
                tab.destroy()


# ---- 2. against the generic call and the C oracle
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_against_the_generic_call_and_the_c_oracle(m, cache, base, n):
    import c_oracle as co
    rng = random.Random(n)
    pts = points(base, n)
    dp = on_device(pts)
    for nbits in (1, 5, 64, 255, 256):
        sets = {"zero": bytes(32 * n), "one": (1).to_bytes(32, "little") * n, "ones": ((1 << nbits) - 1).to_bytes(32, "little") * n, "random": scalars(rng, n)}
        want = {name: co.msm_g1(pts, sc, nbits) for name, sc in sets.items()}
        gen = {name: affine([generic(m, cache, pts, sc, nbits)])[0] for name, sc in sets.items()}
        assert gen == want
        for wbits in (0, 5, 8, 13, 16):
            tab = m.p1s_table_create_device(cache, dp.data_ptr(), n, wbits, nbits)
            try:
                for name, sc in sets.items():
                    ds = on_device(sc)
                    got = m.p1s_mult_table_device(cache, tab, ds.data_ptr(), nbits)
                    assert affine([got])[0] == want[name], (nbits, wbits, name)
                    if name == "zero":
                        assert got == bytes(144)                                       # an infinite result: 144 zero bytes
                assert affine([m.p1s_mult_table(cache, tab, sets["random"], nbits)])[0] == want["random"]      # the host entry
            finally:
                tab.destroy()


# ---- 3. exceptional operands
def test_buckets_and_sums_meet_equal_and_opposite_operands(m, cache):
    """Repeated points under equal scalars (a bucket adds P to P: the doubling branch), P and -P under equal scalars (a bucket sums to
    infinity, and so does the whole MSM), a point at infinity with a non-zero scalar, and test_msm_tail_meets_equal_and_opposite_operands'
    constructions: [2^c] P + 2^c P and [2^c] P - 2^c P make the sets' values equal or opposite whatever wbits the table has."""
    rng = random.Random(91)
    P = o.g1_mul(o.G1_GEN, rng.randrange(1, o.R))
    G = o.g1_mul(o.G1_GEN, rng.randrange(1, o.R))
    le = lambda k: k.to_bytes(32, "little")
    s = rng.getrandbits(255)
    cases = [
        ([P, P, P, G], [s, s, s, 5]),
        ([P, o.g1_neg(P)], [s, s]),
        ([P, o.g1_neg(P), None], [s, s, rng.getrandbits(255)]),
        ([None, G], [rng.getrandbits(255), 3]),
        ([P, o.g1_neg(P), P, o.g1_neg(P)], [1, 1, (1 << 255) - 1, (1 << 255) - 1]),
    ]
    for c in (5, 8, 13, 16):
        Q = o.g1_mul(P, 1 << c)
        cases += [([P, Q], [1 << c, 1]), ([P, o.g1_neg(Q)], [1 << c, 1]), ([P, Q], [1 << c, 0]), ([P, Q, P], [1 << c, 1, (1 << c) + 1])]
    for pts, ks in cases:
        raw = b"".join(o.g1_to_blst_affine(q) for q in pts)
        sc = b"".join(map(le, ks))
        for wbits in (5, 8, 13, 16):
            tab = m.p1s_table_create(cache, raw, wbits, 255)
            try:
                for nbits in (64, 255):
                    want = o.msm_g1(pts, ks, nbits)
                    got = m.p1s_mult_table(cache, tab, sc, nbits)
                    assert g1_jac_to_affine(got) == want, (ks, wbits, nbits)
                    if want is None:
                        assert got == bytes(144)
            finally:
                tab.destroy()
    assert o.msm_g1(*cases[1], 255) is None and o.msm_g1(*cases[2], 255) is None and o.msm_g1(*cases[4], 255) is None


# ---- 4. table reuse
def test_a_table_serves_smaller_nbits_and_other_contexts(m, cache, base):
    n = 65
    rng = random.Random(4)
    pts, sc = points(base, n), scalars(rng, n)
    tab = m.p1s_table_create(cache, pts, 8, 256)
    other = m.BatchedBLSVerifierCache.init(max_sets=64)
    try:
        for nbits in (1, 64, 255, 256):
            want = affine([generic(m, cache, pts, sc, nbits)])
            assert affine([m.p1s_mult_table(cache, tab, sc, nbits)]) == want, nbits
            assert m.debug_p1s_table_last_plan(cache)[0] == windows(8, nbits)          # the call's windows, not the table's
            assert affine([m.p1s_mult_table(other, tab, sc, nbits)]) == want, nbits    # a table made through one context, used through another
    finally:
        other.close()
        tab.destroy()
    small = m.p1s_table_create(cache, pts, 8, 64)
    try:
        assert affine([m.p1s_mult_table(cache, small, sc, 64)]) == affine([generic(m, cache, pts, sc, 64)])
        refused(m, m.p1s_mult_table, cache, small, sc, 65)
    finally:
        small.destroy()


# ---- 5. many
@pytest.mark.parametrize("k", [1, 2, 9])
def test_many_over_one_table(m, cache, base, k):
    import torch
    n = 65
    rng = random.Random(50 + k)
    pts, sc = points(base, n), scalars(rng, k * n)
    tab = m.p1s_table_create(cache, pts, 0, 255)
    try:
        ds = on_device(sc)
        d_out = torch.full((k * 144,), 0xaa, dtype=torch.uint8, device="cuda")
        got = m.p1s_mult_table_many_device(cache, tab, ds.data_ptr(), k, 255, d_out=d_out.data_ptr())
        assert bytes(d_out.cpu().numpy()) == b"".join(got)                            # ret and d_out agree
        singles = [m.p1s_mult_table(cache, tab, sc[32 * n * j:32 * n * (j + 1)], 255) for j in range(k)]
        gen = [generic(m, cache, pts, sc[32 * n * j:32 * n * (j + 1)], 255) for j in range(k)]
        assert affine(got) == affine(singles) == affine(gen)
        assert affine(m.p1s_mult_table_many(cache, tab, sc, 255)) == affine(gen)      # the host entry
        # k = 0 touches nothing
        assert m.p1s_mult_table_many_device(cache, tab, ds.data_ptr(), 0, 255, d_out=d_out.data_ptr()) == []
        assert bytes(d_out.cpu().numpy()) == b"".join(got)
    finally:
        tab.destroy()


# ---- 6. bucket sets
def test_every_number_of_sets_and_both_sides_of_every_hand_over(m, cache, base, slots):
    """The plan's own S over k at 13- and 16-bit windows (the smallest shapes at each side of each change of S, read off the plan), then every
    S from 1 to W forced through the test hook on a 5-bit table, where W = 52 (the plan alone reaches them only with more buckets)."""
    n, nbits = 3, 255
    rng = random.Random(6)
    pts = points(base, n)
    for wbits in (13, 16):
        W = windows(wbits, nbits)
        S_of = lambda k: call_plan(n, wbits, nbits, k, slots=slots)[0]["S"]
        ks = sorted({kk for k in range(1, 40) if S_of(k) != S_of(k + 1) for kk in (k, k + 1)})
        assert len(ks) >= 4 and S_of(ks[-1]) == 1 and S_of(1) == min(W, -(-2 * slots * 64 // (1 << (wbits - 1))))
        tab = m.p1s_table_create(cache, pts, wbits, nbits)
        try:
            for k in ks:
                sc = scalars(rng, k * n)
                got = m.p1s_mult_table_many(cache, tab, sc, nbits)
                assert m.debug_p1s_table_last_plan(cache) == (W, S_of(k), 1 << (wbits - 1)), (wbits, k)
                assert affine(got) == affine([generic(m, cache, pts, sc[32 * n * j:32 * n * (j + 1)], nbits) for j in range(k)]), (wbits, k)
        finally:
            tab.destroy()
    W = windows(5, nbits)
    tab = m.p1s_table_create(cache, pts, 5, nbits)
    try:
        sc = scalars(rng, 2 * n)
        want = affine([generic(m, cache, pts, sc[32 * n * j:32 * n * (j + 1)], nbits) for j in range(2)])
        for S in range(1, W + 1):
            m.debug_p1s_table_set_plan(cache, force_sets=S)
            assert affine(m.p1s_mult_table_many(cache, tab, sc, nbits)) == want, S
            assert m.debug_p1s_table_last_plan(cache) == (W, S, 16)
    finally:
        m.debug_p1s_table_set_plan(cache)
        tab.destroy()


# ---- 7. passes
def test_a_call_cut_into_passes_equals_the_uncut_one(m, cache, base):
    n, k = 65, 9
    rng = random.Random(7)
    pts, sc = points(base, n), scalars(rng, k * n)
    tab = m.p1s_table_create(cache, pts, 8, 255)
    try:
        uncut = affine(m.p1s_mult_table_many(cache, tab, sc, 255))
        assert len(call_plan(n, 8, 255, k, pairs_max=130)[1]) == 5 and len(call_plan(n, 8, 255, k)[1]) == 1
        for bound in (130, 10):                                                        # two MSMs per pass; one
            m.debug_p1s_table_set_plan(cache, pairs_max=bound)
            assert affine(m.p1s_mult_table_many(cache, tab, sc, 255)) == uncut, bound
        assert uncut == affine([generic(m, cache, pts, sc[32 * n * j:32 * n * (j + 1)], 255) for j in range(k)])
    finally:
        m.debug_p1s_table_set_plan(cache)
        tab.destroy()


# ---- 8. resources
def test_live_resources_return_to_their_start(m, base):
    live = m.lib().mi355_bls_debug_live_resources
    rng = random.Random(8)
    pts, sc = points(base, 5), scalars(rng, 5)
    start = live()
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    with_ctx = live()
    tab = m.p1s_table_create(c, pts, 8, 255)
    m.p1s_mult_table(c, tab, sc, 255)
    assert live() > with_ctx
    tab.destroy()
    c.close()
    assert live() == start
    # the context first, the table second: the table survives its maker
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    tab = m.p1s_table_create(c, pts, 8, 255)
    c.close()
    assert live() == start + 1                                                        # the table's rows
    c2 = m.BatchedBLSVerifierCache.init(max_sets=64)
    assert g1_jac_to_affine(m.p1s_mult_table(c2, tab, sc, 255)) is not None
    c2.close()
    m.p1s_table_destroy(tab)
    m.p1s_table_destroy(tab)                                                          # again, and None: no-ops
    m.p1s_table_destroy(None)
    m.lib().mi355_bls_p1s_table_destroy(None)
    assert live() == start


# ---- 9. refusals
def test_refusals_come_before_anything_is_launched(m, cache, base):
    L = m.lib()
    live = L.mi355_bls_debug_live_resources
    pts, sc = points(base, 5), bytes(32 * 5)
    out, h = ctypes.create_string_buffer(144), ctypes.c_void_p()
    tab = m.p1s_table_create(cache, pts, 8, 64)
    start = live()
    plan_before = m.debug_p1s_table_last_plan(cache)
    try:
        for n, wbits, nbits in ((0, 8, 255), (5, 4, 255), (5, 17, 255), (5, 1, 255), (5, 8, 0), (5, 8, 257), ((1 << 31) // 16 + 1, 16, 255)):
            assert L.mi355_bls_p1s_table_create(cache._h, ctypes.byref(h), pts, n, wbits, nbits) == ERR_ARG, (n, wbits, nbits)
            assert L.mi355_bls_p1s_table_create_device(cache._h, ctypes.byref(h), 16, n, wbits, nbits, None) == ERR_ARG
            assert L.mi355_bls_p1s_table_sizeof(n, wbits, nbits) == 0 and not h
        assert L.mi355_bls_p1s_table_sizeof((1 << 31) // 16, 16, 255) == (1 << 31) * 128                 # the bound itself is a table
        assert L.mi355_bls_p1s_table_create(None, ctypes.byref(h), pts, 5, 8, 255) == ERR_ARG
        assert L.mi355_bls_p1s_table_create(cache._h, None, pts, 5, 8, 255) == ERR_ARG
        assert L.mi355_bls_p1s_table_create(cache._h, ctypes.byref(h), None, 5, 8, 255) == ERR_ARG
        assert L.mi355_bls_p1s_table_create_device(cache._h, ctypes.byref(h), None, 5, 8, 255, None) == ERR_ARG
        assert L.mi355_bls_p1s_mult_table(None, out, tab._h, sc, 64) == ERR_ARG
        assert L.mi355_bls_p1s_mult_table(cache._h, None, tab._h, sc, 64) == ERR_ARG
        assert L.mi355_bls_p1s_mult_table(cache._h, out, None, sc, 64) == ERR_ARG
        assert L.mi355_bls_p1s_mult_table(cache._h, out, tab._h, None, 64) == ERR_ARG
        for nbits in (0, 65, 257):
            assert L.mi355_bls_p1s_mult_table(cache._h, out, tab._h, sc, nbits) == ERR_ARG, nbits
            assert L.mi355_bls_p1s_mult_table_device(cache._h, out, tab._h, 16, nbits, None) == ERR_ARG
            assert L.mi355_bls_p1s_mult_table_many(cache._h, out, tab._h, sc, 1, nbits) == ERR_ARG
        assert L.mi355_bls_p1s_mult_table_many_device(cache._h, None, None, tab._h, 16, 1, 64, None) == ERR_ARG          # no output
        assert L.mi355_bls_p1s_mult_table_many_device(None, out, None, tab._h, 16, 0, 64, None) == ERR_ARG              # a NULL context before k == 0
        assert L.mi355_bls_p1s_mult_table_many_device(cache._h, None, None, None, None, 0, 999, None) == 0               # k == 0 touches nothing
        assert L.mi355_bls_debug_p1s_table_rows(tab._h, 0, windows(8, 64) + 1, 0, 1, out) == ERR_ARG
        assert L.mi355_bls_debug_p1s_table_rows(tab._h, 0, 1, 5, 1, out) == ERR_ARG
        assert live() == start and m.debug_p1s_table_last_plan(cache) == plan_before   # nothing was allocated, no plan was made
    finally:
        tab.destroy()
