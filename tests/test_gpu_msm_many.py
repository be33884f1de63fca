"""GPU parity of k G1 MSMs in one device pass (mi355_bls_p1s_mult_pippenger_many / _many_device) against the oracles' MSM of every member
alone: both addressing forms, both entries, neighbours that must not leak into each other, the per-MSM tail's exceptional additions, both
sides of every hand-over of the plan, calls cut into passes, and k = 1.  Results are compared on the canonical affine image."""
import random

import pytest

import bls12381_py as o
from test_msm_many_plan import call_plan, constants
from util import g1_jac_to_affine

pytestmark = pytest.mark.gpu
RAGGED = [0, 1, 2, 31, 32, 33, 0, 1000, 1]


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


def points(base, n, first=0):
    return b"".join(base[(first + i) % len(base)] for i in range(n))


def scalars(rng, n, nbits=256):
    return b"".join(rng.getrandbits(nbits).to_bytes(32, "little") for _ in range(n))


def affine(outs):
    assert all(len(b) == 144 for b in outs)
    return [o.g1_to_blst_affine(g1_jac_to_affine(b)) for b in outs]


def offsets_of(lengths):
    acc = [0]
    for v in lengths:
        acc.append(acc[-1] + v)
    return acc


def want_ragged(pts, sc, lengths, nbits, pippenger=False):
    import c_oracle as co
    fn = co.msm_g1_pippenger if pippenger else co.msm_g1
    offs = offsets_of(lengths)
    return [fn(pts[96 * a:96 * b], sc[32 * a:32 * b], nbits) if b > a else bytes(96) for a, b in zip(offs, offs[1:])]


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


def test_ragged_smallest_shapes(m, cache, base):
    import torch
    rng = random.Random(1)
    n, k = sum(RAGGED), len(RAGGED)
    pts, offs = points(base, n), offsets_of(RAGGED)
    for nbits in (255, 1, 64, 256):
        sc = scalars(rng, n)
        want = want_ragged(pts, sc, RAGGED, nbits)
        got = m.p1s_mult_pippenger_many(cache, pts, sc, offs, nbits)
        assert affine(got) == want, nbits
        for j, v in enumerate(RAGGED):
            if v == 0:
                assert got[j] == bytes(144), (nbits, j)                               # empty members: 144 zero bytes
        dp, ds = on_device(pts), on_device(sc)
        d_out = torch.full((k * 144,), 0xaa, dtype=torch.uint8, device="cuda")
        dev = m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, k, nbits, d_out=d_out.data_ptr())
        assert affine(dev) == want, nbits                                             # the device entry agrees with the host entry
        assert bytes(d_out.cpu().numpy()) == b"".join(dev)                            # ret and d_out agree
        only = m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, k, nbits)
        assert affine(only) == want                                                   # (as points: the order of a bucket's additions, and with it the Jacobian image, varies from run to run)


@pytest.mark.parametrize("k,n", [(3, 5), (64, 4096), (5, 33)])
def test_shared_base(m, cache, base, k, n):
    rng = random.Random(k * n)
    pts, sc = points(base, n), scalars(rng, k * n)
    want = want_ragged(pts * k, sc, [n] * k, 255, pippenger=n >= 1024)
    got = m.p1s_mult_pippenger_many(cache, pts, sc, None, 255)
    assert len(got) == k and affine(got) == want
    # the same call written as a ragged one over k copies of the points
    again = m.p1s_mult_pippenger_many(cache, pts * k, sc, offsets_of([n] * k), 255)
    assert affine(again) == want
    dp, ds = on_device(pts), on_device(sc)
    assert affine(m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), None, k, 255)) == want


def outside_g1(rng, count):
    """points on the curve but outside G1 (tests/test_gpu_msm.py test_msm_edges)"""
    out = []
    while len(out) < count:
        x = rng.randrange(o.P)
        rhs = (x * x * x + 4) % o.P
        y = pow(rhs, (o.P + 1) // 4, o.P)
        if y * y % o.P == rhs and o.g1_mul((x, y), o.R) is not None:
            out.append((x, y))
    return out


def test_neighbours_do_not_leak(m, cache):
    rng = random.Random(33)
    G = [o.g1_mul(o.G1_GEN, rng.randrange(1, o.R)) for _ in range(6)]
    P, s = G[0], rng.getrandbits(255)
    out = outside_g1(rng, 4)
    members = [
        ([G[1], G[2]], [rng.getrandbits(255), rng.getrandbits(255)]),
        ([P], [s]),                                                                   # [s]P and, next to it, [s](-P): non-zero and opposite
        ([o.g1_neg(P)], [s]),
        ([G[3], G[4], G[5]], [0, 0, 0]),                                              # all-zero scalars between two ordinary members
        ([G[2], G[3]], [rng.getrandbits(255), 5]),
        ([None, None, None], [rng.getrandbits(255) for _ in range(3)]),               # all points at infinity
        ([G[4]], [rng.getrandbits(255)]),
        ([P, o.g1_neg(P)], [s, s]),                                                   # P and -P inside one member: infinity, the neighbours not
        ([G[5], G[1]], [rng.getrandbits(255), (1 << 256) - 1]),
        (out, [rng.getrandbits(255) for _ in out]),                                   # on the curve, outside G1
        ([G[0]], [1]),
    ]
    pts = b"".join(o.g1_to_blst_affine(q) for ps, _ in members for q in ps)
    sc = b"".join(k.to_bytes(32, "little") for _, ks in members for k in ks)
    want = [o.msm_g1(ps, ks, 255) for ps, ks in members]
    assert want[1] is not None and want[2] == o.g1_neg(want[1])
    assert want[3] is None and want[5] is None and want[7] is None and want[4] is not None and want[6] is not None and want[8] is not None
    got = m.p1s_mult_pippenger_many(cache, pts, sc, offsets_of([len(ps) for ps, _ in members]), 255)
    assert [g1_jac_to_affine(b) for b in got] == want


def test_the_per_msm_tail_meets_equal_and_opposite_operands(m, cache, base):
    """tests/test_gpu_msm.py test_msm_tail_meets_equal_and_opposite_operands' four constructions as members 0 .. 3 of one ragged call beside a
    200-point random member, whatever window width c the plan picks for the call"""
    import c_oracle as co
    rng = random.Random(91)
    P = o.g1_mul(o.G1_GEN, rng.randrange(1, o.R))
    le = lambda k: k.to_bytes(32, "little")
    rnd_pts, rnd_sc = points(base, 200), scalars(rng, 200)
    rnd_want = {}
    for c in range(3, 18):
        Q = o.g1_mul(P, 1 << c)
        members = (([P, Q], [1 << c, 1]), ([P, o.g1_neg(Q)], [1 << c, 1]), ([P, Q], [1 << c, 0]), ([P, Q, P], [1 << c, 1, (1 << c) + 1]))
        pts = b"".join(o.g1_to_blst_affine(q) for ps, _ in members for q in ps) + rnd_pts
        sc = b"".join(le(k) for _, ks in members for k in ks) + rnd_sc
        offs = offsets_of([len(ps) for ps, _ in members] + [200])
        for nbits in (c + 1, 64, 255):
            if nbits not in rnd_want:
                rnd_want[nbits] = co.msm_g1(rnd_pts, rnd_sc, nbits)
            got = m.p1s_mult_pippenger_many(cache, pts, sc, offs, nbits)
            assert [g1_jac_to_affine(b) for b in got[:4]] == [o.msm_g1(ps, ks, nbits) for ps, ks in members], (c, nbits)
            assert affine(got[4:]) == [rnd_want[nbits]], (c, nbits)


def many_forms(k, n, nbits=255):
    """what a shared call of k MSMs over n points launches differently from another: (team width of the reduction, partial sums per window)"""
    head, passes = call_plan(k, nbits, n=n)
    assert len(passes) == 1 and not passes[0]["single"]
    return passes[0]["team"], head["nsplit"]


def test_both_sides_of_every_plan_hand_over(m, cache, base):
    """Below 2^18 pairs the plan has the team widths 4, 2 and 1 (by the pass's segments: found here over k at n = 64) and 1 or 4 partial sums per
    window (by the window width: found over n at k = 2).  16 partial sums need 2^14-bucket windows, a shared n of 2^17 and more, which two MSMs
    do not fit below 2^18 pairs: that form is the single path's too and is covered there (tests/test_gpu_msm.py)."""
    limit = 1 << 18
    sizes = []
    n = 64
    one_pass = call_plan(2, 255, n=n)[0]["msms_max"]                                  # beyond it a call is cut: test_calls_cut_into_passes
    for k in range(2, min(limit // n, one_pass)):
        if many_forms(k, n)[0] != many_forms(k + 1, n)[0]:
            sizes += [(k, n), (k + 1, n)]
    for e in range(1, 17):
        t = (1 << e) - 1
        if many_forms(2, t)[1] != many_forms(2, t + 1)[1]:
            sizes += [(2, t), (2, t + 1)]
    met = {many_forms(k, n) for k, n in sizes}
    assert {t for t, _ in met} == {4, 2, 1} and {s for _, s in met} == {1, 4}, met
    assert len(sizes) == 6
    rng = random.Random(7)
    for k, n in sizes:
        pts, sc = points(base, n), scalars(rng, k * n)
        want = want_ragged(pts * k, sc, [n] * k, 255, pippenger=n >= 1024)
        assert affine(m.p1s_mult_pippenger_many(cache, pts, sc, None, 255)) == want, (k, n, many_forms(k, n))


def test_calls_cut_into_passes(m, cache, base):
    """k just above what one pass takes at n = 8 per MSM: two passes; equal to the per-member oracle and to the same MSMs taken one call each
    through p1s_mult_pippenger.  (A member longer than the per-pass pair bound: test_a_member_over_the_pair_bound_between_ordinary_passes.)"""
    n = 8
    head, _ = call_plan(2, 255, n=n)
    k = head["msms_max"] + 1
    _, passes = call_plan(k, 255, lengths=[n] * k)
    assert [p["j1"] - p["j0"] for p in passes] == [k - 1, 1] and constants()["VWIN_MAX"] // head["nwin"] == k - 1
    rng = random.Random(8)
    pts, sc = points(base, n * k), scalars(rng, n * k)
    want = want_ragged(pts, sc, [n] * k, 255)
    got = affine(m.p1s_mult_pippenger_many(cache, pts, sc, offsets_of([n] * k), 255))
    assert got == want
    one_each = [m.p1s_mult_pippenger(cache, pts[96 * n * j:96 * n * (j + 1)], sc[32 * n * j:32 * n * (j + 1)], 255) for j in range(k)]
    assert affine(one_each) == got
    # the shared form cut the same way
    sh_pts = points(base, n)
    assert affine(m.p1s_mult_pippenger_many(cache, sh_pts, sc, None, 255)) == want_ragged(sh_pts * k, sc, [n] * k, 255)


@pytest.mark.parametrize("n", [1, 33, 1000])
def test_one_msm_equals_the_single_call(m, cache, base, n):
    rng = random.Random(n)
    pts, sc = points(base, n), scalars(rng, n)
    dp, ds = on_device(pts), on_device(sc)
    single = m.p1s_mult_pippenger_device(cache, dp.data_ptr(), n, ds.data_ptr(), 255)
    for offs in (None, [0, n]):
        got = m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, 1, 255)
        assert affine(got) == affine([single])
    assert affine(m.p1s_mult_pippenger_many(cache, pts, sc, [0, n], 255)) == affine([single])


def device_scalars(seed, n):
    import numpy as np
    import torch
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()


def test_a_member_over_the_pair_bound_between_ordinary_passes(m, cache, base):
    """A member of 2^20 + 1 points (over MSM_MANY_PAIRS_MAX: handed to the single-MSM path, window groups on two streams and all) between
    ordinary members, device-resident: pass, single path, pass on the caller's stream.  Expected: the same members one call each through
    p1s_mult_pippenger_device (the CPU oracle over 2^20 points takes longer than a test may; that call has its own oracle test in
    tests/test_gpu_msm.py), the small ones against the C oracle as well."""
    import torch
    big = constants()["PAIRS_MAX"] + 1
    lengths = [100, 33, big, 0, 100]
    _, passes = call_plan(len(lengths), 255, lengths=lengths)
    assert [(p["single"], p["j0"], p["j1"]) for p in passes] == [(0, 0, 2), (1, 2, 3), (0, 3, 5)]
    n, offs = sum(lengths), offsets_of(lengths)
    dp = on_device(points(base, len(base))).repeat(n // len(base) + 1)[:96 * n].contiguous()
    ds = device_scalars(20, n)
    got = m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, len(lengths), 255)
    assert got[3] == bytes(144)
    for j, v in enumerate(lengths):
        if v:
            one = m.p1s_mult_pippenger_device(cache, dp.data_ptr() + 96 * offs[j], v, ds.data_ptr() + 32 * offs[j], 255)
            assert affine([got[j]]) == affine([one]), j
    host_pts, host_sc = bytes(dp[:96 * 133].cpu().numpy()), bytes(ds[:133].cpu().numpy().tobytes())
    assert affine(got[:2]) == want_ragged(host_pts, host_sc, [100, 33], 255)
    torch.cuda.synchronize()


def test_sixteen_partial_sums_per_window(m, cache, base):
    """two MSMs over 2^18 shared points: 2^14-bucket windows, the form in which k_pip_winpart writes 16 parts per virtual window and
    k_pip_rowtail_many adds them; expected as above: one p1s_mult_pippenger_device call each"""
    n, k = 1 << 18, 2
    head, passes = call_plan(k, 255, n=n)
    assert head["nsplit"] == 16 and len(passes) == 1 and not passes[0]["single"]
    dp = on_device(points(base, len(base))).repeat(n // len(base) + 1)[:96 * n].contiguous()
    ds = device_scalars(21, k * n)
    got = m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), None, k, 255)
    for j in range(k):
        one = m.p1s_mult_pippenger_device(cache, dp.data_ptr(), n, ds.data_ptr() + 32 * n * j, 255)
        assert affine([got[j]]) == affine([one]) and affine([one]) != [bytes(96)], j
