"""GPU parity of k G2 MSMs in one device pass (mi355_bls_p2s_mult_pippenger_many / _many_device) against the oracles' MSM of every member alone:
both addressing forms, both entries and every output choice, neighbours that must not leak into each other, the per-MSM walk's exceptional
additions, a call cut into passes, k = 1, and the context's resources.  Results are compared on the canonical affine image."""
import random

import pytest

import bls12381_py as o
import g2many_helpers as h
from util import g2_jac_to_affine

pytestmark = pytest.mark.gpu
RAGGED = [0, 1, 2, 31, 32, 33, 0, 100, 1]


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
    """a hundred distinct points of G2, repeated by every test: signatures of one message under a hundred keys (the C oracle makes them fast)"""
    import c_oracle as co
    rng = random.Random(4321)
    return [co.sign(rng.getrandbits(96) | 1, b"g2 many") for _ in range(100)]


def points(base, n, first=0):
    return b"".join(base[(first + i) % len(base)] for i in range(n))


def scalars(rng, n, nbits=256):
    return b"".join(rng.getrandbits(nbits).to_bytes(32, "little") for _ in range(n))


def affine(outs):
    assert all(len(b) == 288 for b in outs)
    return [h.g2_affine_bytes(g2_jac_to_affine(b)) for b in outs]


def want_ragged(pts, sc, lengths, nbits):
    import c_oracle as co
    offs = h.offsets_of(lengths)
    return [co.msm_g2(pts[192 * a:192 * b], sc[32 * a:32 * b], nbits) if b > a else bytes(192) for a, b in zip(offs, offs[1:])]


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data) if data else bytearray(16), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("nbits", [5, 64, 255, 256])
def test_ragged_smallest_shapes_and_every_output_choice(m, cache, base, nbits):
    import torch
    rng = random.Random(nbits)
    n, k = sum(RAGGED), len(RAGGED)
    pts, offs, sc = points(base, n), h.offsets_of(RAGGED), scalars(rng, n)
    want = want_ragged(pts, sc, RAGGED, nbits)
    got = m.p2s_mult_pippenger_many(cache, pts, sc, offs, nbits)
    assert affine(got) == want
    for j, v in enumerate(RAGGED):
        if v == 0:
            assert got[j] == bytes(288), j                                            # empty members: 288 zero bytes
    dp, ds = on_device(pts), on_device(sc)
    d_out = torch.full((k * 288,), 0xaa, dtype=torch.uint8, device="cuda")
    both = m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, k, nbits, d_out=d_out.data_ptr())
    assert affine(both) == want and bytes(d_out.cpu().numpy()) == b"".join(both)       # ret and d_out
    assert affine(m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, k, nbits)) == want      # ret only
    d_out.fill_(0xaa)
    assert m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, k, nbits, d_out=d_out.data_ptr(), ret=False) is None
    raw = bytes(d_out.cpu().numpy())                                                  # d_out only
    assert affine([raw[288 * j:288 * j + 288] for j in range(k)]) == want


@pytest.mark.parametrize("k,n", [(3, 5), (5, 33), (64, 256)])
def test_shared_base(m, cache, base, k, n):
    rng = random.Random(k * n)
    pts, sc = points(base, n), scalars(rng, k * n)
    want = want_ragged(pts * k, sc, [n] * k, 255)
    got = m.p2s_mult_pippenger_many(cache, pts, sc, None, 255)
    assert len(got) == k and affine(got) == want
    assert affine(m.p2s_mult_pippenger_many(cache, pts * k, sc, h.offsets_of([n] * k), 255)) == want      # the same call written as a ragged one
    dp, ds = on_device(pts), on_device(sc)
    assert affine(m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), None, k, 255)) == want


def test_neighbours_do_not_leak(m, cache):
    rng = random.Random(33)
    G = [o.g2_mul(o.G2_GEN, rng.randrange(1, o.R)) for _ in range(5)]
    P, s = G[0], rng.getrandbits(255)
    members = [
        ([G[1], G[2]], [rng.getrandbits(255), rng.getrandbits(255)]),
        ([P], [s]),                                                                   # [s]P and, next to it, [s](-P): non-zero and opposite
        ([o.g2_neg(P)], [s]),
        ([G[3], G[4]], [0, 0]),                                                       # all-zero scalars between two ordinary members
        ([G[2], None, G[3]], [rng.getrandbits(255), rng.getrandbits(255), 5]),        # an infinity image among the points
        ([None, None], [rng.getrandbits(255), 1]),                                    # all points at infinity
        ([P, o.g2_neg(P)], [s, s]),                                                   # P and -P inside one member: infinity, the neighbours not
        ([G[4], G[1]], [rng.getrandbits(255), (1 << 256) - 1]),
        ([G[0]], [1]),
    ]
    pts = b"".join(h.g2_affine_bytes(q) for ps, _ in members for q in ps)
    sc = b"".join(k.to_bytes(32, "little") for _, ks in members for k in ks)
    want = [h.msm_g2(ps, ks, 255) for ps, ks in members]
    assert want[1] is not None and want[2] == o.g2_neg(want[1]) and want[3] is None and want[5] is None and want[6] is None and want[4] is not None
    got = m.p2s_mult_pippenger_many(cache, pts, sc, h.offsets_of([len(ps) for ps, _ in members]), 255)
    assert [g2_jac_to_affine(b) for b in got] == want
    assert got[3] == bytes(288) and got[5] == bytes(288) and got[6] == bytes(288)     # an infinite result made by a pass: 288 zero bytes


def test_the_per_msm_walk_meets_equal_opposite_and_infinite_operands(m, cache, base):
    """tests/test_gpu_msm_many.py's four constructions with a second point 2^c P, as members 0 .. 3 of one ragged call beside a 50-point random
    member, for every c around the window widths the plan gives this call (4 and 5 bits at 255 bits, by the mean member length)"""
    import c_oracle as co
    rng = random.Random(91)
    P = o.g2_mul(o.G2_GEN, rng.randrange(1, o.R))
    le = lambda k: k.to_bytes(32, "little")
    rnd_pts, rnd_sc = points(base, 50), scalars(rng, 50)
    head, _ = h.call_plan(5, 255, lengths=[2, 2, 2, 3, 50])
    assert {head["wbase"], head["wbase"] + (1 if head["wrem"] else 0)} <= set(range(3, 9))
    for c in range(3, 9):
        Q = o.g2_mul(P, 1 << c)
        members = (([P, Q], [1 << c, 1]), ([P, o.g2_neg(Q)], [1 << c, 1]), ([P, Q], [1 << c, 0]), ([P, Q, P], [1 << c, 1, (1 << c) + 1]))
        pts = b"".join(h.g2_affine_bytes(q) for ps, _ in members for q in ps) + rnd_pts
        sc = b"".join(le(k) for _, ks in members for k in ks) + rnd_sc
        offs = h.offsets_of([len(ps) for ps, _ in members] + [50])
        for nbits in (c + 1, 64, 255):
            got = m.p2s_mult_pippenger_many(cache, pts, sc, offs, nbits)
            assert [g2_jac_to_affine(b) for b in got[:4]] == [h.msm_g2(ps, ks, nbits) for ps, ks in members], (c, nbits)
            assert affine(got[4:]) == [co.msm_g2(rnd_pts, rnd_sc, nbits)], (c, nbits)


@pytest.mark.parametrize("n", [1, 33])
def test_one_msm_equals_the_single_call_bit_for_bit(m, cache, base, n):
    rng = random.Random(n)
    pts, sc = points(base, n), scalars(rng, n)
    dp, ds = on_device(pts), on_device(sc)
    single = m.p2s_mult_pippenger_device(cache, dp.data_ptr(), n, ds.data_ptr(), 255)
    for offs in (None, [0, n]):
        assert m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, 1, 255) == [single]
    assert m.p2s_mult_pippenger_many(cache, pts, sc, [0, n], 255) == [single]


def test_a_call_cut_into_two_passes(m, cache, base):
    """k single-point MSMs at nbits = 64, k one above what a pass takes (from the plan library): two non-single passes, asserted here so that a
    plan change cannot quietly make this a one-pass test.  Forty distinct (point, scalar) members, repeated."""
    import c_oracle as co
    head, _ = h.call_plan(2, 64, lengths=[1, 1])
    k = head["msms_max"] + 1
    _, passes = h.call_plan(k, 64, lengths=[1] * k)
    assert len(passes) >= 2 and not any(p["single"] for p in passes) and [p["j1"] - p["j0"] for p in passes] == [k - 1, 1]
    rng = random.Random(64)
    some_sc = [rng.getrandbits(64).to_bytes(32, "little") for _ in range(5)]
    pts = b"".join(base[j % 8] for j in range(k))
    sc = b"".join(some_sc[j % 5] for j in range(k))
    one = {(a, b): co.msm_g2(base[a], some_sc[b], 64) for a in range(8) for b in range(5)}
    dp, ds = on_device(pts), on_device(sc)
    got = affine(m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), k, ds.data_ptr(), list(range(k + 1)), k, 64))
    assert got == [one[(j % 8, j % 5)] for j in range(k)]


def device_scalars(seed, n):
    import numpy as np
    import torch
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()


@pytest.mark.parametrize("n,nsplit", [(1 << 15, 4), (1 << 18, 16)])
def test_several_partial_sums_per_window(m, cache, base, n, nsplit):
    """Members long enough for k_pip_winpart to write 4 and 16 parts per window: the tail then ADDS parts (wave 0 alone, lanes and shuffles) where
    every smaller shape only copies one.  The part count is asserted from the plan library.  Expected: the C oracle's Pippenger at 2^15
    points; at 2^18, where it takes longer than a test may, one p2s_mult_pippenger_device call per member (it has its own oracle tests)."""
    import c_oracle as co
    k = 2
    head, passes = h.call_plan(k, 255, n=n)
    assert head["nsplit"] == nsplit > 1 and len(passes) == 1 and not passes[0]["single"]
    dp = on_device(points(base, len(base))).repeat(n // len(base) + 1)[:192 * n].contiguous()
    ds = device_scalars(n, k * n)
    got = m.p2s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), None, k, 255)
    assert all(g != bytes(288) for g in got)
    if n <= 1 << 15:
        pts, sc = bytes(dp.cpu().numpy()), bytes(ds.cpu().numpy().tobytes())
        assert affine(got) == [co.msm_g2_pippenger(pts, sc[32 * n * j:32 * n * (j + 1)], 255) for j in range(k)]
    else:
        one = [m.p2s_mult_pippenger_device(cache, dp.data_ptr(), n, ds.data_ptr() + 32 * n * j, 255) for j in range(k)]
        assert affine(got) == affine(one)
    # the same members as a ragged call over k copies of the points: the other addressing form through the same tail
    if n <= 1 << 15:
        d2 = dp.repeat(k).contiguous()
        again = m.p2s_mult_pippenger_many_device(cache, d2.data_ptr(), k * n, ds.data_ptr(), [0, n, 2 * n], k, 255)
        assert affine(again) == affine(got)


def test_live_resources_return_to_their_start(m, base):
    live = m.lib().mi355_bls_debug_live_resources
    rng = random.Random(8)
    start = live()
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    with_ctx = live()
    got = m.p2s_mult_pippenger_many(c, points(base, 6), scalars(rng, 6), [0, 2, 6], 255)
    assert len(got) == 2 and live() > with_ctx
    m.p2s_to_affine(c, b"".join(got))
    c.close()
    assert live() == start
