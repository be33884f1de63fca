"""Batch verification with blinding scalars of the test's choice (mi355_bls_debug_batch_verify_scalars): the two pieces of device arithmetic that
only ever saw what a SHA-256 chain produces - k_pkmul / k_pkmul_spread (one generated assembly statement whose digit extraction and loop control
no CPU interpreter runs) and the signature side's digit sort and buckets (k_msm_hist, k_msm_scan, k_msm_scatter, k_sig_bucket, k_sig_fold) - on
the scalar families of tests/blind_scalars.py: every signed digit at every position, both values of the carry digit, every depth of a
not-started accumulator, zero digits behind a started one, waves whose 64 lanes all agree (the only time a branch on an empty execution mask
is taken), windows with every bucket empty and buckets that hold the whole batch.  Everything is bit-exact (after canonicalisation) against
the C restatement with the same scalars (oracle_batch_verify_scalars); which kernels and digit widths a case runs is ASKED of the plan
(csrc/plan.hpp through tests/util.py slice_plan) and asserted, not assumed.  Every input is a valid point and a non-zero scalar.

Where all the scalars of a batch are equal, swapping two signatures leaves sum [r]S_i - and so the verdict - unchanged; the defective batch of
those cases replaces one signature by another set's (a valid point that is not the set's signature) instead."""
import ctypes
import math
import struct

import pytest

import bls12381_py as o
import blind_scalars as bs
import util
from util import fp12_from_bytes, g2_jac_to_affine, slice_plan

pytestmark = pytest.mark.gpu

N = len(bs.ALL)
MODES = [pytest.param(True, id="latency"), pytest.param(False, id="throughput")]


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def S():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def plan_of(n, S, coop):
    return slice_plan(n, S, coop, have_side=coop)            # run_pairs: a throughput-mode context asks for no fork stream


_R2, _R3 = pow(o.MONT_R, 2, o.P), pow(o.MONT_R, 3, o.P)


def same_g1(jac144, aff96):
    """the Jacobian image (X, Y, Z) is the affine point (x, y): X = x Z^2, Y = y Z^3, Z != 0 (all-zero affine image: Z = 0).  No inversion and no
    decoding: on the Montgomery images themselves (a R mod p) the two equations read X' R^2 = x' Z'^2 and Y' R^3 = y' Z'^3."""
    X, Y, Z, x, y = (int.from_bytes(b, "little") for b in (jac144[:48], jac144[48:96], jac144[96:144], aff96[:48], aff96[48:96]))
    assert max(X, Y, Z, x, y) < o.P
    if x == 0 and y == 0:
        return Z == 0
    z2 = Z * Z % o.P
    return Z != 0 and X * _R2 % o.P == x * z2 % o.P and Y * _R3 % o.P == y * z2 * Z % o.P


def swap_sigs(rec, i, j):
    bad = bytearray(rec)
    bad[320 * i + 128:320 * i + 320], bad[320 * j + 128:320 * j + 320] = rec[320 * j + 128:320 * j + 320], rec[320 * i + 128:320 * i + 320]
    return bytes(bad)


def copy_sig(rec, i, j):
    """set i gets set j's signature (a valid point, not its own)"""
    assert rec[320 * i + 128:320 * i + 320] != rec[320 * j + 128:320 * j + 320]
    return rec[:320 * i + 128] + rec[320 * j + 128:320 * j + 320] + rec[320 * i + 320:]


def run_and_check(m, cache, rec, named, want_ok, st, label, every_pk=True):
    """one hook call against the restatement's stages `st` of the same sets and scalars: verdict, fetch(0) the scalars, every fetch(2) entry,
    fetch(3), fetch(4)"""
    n = len(named)
    scalars = [v for _, v in named]
    assert m.debugBatchVerifyScalars(cache, rec, scalars) is want_ok, label
    assert list(struct.unpack("<%dQ" % n, cache.fetch(0, 8 * n))) == scalars, label
    if every_pk:
        P = cache.fetch(2, 144 * n)
        for i, (name, r) in enumerate(named):
            assert same_g1(P[144 * i:144 * i + 144], st["rPK"][96 * i:96 * i + 96]), "%s: [r]PK of set %d (lane %d), r = %s" % (label, i, i % 64, name)
    assert o.g2_to_blst_affine(g2_jac_to_affine(cache.fetch(3, 288))) == st["aggsig"], label
    assert cache.fetch(4, 576) == st["gt"], label
    if want_ok:
        assert fp12_from_bytes(st["gt"]) == o.F12_ONE, label


def new_cache(m, n, coop):
    cache = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4)
    cache.set_cooperative(coop)
    return cache


# ---- mixed waves: every family scalar, scalar i on set i; then the list rotated by 17
@pytest.fixture(scope="module")
def mixed():
    import c_oracle as co
    rec = co.make_batch(N, seed=20261019)
    out = {}
    for rot in (0, 17):
        named = bs.rotated(rot)
        scalars = [v for _, v in named]
        i, j = 5, N - 3                                       # a full wave's lane and one of the partial last wave
        assert scalars[i] != scalars[j]
        bad = swap_sigs(rec, i, j)
        ok, st = co.batch_verify_scalars(rec, scalars)
        nok, nst = co.batch_verify_scalars(bad, scalars)
        assert ok is True and nok is False
        out[rot] = (named, st, bad, nst)
    return rec, out


@pytest.mark.parametrize("coop", MODES)
def test_mixed_waves(m, S, mixed, coop):
    rec, cases = mixed
    p = plan_of(N, S, coop)
    assert p["pkmul_spread"] == int(coop) and p["cw"] == 4 and p["nb"] == (N + 63) // 64 and N % 64      # k_pkmul_spread | k_pkmul; the last wave partial
    cache = new_cache(m, N, coop)
    try:
        for rot, (named, st, bad, nst) in cases.items():
            run_and_check(m, cache, rec, named, True, st, "rotation %d" % rot)
            run_and_check(m, cache, bad, named, False, nst, "rotation %d, two signatures swapped" % rot, every_pk=False)
    finally:
        cache.close()


# ---- uniform waves: all 64 lanes hold one scalar
@pytest.fixture(scope="module")
def uniform():
    import c_oracle as co
    rec = co.make_batch(128, seed=64064)
    memo = {}

    def stages(n, named, bad):
        key = (n, tuple(v for _, v in named), bad)
        if key not in memo:
            memo[key] = co.batch_verify_scalars(bad or rec[:320 * n], [v for _, v in named])
        return memo[key]
    return rec, stages


@pytest.mark.parametrize("coop", MODES)
@pytest.mark.parametrize("which", range(len(bs.UNIFORM)), ids=[nm for nm, _ in bs.UNIFORM])
def test_uniform_wave(m, S, uniform, which, coop):
    rec, stages = uniform
    name, r = bs.UNIFORM[which]
    n = 64
    p = plan_of(n, S, coop)
    assert p["pkmul_spread"] == int(coop) and p["nb"] == 1 and p["cw"] == 4
    named = [("uniform wave of " + name, r)] * n
    rec64 = rec[:320 * n]
    bad = copy_sig(rec64, 9, 40)                              # equal scalars: a swap would leave sum [r]S_i unchanged
    ok, st = stages(n, named, None)
    nok, nst = stages(n, named, bad)
    assert ok is True and nok is False
    cache = new_cache(m, n, coop)
    try:
        run_and_check(m, cache, rec64, named, True, st, name)
        run_and_check(m, cache, bad, named, False, nst, name + ", one signature replaced", every_pk=False)
    finally:
        cache.close()


@pytest.mark.parametrize("coop", MODES)
def test_uniform_wave_beside_a_mixed_one(m, S, uniform, coop):
    rec, stages = uniform
    n = 128
    assert plan_of(n, S, coop)["pkmul_spread"] == int(coop) and plan_of(n, S, coop)["nb"] == 2
    named = [("uniform wave of 2^64-1", bs.MASK64)] * 64 + bs.ALL[1::4][:64]
    assert len(named) == n and len({v for _, v in named[64:]}) > 48
    i, j = 7, 64 + 20
    assert named[i][1] != named[j][1]
    bad = swap_sigs(rec, i, j)
    ok, st = stages(n, named, None)
    nok, nst = stages(n, named, bad)
    assert ok is True and nok is False
    cache = new_cache(m, n, coop)
    try:
        run_and_check(m, cache, rec, named, True, st, "uniform + mixed")
        run_and_check(m, cache, bad, named, False, nst, "uniform + mixed, two signatures swapped", every_pk=False)
    finally:
        cache.close()


# ---- crowded and empty buckets at 4-bit digits: 1 024 distinct sets, one scalar
@pytest.fixture(scope="module")
def crowd():
    import c_oracle as co
    n = 1024
    rec = co.make_batch(n, seed=1024)
    total = co.g2_sum(b"".join(rec[320 * i + 128:320 * i + 320] for i in range(n)))
    return n, rec, total


@pytest.mark.parametrize("coop", MODES)
@pytest.mark.parametrize("name,r", [("1", 1), ("2^64-1", bs.MASK64), ("16^15", 1 << 60)])
def test_crowded_and_empty_buckets(m, S, crowd, name, r, coop):
    """r = 1: bucket 1 of window 0 holds all 1 024 signatures, fifteen windows are empty; 2^64 - 1: bucket 15 of every window holds them all;
    16^15: only the top window is populated.  sum [r]S_i = [r] sum S_i: one oracle multiplication."""
    import c_oracle as co
    n, rec, total = crowd
    p = plan_of(n, S, coop)
    assert p["cw"] == 4 and p["nwin"] == 16 and p["total"] == 256
    dg = bs.unsigned_digits(r, 4)
    assert {"1": dg == [1] + [0] * 15, "2^64-1": dg == [15] * 16, "16^15": dg == [0] * 15 + [1]}[name]
    cache = new_cache(m, n, coop)
    try:
        assert m.debugBatchVerifyScalars(cache, rec, [r] * n) is True, name
        assert o.g2_to_blst_affine(g2_jac_to_affine(cache.fetch(3, 288))) == co.g2_mul(total, r), name
        assert fp12_from_bytes(cache.fetch(4, 576)) == o.F12_ONE, name
        assert m.debugBatchVerifyScalars(cache, copy_sig(rec, 100, 900), [r] * n) is False, name      # equal scalars: a replaced signature, not a swap
    finally:
        cache.close()


# ---- 8-bit digits: the smallest batch the plan gives them, five sets and their negations tiled, the scalars cycling through the families
def _neg_record(rec):
    pk, sig = o.g1_from_blst_affine(rec[:96]), o.g2_from_blst_affine(rec[128:320])
    return o.g1_to_blst_affine(o.g1_neg(pk)) + rec[96:128] + o.g2_to_blst_affine(o.g2_neg(sig))


@pytest.fixture(scope="module")
def wide(S):
    import c_oracle as co
    n = util.SIG_WIDE_MIN
    while plan_of(n - 1, S, True)["cw"] == 8:                 # the smallest n the plan gives 8-bit digits
        n -= 1
    while plan_of(n, S, True)["cw"] != 8:
        n += 1
    five = co.make_batch(5, seed=5005)
    recs = [five[320 * j:320 * j + 320] for j in range(5)]
    recs += [_neg_record(x) for x in recs]                    # (-pk, m, -sig) verifies when (pk, m, sig) does
    rec = b"".join(recs[i % 10] for i in range(n))
    scalars = [bs.SCALARS[i % N] for i in range(n)]
    # sum [r_i]S_i in integers mod the group order: one multiplication per distinct signature
    want = None
    for j in range(5):
        k = (sum(scalars[j::10]) - sum(scalars[j + 5::10])) % o.R
        sj = o.g2_from_blst_affine(co.g2_mul(recs[j][128:320], k)) if k else None
        want = o.g2_add(want, sj)
    # [r]PK of every distinct (key, scalar) pair, once: the pairs repeat with period lcm(10, N)
    period = math.lcm(10, N)
    assert period <= n
    ok, st = co.batch_verify_scalars(rec[:320 * period], scalars[:period])
    assert ok is True
    unrelated = co.make_batch(1, seed=77)[128:320]
    return n, rec, scalars, want, period, st["rPK"], unrelated


@pytest.mark.parametrize("coop", MODES)
def test_eight_bit_digits(m, S, wide, coop):
    n, rec, scalars, want, period, rpk, unrelated = wide
    p = plan_of(n, S, coop)
    assert p["cw"] == 8 and p["nwin"] == 8 and p["total"] == 2048 and plan_of(n - 1, S, coop)["cw"] == 4
    assert coop or not p["pkmul_spread"]                      # throughput mode: k_pkmul; latency mode: whichever the plan names at this size
    cache = new_cache(m, n, coop)
    try:
        assert m.debugBatchVerifyScalars(cache, rec, scalars) is True
        assert list(struct.unpack("<%dQ" % n, cache.fetch(0, 8 * n))) == scalars
        assert fp12_from_bytes(cache.fetch(4, 576)) == o.F12_ONE
        assert g2_jac_to_affine(cache.fetch(3, 288)) == want
        P = cache.fetch(2, 144 * n)
        for i in range(n):
            t = i % period
            assert same_g1(P[144 * i:144 * i + 144], rpk[96 * t:96 * t + 96]), "[r]PK of set %d (key %d, lane %d), r = %s" % (i, i % 10, i % 64, bs.NAMES[i % N])
        at = 12345
        bad = rec[:320 * at + 128] + unrelated + rec[320 * at + 320:]
        assert m.debugBatchVerifyScalars(cache, bad, scalars) is False
    finally:
        cache.close()


# ---- the hook's argument checks
def test_hook_rejects_bad_arguments(m):
    """a null pointer, n == 0, n > max_sets, a context with a batch pending, any zero scalar: MI355_BLS_ERR_ARG (-3), as the other hooks answer"""
    import torch
    import c_oracle as co
    L, cap = m.lib(), 8
    cache = m.BatchedBLSVerifierCache.init(max_sets=cap, numThreads=4)
    rec = co.make_batch(cap + 1, seed=3)

    def u64s(*v):
        return (ctypes.c_uint64 * len(v))(*v)
    ones = u64s(*[1] * (cap + 1))
    try:
        for args in ((None, rec, 3, ones), (cache._h, None, 3, ones), (cache._h, rec, 3, None), (cache._h, rec, 0, ones), (cache._h, rec, cap + 1, ones),
                     (cache._h, rec, 3, u64s(0, 1, 1)), (cache._h, rec, 3, u64s(1, 0, 1)), (cache._h, rec, 3, u64s(1, 1, 0)), (cache._h, rec, 1, u64s(0))):
            assert L.mi355_bls_debug_batch_verify_scalars(*args) == -3, args[2]
        with pytest.raises(m.BlsGpuError):
            m.debugBatchVerifyScalars(cache, rec[:320 * 3], [1, 0, 1])
        with pytest.raises(ValueError):
            m.debugBatchVerifyScalars(cache, rec[:320 * 3], [1, 1])
        d = torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        cache.submit_device(d.data_ptr(), 3, bytes(32), s.cuda_stream)
        assert L.mi355_bls_debug_batch_verify_scalars(cache._h, rec, 3, ones) == -3      # a batch is pending
        assert cache.wait() is True
        assert m.debugBatchVerifyScalars(cache, rec[:320 * cap], [1] * cap) is True      # n == max_sets is inside
    finally:
        cache.close()
