"""Every point sum of the device with partial sums that are equal, opposite or infinite when they meet - in Jacobian representations that
differ, so that the complete addition formulas of csrc/curve.hpp (jac_add_aff, jac_add_body / jac_add, xyzz_add_aff) decide their branch on
H = a non-zero multiple of p instead of on limbs that are literally zero.  Inputs: the small multiples [k]P, k = -8 .. 8, of
tests/small_multiples.py (any list sums to [sum k_i]P whatever the reduction's order) and Jacobian images with a Z of the test's choice
(util.g1_jac_image / g2_jac_image).  Everything is bit-exact against the big-int oracle, or the C restatement for the batch path; that the
drawn inputs do meet every class at every level of every kernel is held by tests/test_point_sum_census.py."""
import hashlib
import random
import struct

import pytest

import bls12381_py as o
import small_multiples as sm
from util import LAMBDAS_FP, LAMBDAS_FP2, g1_jac_image, g1_jac_to_affine, g2_jac_image, g2_jac_to_affine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=2048, numThreads=4096)
    yield c
    c.close()


def dec(fam, image):
    return (g2_jac_to_affine if fam.g2 else g1_jac_to_affine)(image)


# ---- (a) one device padd(A, B) on representations of the test's choice: mi355_bls_p1s_add / p2s_add with k = 2
@pytest.mark.parametrize("name", ["g1", "g2", "outside"])
def test_one_addition_in_every_class_for_every_pair_of_z(m, cache, name):
    fam = sm.family(name)
    classes = None if name != "outside" else ("equal", "opposite")
    for cl, pair, a, b, want in sm.pair_table(fam, classes):
        got = m.p1s_add(cache, a + b, g2=fam.g2)
        assert dec(fam, got) == want, (cl, pair)          # an infinite sum decodes as infinity: None, by Z alone


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_equal_and_opposite_operands_whose_h_is_a_nonzero_multiple_of_p(m, cache, name):
    """The searched Z pairs of small_multiples.HARD_PAIRS: H (or r) of the addition is zero mod p with limbs that are not zero - the case the
    fixed lambda set above never makes (tests/test_host_emu.py holds the pairs to that through the CPU build's probe)."""
    fam = sm.family(name)
    for cl, pair, a, b, want in sm.hard_pair_table(fam):
        assert dec(fam, m.p1s_add(cache, a + b, g2=fam.g2)) == want, (cl, pair)
        G = fam.jac(7, 2)
        assert dec(fam, m.p1s_add(cache, a + G + b, g2=fam.g2)) == (o.g2_add if fam.g2 else o.g1_add)(want, fam.T[7]), (cl, pair)


def test_three_operands_through_the_device_entry(m, cache):
    """k = 3 is lane 0 += lane 2, then lane 0 += lane 1: (A, generic, B) adds the equal or opposite pair first and the generic point to its result
    (a doubling's, or infinity); (A, B, generic) meets B with A + generic.  Device-resident operands 144 and 256 bytes apart."""
    import torch
    fam = sm.family("g1")
    cases = []
    for cl, (ia, ib), a, b, want in sm.pair_table(fam, ("equal", "opposite")):
        g = 5 + (ia + ib) % 3
        G = fam.jac(g, (ia + ib + 3) % len(fam.lambdas))
        want3 = o.g1_add(want, fam.T[g])
        cases += [((a, G, b), want3, (cl, ia, ib, "A G B")), ((a, b, G), want3, (cl, ia, ib, "A B G"))]
    for stride in (144, 256):
        raw = b"".join(x + bytes(stride - 144) for ops, _, _ in cases for x in ops)
        d = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        for i, (_, want, label) in enumerate(cases):
            got = m.p1s_add_device(cache, d.data_ptr() + 3 * stride * i, 3, stride)
            assert g1_jac_to_affine(got) == want, (stride, label)


# ---- (b) k_jac_sum_blst trees
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_jacobian_sum_trees(m, cache, name):
    fam = sm.family(name)
    for label, ks, lams in sm.jac_cases(len(fam.lambdas)):
        got = m.p1s_add(cache, fam.jac_list(ks, lams), g2=fam.g2)
        assert dec(fam, got) == fam.mul(sum(ks)), label


# ---- (c) aggregateAll / aggregateAllSignatures
@pytest.mark.parametrize("name", ["g1", "g2", "outside"])
def test_aggregate_all_of_small_multiples(m, cache, name):
    fam = sm.family(name)
    agg = m.aggregateAllSignatures if fam.g2 else m.aggregateAll
    zero_lists = 0
    for label, ks in sm.agg_cases():
        got = agg(cache, fam.affine_list(ks))
        assert dec(fam, got) == fam.mul(sum(ks)), label
        zero_lists += sum(ks) == 0
    assert zero_lists >= len(sm.AGG_SIZES)


def test_fast_aggregate_verify_of_keys_that_cancel(m, cache):
    import c_oracle as co
    fam = sm.family("g1")
    msg = hashlib.sha256(b"keys that cancel").digest()
    sig = co.sign(12345, msg)
    for n in (65, 1025):
        ks = sm.draw_zero(n, 1000 * n)
        assert m.fastAggregateVerify(cache, fam.affine_list(ks), msg, sig) is False, n
    assert m.fastAggregateVerify(cache, co.sk_to_pk(12345), msg, sig) is True


# ---- (d) aggregate_sets
def test_aggregate_sets_of_small_multiples(m, cache):
    from test_aggsets_plan import plan_aggsets_lib
    C = plan_aggsets_lib().aggsets_plan_c()
    fam = sm.family("g1")
    lists = sm.aggsets_lists(C)
    k = len(lists)
    msgs, sigs = bytes(32 * k), bytes(192 * k)
    table = b"".join(fam.aff(kk) for kk in sm.KS)
    idx, offsets = [], [0]
    for _, ks in lists:
        idx += [kk + sm.KMAX for kk in ks]
        offsets.append(len(idx))
    want_key = [fam.to_affine_bytes(fam.mul(sum(ks))) for _, ks in lists]
    want_status = bytes(2 if sum(ks) == 0 else 0 for _, ks in lists)
    assert 2 in want_status and 0 in want_status
    drawn_table = b"".join(fam.affine_list(ks) for _, ks in lists)
    for form, keys in (("idx", (table, idx, offsets)), ("ranges", (drawn_table, None, offsets)), ("lists", [fam.affine_list(ks) for _, ks in lists])):
        ok, rec, st = m.aggregateSets(cache, keys, msgs, sigs)
        assert ok is False and st == want_status, form
        for s, (label, _) in enumerate(lists):
            assert rec[320 * s:320 * s + 96] == want_key[s], (form, label)


# ---- (e) Pippenger
def _msm_input(fam, n, seed, scalars):
    rng = random.Random(seed)
    ks = [rng.randint(-sm.KMAX, sm.KMAX) for _ in range(n)]
    return ks, [rng.choice(scalars) for _ in range(n)]


def _msm_want(fam, ks, sc, nbits):
    mask = (1 << nbits) - 1
    return fam.mul(sum(k * (s & mask) for k, s in zip(ks, sc)) % o.R)             # integers mod r, then one oracle multiplication


def _le(sc, size):
    return b"".join(s.to_bytes(32, "little")[:size] for s in sc)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_pippenger_of_small_multiples(m, cache, name):
    fam = sm.family(name)
    scalars = sm.pippenger_scalars()
    inputs = [_msm_input(fam, n, 31 * n + nb, scalars) for n in (2, 7, 64, 300) for nb in (0, 1)]
    half_k, half_s = _msm_input(fam, 32, 3232, scalars)
    inputs.append((half_k + [-k for k in half_k], half_s + half_s))               # the total is infinity
    for ks, sc in inputs:
        pts = fam.affine_list(ks)
        for nbits in (64, 255):
            want = _msm_want(fam, ks, sc, nbits)
            got = m.blst_p1s_mult_pippenger(pts, _le(sc, (nbits + 7) // 8), nbits, g2=fam.g2)
            assert dec(fam, got) == want, (len(ks), nbits, "blst form")
            if fam.g2:
                got = m.p1s_mult_pippenger_multi([cache], pts, _le(sc, 32), nbits, g2=True)
            else:
                got = m.p1s_mult_pippenger(cache, pts, _le(sc, 32), nbits)
            assert dec(fam, got) == want, (len(ks), nbits, "context form")
    assert _msm_want(fam, *inputs[-1], 255) is None


def test_pippenger_g2_lds_sort_path_with_crowded_buckets(m):
    """n = 33 000 (the counting sort in LDS) with scalars below 2^16 from a set of 45: a handful of buckets hold thousands of +-kP each"""
    fam = sm.family("g2")
    scalars = [s for s in sm.pippenger_scalars() if s < 1 << 16]
    ks, sc = _msm_input(fam, 33000, 33000, scalars)
    got = m.blst_p2s_mult_pippenger(fam.affine_list(ks), _le(sc, 8), 64)
    assert g2_jac_to_affine(got) == _msm_want(fam, ks, sc, 64)


# ---- (f) the signature side of a batch: k_sig_bucket (xyzz_add_aff per lane, jac_add fold) and k_sig_fold with equal and opposite signatures
def _neg_record(rec):
    pk, sig = o.g1_from_blst_affine(rec[:96]), o.g2_from_blst_affine(rec[128:320])
    return o.g1_to_blst_affine(o.g1_neg(pk)) + rec[96:128] + o.g2_to_blst_affine(o.g2_neg(sig))


@pytest.fixture(scope="module")
def sig_batches():
    """n -> (records, kinds, C restatement's stages): copies of one valid set, copies of its negation ((-pk, m, -sig) verifies when (pk, m, sig)
    does) and five unrelated sets, shuffled; made once"""
    import c_oracle as co
    rnd = o.sha256(b"signature side")
    one = co.make_batch(1, seed=2026)
    neg = _neg_record(one)
    other = co.make_batch(5, seed=909)
    out = {}
    for n, copies in ((1024, 700), (1100, 600)):
        kinds = [1] * copies + [-1] * (n - 5 - copies) + [2, 3, 4, 5, 6]
        random.Random(n).shuffle(kinds)
        rec = b"".join(one if kd == 1 else neg if kd == -1 else other[320 * (kd - 2):320 * (kd - 1)] for kd in kinds)
        ok, st = co.batch_verify(rec, rnd, 4096, stages=True)
        assert ok
        out[n] = (rec, kinds, st)
    return rnd, one, other, out


@pytest.mark.parametrize("coop", [True, False])
@pytest.mark.parametrize("n", [1024, 1100])
def test_signature_side_with_equal_and_opposite_signatures(m, sig_batches, n, coop):
    rnd, one, other, batches = sig_batches
    rec, kinds, st = batches[n]
    cache = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4096)
    try:
        cache.set_cooperative(coop)                                               # latency mode / throughput mode
        assert m.batchVerifyParallel(cache, rec, rnd) is True
        r = struct.unpack("<%dQ" % n, cache.fetch(0, 8 * n))
        assert list(r) == st["r"]
        S = o.g2_from_blst_affine(one[128:320])
        want = o.g2_mul(S, sum(ri * kd for ri, kd in zip(r, kinds) if abs(kd) == 1))
        for ri, kd in zip(r, kinds):
            if kd >= 2:
                want = o.g2_add(want, o.g2_mul(o.g2_from_blst_affine(other[320 * (kd - 2) + 128:320 * (kd - 1)]), ri))
        assert g2_jac_to_affine(cache.fetch(3, 288)) == want                      # sum r_i S_i, folded from the buckets
        assert o.g2_to_blst_affine(want) == st["aggsig"]
        assert cache.fetch(4, 576) == st["gt"]
        at = kinds.index(1)
        bad = rec[:320 * at + 128] + other[128:320] + rec[320 * at + 320:]         # one copy's signature: an unrelated valid point
        assert m.batchVerifyParallel(cache, bad, rnd) is False
        if coop:
            assert m.verifyEach(cache, rec) == [True] * n
    finally:
        cache.close()


# ---- (g) Jacobian arguments with Z != 1 further along
def test_aggregates_with_their_own_z_give_the_same_verdict_and_gt(m, cache):
    import c_oracle as co
    msg = hashlib.sha256(b"aggregate with a z").digest()
    sks = [1000003 + 17 * i for i in range(3)]
    pks = [co.sk_to_pk(s) for s in sks]
    agg = o.g1_from_blst_affine(co.sk_to_pk(sum(sks)))
    good, bad = co.sign(sum(sks), msg), co.sign(sum(sks) + 1, msg)
    ref = {}
    for lam in LAMBDAS_FP:                                                         # LAMBDAS_FP[0] = 1: the reference of the others
        for sig, verdict in ((good, True), (bad, False)):
            assert m.verifyAggregate(cache, g1_jac_image(agg, lam), msg, sig) is verdict, lam
            assert ref.setdefault(sig, cache.fetch(4, 576)) == cache.fetch(4, 576), lam
    msgs = [hashlib.sha256(b"aggv %d" % i).digest() for i in range(3)]
    sigs = [o.g2_from_blst_affine(co.sign(s, x)) for s, x in zip(sks, msgs)]
    total = o.g2_add(o.g2_add(sigs[0], sigs[1]), sigs[2])
    wrong = o.g2_add(total, sigs[0])
    ref = {}
    for lam in LAMBDAS_FP2:
        for point, verdict in ((total, True), (wrong, False)):
            image = g2_jac_image(point, lam)
            assert m.aggregateVerify(cache, pks, msgs, image) is verdict, lam
            gt = cache.fetch(4, 576)
            assert ref.setdefault(verdict, gt) == gt, lam
            ctx = m.ContextCoreAggregateVerify(cache)
            ctx.init()
            assert all(ctx.update(pk, x) for pk, x in zip(pks, msgs))
            assert ctx.finish(image) is verdict, lam
            assert cache.fetch(4, 576) == gt, lam
    assert m.aggregateVerify(cache, pks, msgs, o.g2_to_blst_affine(total)) is True and cache.fetch(4, 576) == ref[True]
