"""What a context owns goes with it.  mi355_bls_debug_live_resources counts the device buffers, events, streams and pinned buffers the
library holds; a context that has been through every path that makes resources lazily (the lanes of a sliced call, the per-set pair store
and its growable outputs, the buffers of aggregateSets, both MSM workspaces, the grown staging buffers) gives all of them back when it is
destroyed, and a second context that does the same work holds exactly as many.  Every call's result is held to the C restatement on the way."""
import ctypes
import hashlib
import random

import pytest

import bls12381_py as o
from util import g1_jac_to_affine, g2_jac_to_affine

pytestmark = pytest.mark.gpu

ERR_HIP = -1
RND = hashlib.sha256(b"ctx resources rnd").digest()


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def work():
    """The inputs of every call and what the C restatement says about them: computed once, never changed."""
    import c_oracle as co
    rng = random.Random(20261017)
    w = {}
    rec8, rec193 = co.make_batch(8, seed=9100), co.make_batch(193, seed=9200)
    w["batch8"] = (rec8,) + co.batch_verify(rec8, RND, 4, stages=True)
    w["batch193"] = (rec193,) + co.batch_verify(rec193, RND, 4, stages=True)
    # per-set: 8 sets with two defects (their values too), then 200 with five
    sets = [(rec193 + rec8)[320 * i:320 * i + 320] for i in range(200)]
    each8 = list(sets[:8])
    each8[2] = each8[2][:96] + bytes([each8[2][96] ^ 1]) + each8[2][97:]                 # wrong message
    each8[5] = each8[5][:128] + each8[6][128:]                                          # another set's signature
    w["each8"] = (b"".join(each8), [co.aggregate_verify([s[:96]], [s[96:128]], s[128:], gt=True) for s in each8])
    each200 = list(sets)
    for i in (0, 63, 64, 150, 199):
        each200[i] = each200[i][:96] + bytes([each200[i][96] ^ 1]) + each200[i][97:]
    w["each200"] = (b"".join(each200), [co.core_verify(s[:96], s[96:128], s[128:]) for s in each200])
    # key lists through an index array into one table of 80 keys: lengths 1, 9 and 70, then 40 short lists
    table, _ = co.make_pks(80, seed=9300)
    key = [table[96 * i:96 * i + 96] for i in range(80)]
    perm = rng.sample(range(80), 80)
    for name, lengths in (("agg3", [1, 9, 70]), ("agg40", [rng.randint(1, 5) for _ in range(40)])):
        idx, offsets = [], [0]
        for n in lengths:
            idx += [perm[(len(idx) + j) % 80] for j in range(n)]
            offsets.append(len(idx))
        k = len(lengths)
        msgs, sigs = b"".join(s[96:128] for s in sets[:k]), b"".join(s[128:] for s in sets[:k])
        want = b"".join(co.g1_sum(b"".join(key[i] for i in idx[offsets[s]:offsets[s + 1]])) + sets[s][96:128] + sets[s][128:] for s in range(k))
        w[name] = ((table, idx, offsets), msgs, sigs, want)
    # Pippenger: 64 and 300 points in both groups
    p1, _ = co.make_pks(300, seed=9400)
    p2 = b"".join(sets[i % 200][128:] for i in range(300))
    for n in (64, 300):
        sc = bytes(rng.getrandbits(8) for _ in range(32 * n))
        w["msm%d" % n] = (p1[:96 * n], p2[:192 * n], sc, co.msm_g1(p1[:96 * n], sc, 255), co.msm_g2(p2[:192 * n], sc, 255, 32))
    # combine on 8 sets over one message
    msg = hashlib.sha256(b"ctx resources combine").digest()
    sks = [5000 + 11 * i for i in range(8)]
    hm = co.hash_to_g2(msg, o.DST_SIG)
    pks, sgs = [co.sk_to_pk(s) for s in sks], [co.g2_mul(hm, s) for s in sks]
    w["combine"] = (pks, msg, sgs) + co.combine(RND, b"".join(pks), b"".join(sgs))[:2]
    # fastAggregateVerify with 300 keys: more than the 64 x 320 bytes of staging the context starts with
    keys, sk = co.make_pks(300, seed=9500)
    good, bad = co.sign(sk, msg), co.sign(sk + 1, msg)
    assert co.fast_aggregate_verify(keys, msg, good) is True and co.fast_aggregate_verify(keys, msg, bad) is False
    w["fav"] = (keys, msg, good, bad)
    return w


def p2s_pippenger(m, cache, points, scalars):
    n = len(points) // 192
    pb, sb = ctypes.create_string_buffer(points, len(points)), ctypes.create_string_buffer(scalars, len(scalars))
    pl, sl = (ctypes.c_void_p * 2)(ctypes.addressof(pb), None), (ctypes.c_void_p * 2)(ctypes.addressof(sb), None)
    out = ctypes.create_string_buffer(288)
    assert m._check(m.lib().mi355_bls_p2s_mult_pippenger(cache._h, out, pl, n, sl, 255)) == 0
    return out.raw


def use_everything(m, w):
    """A context of 64 sets through every path that creates resources lazily; -> the live count at the end, the context still alive."""
    live = m.lib().mi355_bls_debug_live_resources
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        built = live()
        for name in ("batch8", "batch193"):                       # 193 = 3 x 64 + 1 host records: four slices over this context and both lanes
            rec, ok, st = w[name]
            assert ok is True and m.batchVerifyParallel(c, rec, RND) is True, name
            assert c.fetch(4, 576) == st["gt"], name
        assert live() > built                                     # the lanes
        rec, want = w["each8"]                                    # the per-set pair store, the verdict bytes, the values
        assert [v for v, _ in want] == [True, True, False, True, True, False, True, True]
        assert m.verifyEachValues(c, rec) == ([v for v, _ in want], [g for _, g in want])
        rec, want = w["each200"]                                  # more verdict bytes
        assert m.verifyEach(c, rec) == want and want.count(False) == 5
        for name in ("agg3", "agg40"):
            keys, msgs, sigs, want = w[name]
            assert m.aggregateSets(c, keys, msgs, sigs) == (True, want, bytes(len(msgs) // 32)), name
        for n in (64, 300):                                       # the MSM workspace, then a larger one
            p1, p2, sc, want1, want2 = w["msm%d" % n]
            assert o.g1_to_blst_affine(g1_jac_to_affine(m.p1s_mult_pippenger(c, p1, sc, 255))) == want1, n
            assert o.g2_to_blst_affine(g2_jac_to_affine(p2s_pippenger(m, c, p2, sc))) == want2, n
        pks, msg, sgs, want_pk, want_sg = w["combine"]            # the second MSM workspace
        assert m.MultiSignatureSet.init(pks, msg, sgs).combine(c, RND) == (want_pk, msg, want_sg)
        keys, msg, good, bad = w["fav"]                           # the staging buffers grow
        assert m.fastAggregateVerify(c, keys, msg, good) is True and m.fastAggregateVerify(c, keys, msg, bad) is False
        rec, ok, st = w["batch8"]                                 # and the batch path still stands on what it was given
        assert m.batchVerifyParallel(c, rec, RND) is True and c.fetch(4, 576) == st["gt"]
        return live()
    finally:
        c.close()


def test_destroy_returns_everything_and_growth_does_not_ratchet(m, work):
    L = m.lib()
    L.mi355_bls_default_ctx_release()
    c0 = L.mi355_bls_debug_live_resources()
    first = use_everything(m, work)
    assert first > c0
    assert L.mi355_bls_debug_live_resources() == c0
    second = use_everything(m, work)
    assert L.mi355_bls_debug_live_resources() == c0
    assert second == first


def test_failed_creation_leaves_nothing(m):
    import torch
    L = m.lib()
    before = L.mi355_bls_debug_live_resources()
    h = ctypes.c_void_p(1)
    assert L.mi355_bls_ctx_create(ctypes.byref(h), torch.cuda.device_count(), 64) == ERR_HIP
    assert h.value is None
    assert L.mi355_bls_debug_live_resources() == before
