"""Pairing-product checks over caller-supplied pairs on the device (mi355_bls_pairing_check_each, mi355_bls_pairing_products,
mi355_bls_batch_pairing_check[_locate], the scalar hook).  Values are held byte for byte to oracle/bls12381_py.py
(fp12_to_bytes(final_exp(miller_loop(pairs)))), 60 ms a pair there, so the value tests stay small; verdicts come from bilinearity
(tests/pairprod_cases.py) and need no oracle pairing.  The CPU half is tests/test_pairprod_plan.py, tests/test_pairprod_emu.py and
tests/test_cabi_pairprod.py."""
import ctypes
import hashlib
import random

import pytest

import bls12381_py as o
import pairprod_cases as pc
from util import fp12_to_bytes, g2_jac_to_affine

pytestmark = pytest.mark.gpu

ERR_ARG = -3
ONE = fp12_to_bytes(o.F12_ONE)


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=4096, numThreads=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    return pc.Pool(20261020)


def value(pairs):
    return fp12_to_bytes(o.final_exp(o.miller_loop(pairs)))


@pytest.fixture(scope="module")
def random_groups(pool):
    """groups of 1, 2, 3, 8, 9 pairs with random (not cancelling) scalars, and the oracle's value of each, computed once"""
    rng = random.Random(5)
    gs = [[(pc.g1(rng.choice(pool.a)), pc.g2(rng.choice(pool.b))) for _ in range(n)] for n in (1, 2, 3, 8, 9)]
    return gs, [value(g) for g in gs]


def test_values_equal_the_oracle_in_both_modes(m, cache, random_groups):
    gs, want = random_groups
    try:
        for coop in (True, False):                                     # the Fp12 engine tail, then the one-lane tail
            cache.set_cooperative(coop)
            v, gt = m.pairingProducts(cache, [pc.images(g) for g in gs])
            assert gt == want, coop
            assert v == [False] * 5, coop
            assert m.pairingCheckEach(cache, [pc.images(g) for g in gs]) == v
    finally:
        cache.set_cooperative(True)


LENGTHS = [1, 2, 7, 8, 9, 64, 65]


@pytest.fixture(scope="module")
def forty(pool):
    rng = random.Random(40)
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(40)]
    rng.shuffle(lens)
    valid = [rng.random() < 0.5 for _ in lens]
    return [pc.images(pool.group(rng, n, ok)) for n, ok in zip(lens, valid)], valid


def test_verdicts_of_forty_groups(m, cache, forty):
    gs, valid = forty
    assert 10 < valid.count(True) < 30
    assert m.pairingCheckEach(cache, gs) == valid
    L, sz = m.lib(), ctypes.c_size_t
    good = [g for g, ok in zip(gs, valid) if ok]
    offs = [0]
    for g in good:
        offs.append(offs[-1] + len(g))
    out = ctypes.create_string_buffer(len(good))
    p1, q2 = b"".join(p for g in good for p, _ in g), b"".join(q for g in good for _, q in g)
    assert L.mi355_bls_pairing_check_each(cache._h, p1, q2, (sz * len(offs))(*offs), len(good), 0, out, None) == 1      # returns 1 iff all are 1
    assert out.raw == b"\1" * len(good)


def test_a_group_does_not_depend_on_its_neighbours(m, cache, pool, forty):
    gs, valid = forty
    v0, gt0 = m.pairingProducts(cache, gs)
    assert v0 == valid and all((g == ONE) == ok for g, ok in zip(gt0, valid))
    rng = random.Random(41)
    order = list(range(len(gs)))
    rng.shuffle(order)
    mixed = []
    for i in order:
        mixed.append(("x", pc.images(pool.group(rng, rng.choice((1, 3, 9)), rng.random() < 0.5))))
        mixed.append((i, gs[i]))
    v, gt = m.pairingProducts(cache, [g for _, g in mixed])
    for at, (i, _) in enumerate(mixed):
        if i != "x":
            assert (v[at], gt[at]) == (v0[i], gt0[i]), i


def test_infinity_and_empty_groups(m, cache, pool):
    rng = random.Random(7)
    p, q = pc.p1b(pc.g1(5)), pc.q2b(pc.g2(9))
    ok3 = pc.images(pool.group(rng, 3))
    bad3 = pc.images(pool.group(rng, 3, False))
    gs = [[], [(pc.INF1, q)], [(p, pc.INF2)], [(pc.INF1, pc.INF2)], [(pc.INF1, q), (p, pc.INF2), (pc.INF1, pc.INF2)], [],
          ok3[:1] + [(pc.INF1, q)] + ok3[1:], bad3 + [(p, pc.INF2)], [], []]
    v, gt = m.pairingProducts(cache, gs)
    assert v == [True, True, True, True, True, True, True, False, True, True]
    assert all(g == ONE for g, ok in zip(gt, v) if ok) and gt[7] != ONE
    assert gt[7] == m.pairingProducts(cache, [bad3])[1][0]              # the infinite pair contributes 1
    assert m.pairingCheckEach(cache, [[], []]) == [True, True]         # nothing but empty groups
    L, sz = m.lib(), ctypes.c_size_t
    out = ctypes.create_string_buffer(b"\x5a" * 4, 4)
    assert L.mi355_bls_pairing_check_each(cache._h, None, None, (sz * 1)(0), 0, 0, out, None) == 0 and out.raw == b"\x5a" * 4      # k == 0


def test_slices_and_the_carry(m, small, cache, pool):
    rng = random.Random(150)
    for wrong in (False, True):
        lens = [3, 1, 150, 2, 64, 1, 5, 0, 9]
        gs = [pc.images(pool.group(rng, n, not (wrong and n == 150))) if n else [] for n in lens]
        try:
            for coop in (True, False):
                small.set_cooperative(coop), cache.set_cooperative(coop)
                v, gt = m.pairingProducts(small, gs)                       # max_sets = 64: the group of 150 runs in three parts
                assert v == [not (wrong and n == 150) for n in lens], (wrong, coop)
                assert (v, gt) == m.pairingProducts(cache, gs), (wrong, coop)
        finally:
            small.set_cooperative(True), cache.set_cooperative(True)


def test_validation(m, cache, pool):
    adv = pc.adversarial()
    rng = random.Random(11)
    p, q = pc.p1b(pc.g1(5)), pc.q2b(pc.g2(9))
    gs, want_st, hostile = [], [], []
    for name, (img, st) in sorted(adv.items()):
        good = pc.images(pool.group(rng, 3))
        gs.append(good)                                                 # a valid group in front of every hostile one
        want_st += [0, 0, 0]
        pair = (img, q) if len(img) == 96 else (p, img)
        gs.append(good[:2] + [pair] + good[2:])                         # the same valid group with the hostile pair inside
        want_st += [0, 0, st, 0]
        hostile.append(len(gs) - 1)
    gs.append([(pc.INF1, pc.INF2), (pc.INF1, q)])                        # infinity passes validation
    want_st += [0, 0]
    v, st = m.pairingCheckEach(cache, gs, flags=m.PAIR_VALIDATE, with_status=True)
    assert st == want_st and set(want_st) == {0, 1, 2, 3, 4}
    assert v == [i not in hostile for i in range(len(gs))]
    # a failing pair is given infinite operands: what is left of its group is the valid group, whose value is one
    v2, gt, st2 = m.pairingProducts(cache, gs, flags=m.PAIR_VALIDATE, with_status=True)
    assert (v2, st2) == (v, st) and all(g == ONE for g in gt)
    ok, st3 = m.batchPairingCheck(cache, gs, hashlib.sha256(b"validate").digest(), flags=m.PAIR_VALIDATE, with_status=True)
    assert ok is False and st3 == want_st
    # the same valid input with and without validation
    valid = [g for i, g in enumerate(gs) if i not in hostile]
    a = m.pairingCheckEach(cache, valid, flags=m.PAIR_VALIDATE, with_status=True)
    assert a == ([True] * len(valid), [0] * sum(len(g) for g in valid)) and m.pairingCheckEach(cache, valid) == a[0]
    assert m.batchPairingCheck(cache, valid, hashlib.sha256(b"validate").digest(), flags=m.PAIR_VALIDATE) is True
    L, sz = m.lib(), ctypes.c_size_t
    out = ctypes.create_string_buffer(1)
    assert L.mi355_bls_pairing_check_each(cache._h, p, q, (sz * 2)(0, 1), 1, m.PAIR_VALIDATE, out, None) == ERR_ARG      # status is required
    assert L.mi355_bls_pairing_check_each(cache._h, p, q, (sz * 2)(0, 1), 1, 2, out, None) == ERR_ARG                    # unknown flag bit


def test_blinded_form(m, cache, small, pool, random_groups):
    rng = random.Random(64)
    rnd = hashlib.sha256(b"batch pairing check").digest()
    lens = [1, 2, 0, 9, 65, 3, 0, 8]
    gs = [pc.images(pool.group(rng, n)) if n else [] for n in lens]
    try:
        for c in (cache, small):                                            # one slice; parts of 64 pairs carried
            for coop in (True, False):
                c.set_cooperative(coop)
                assert m.batchPairingCheck(c, gs, rnd) is True
                assert m.batchPairingCheckLocate(c, gs, rnd) == (True, [True] * len(gs))
                bad = list(gs)
                bad[4] = pc.images(pool.group(rng, 65, False))
                assert m.batchPairingCheck(c, bad, rnd) is False
                assert m.batchPairingCheckLocate(c, bad, rnd) == (False, [i != 4 for i in range(len(gs))])
    finally:
        cache.set_cooperative(True), small.set_cooperative(True)
    assert m.batchPairingCheck(cache, [[], []], rnd) is True              # nothing but empty groups: the empty product
    # the value under chosen scalars equals the oracle's over ([r_g]P, Q)
    pts, _ = random_groups
    r = [3, 5, 7, 11, 13]
    want = value([(o.g1_mul(p, rg), q) for g, rg in zip(pts, r) for p, q in g])
    ok, gt = m.batchPairingCheckScalars(cache, [pc.images(g) for g in pts], r)
    assert (ok, gt) == (False, want)
    assert m.batchPairingCheckScalars(small, [pc.images(g) for g in pts], r) == (False, want)


def test_blinding_defeats_cancellation(m, cache):
    a = 123457
    A, B = [(pc.p1b(pc.g1(a)), pc.q2b(pc.g2(1)))], [(pc.p1b(pc.g1(-a)), pc.q2b(pc.g2(1)))]
    assert m.pairingCheckEach(cache, [A, B]) == [False, False]
    assert m.batchPairingCheckScalars(cache, [A, B], [1, 1]) == (True, ONE)                 # unblinded, the two failures cancel
    ok, gt = m.batchPairingCheckScalars(cache, [A, B], [3, 5])
    assert ok is False and gt != ONE
    rnd = hashlib.sha256(b"cancellation").digest()
    assert m.batchPairingCheck(cache, [A, B], rnd) is False
    # the public call decides what the hook's value under the chain's own scalars says
    r = o.blinding_scalars(rnd, 2)
    ok, gt = m.batchPairingCheckScalars(cache, [A, B], r)
    assert ok is False and gt == value([(o.g1_mul(pc.g1(a), r[0]), pc.g2(1)), (o.g1_mul(pc.g1(-a), r[1]), pc.g2(1))])


def test_consistent_with_verify_each(m, cache):
    import c_oracle as co
    n = 12
    rec = bytearray(co.make_batch(n, seed=4242))
    rec[320 * 3 + 96] ^= 1                                              # another message for set 3
    rec[320 * 7 + 128:320 * 7 + 320] = rec[320 * 8 + 128:320 * 8 + 320]        # another set's signature for set 7
    rec = bytes(rec)
    want_v, want_gt = m.verifyEachValues(cache, rec)
    assert want_v == [i not in (3, 7) for i in range(n)]
    neg_g1 = pc.p1b(o.g1_neg(o.G1_GEN))
    gs = []
    for i in range(n):
        pk, msg, sig = rec[320 * i:320 * i + 96], rec[320 * i + 96:320 * i + 128], rec[320 * i + 128:320 * i + 320]
        out = ctypes.create_string_buffer(288)
        assert m._check(m.lib().mi355_bls_debug_hash_to_g2(cache._h, msg, 32, o.DST_SIG, len(o.DST_SIG), out)) == 0
        gs.append([(pk, o.g2_to_blst_affine(g2_jac_to_affine(out.raw))), (neg_g1, sig)])
    assert m.pairingProducts(cache, gs) == (want_v, want_gt)


def test_device_forms_streams_and_resources(m, pool):
    import torch
    rng = random.Random(77)
    lens = [2, 0, 9, 1, 70]
    gs = [pc.images(pool.group(rng, n, n != 9)) if n else [] for n in lens]
    offs = [0]
    for g in gs:
        offs.append(offs[-1] + len(g))
    rnd = hashlib.sha256(b"device forms").digest()
    live = m.lib().mi355_bls_debug_live_resources
    before = live()
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        host = m.pairingProducts(c, gs)
        d_p = torch.frombuffer(bytearray(b"".join(p for g in gs for p, _ in g)), dtype=torch.uint8).cuda()
        d_q = torch.frombuffer(bytearray(b"".join(q for g in gs for _, q in g)), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        for s in (0, stream.cuda_stream):
            assert m.pairingProducts_device(c, d_p.data_ptr(), d_q.data_ptr(), offs, stream=s) == host
            assert m.pairingCheckEach_device(c, d_p.data_ptr(), d_q.data_ptr(), offs, flags=m.PAIR_VALIDATE, stream=s) == (host[0], [0] * offs[-1])
            assert m.batchPairingCheck_device(c, d_p.data_ptr(), d_q.data_ptr(), offs, rnd, stream=s) is False
            assert m.batchPairingCheckLocate_device(c, d_p.data_ptr(), d_q.data_ptr(), offs, rnd, stream=s) == (False, host[0])
        assert host[0] == [n != 9 for n in lens]
        out = ctypes.create_string_buffer(len(gs))
        assert m.lib().mi355_bls_pairing_check_each_device(c._h, d_p.data_ptr() + 1, d_q.data_ptr(), (ctypes.c_size_t * len(offs))(*offs), len(gs), 0, out, None,
                                                           None) == ERR_ARG      # a misaligned device pointer
        torch.cuda.synchronize()
    finally:
        c.close()
    assert live() == before
