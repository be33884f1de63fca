"""Per-set verdicts on the device (mi355_bls_verify_each, mi355_bls_batch_verify_locate): verify = coreVerifyNoGroupCheck
(bls_sig_min_pubkey.nim:108-125, blst_min_pubkey_sig_core.nim:269-297) for every set of the input in one pass.  Verdicts and values are held
bit-exact to tests/golden/verify_each.json and to the C restatement; a set's verdict must not depend on its position, its neighbours, the
slice it falls into or the executor its size selects."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("wrong_message", "other_key", "infinity_signature", "infinity_public_key", "doubled_signature")


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=65536, numThreads=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def signed(m, cache):
    """66 000 valid sets from the device signer (deterministic keys and messages): every larger test cuts its inputs from these"""
    n = 66000
    sks = b"".join(hashlib.sha256(b"each sk %d" % i).digest()[:31] + b"\x00" for i in range(n))
    msgs = b"".join(hashlib.sha256(b"each msg %d" % i).digest() for i in range(n))
    ok, rec, _ = m.signSets(cache, sks, msgs)
    assert ok
    return [rec[320 * i:320 * i + 320] for i in range(n)]


def corrupt(rec, kind, other):
    import c_oracle as co
    pk, msg, sig = rec[:96], rec[96:128], rec[128:]
    if kind == "wrong_message":
        msg = bytes([msg[0] ^ 1]) + msg[1:]
    elif kind == "other_key":
        sig = other[128:]
    elif kind == "infinity_signature":
        sig = bytes(192)
    elif kind == "infinity_public_key":
        pk = bytes(96)
    elif kind == "doubled_signature":
        sig = co.g2_mul(sig, 2)
    return pk + msg + sig


def oracle_verdict(rec):
    import c_oracle as co
    return co.core_verify(rec[:96], rec[96:128], rec[128:])


def with_bad(sets, bad_at, seed):
    """copies of `sets` with the sets at bad_at corrupted by a seeded choice among the fixture's kinds"""
    rng = random.Random(seed)
    out = list(sets)
    for i in bad_at:
        out[i] = corrupt(sets[i], rng.choice(KINDS), sets[(i + 1) % len(sets)])
    return out


def test_fixture_sets_bit_exact_in_both_modes(m):
    from util import golden
    fx = golden("verify_each")["sets"]
    rec = b"".join(bytes.fromhex(s["set"]) for s in fx)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            ok, gts = m.verifyEachValues(c, rec)
            assert ok == [bool(s["verdict"]) for s in fx], coop
            assert [g.hex() for g in gts] == [s["gt"] for s in fx], coop
            assert m.verifyEach(c, rec) == ok
            out = ctypes.create_string_buffer(len(fx))
            assert m.lib().mi355_bls_verify_each(c._h, rec, len(fx), out) == 0       # not every set verified
            assert list(out.raw) == [s["verdict"] for s in fx]
            good = b"".join(bytes.fromhex(s["set"]) for s in fx if s["verdict"])
            assert m.lib().mi355_bls_verify_each(c._h, good, len(good) // 320, out) == 1
            assert m.lib().mi355_bls_verify_each(c._h, good, 0, out) == 0             # n = 0: 0, nothing written
    finally:
        c.close()


def test_position_and_neighbour_independence(m, cache, signed):
    rng = random.Random(7)
    base = with_bad(signed[:200], rng.sample(range(200), 40), 11)
    want = [oracle_verdict(r) for r in base]
    assert want.count(False) == 40
    alone = m.verifyEach(cache, b"".join(base))
    assert alone == want
    perm = list(range(200))
    rng.shuffle(perm)
    got = m.verifyEach(cache, b"".join(base[p] for p in perm))
    assert [got[perm.index(i)] for i in range(200)] == alone
    others = with_bad(signed[1000:6000], rng.sample(range(5000), 100), 13)
    at = sorted(rng.sample(range(5200), 200))
    mixed, it, k = [], iter(others), 0
    for pos in range(5200):
        if k < 200 and pos == at[k]:
            mixed.append(base[k])
            k += 1
        else:
            mixed.append(next(it))
    got = m.verifyEach(cache, b"".join(mixed))
    assert [got[p] for p in at] == alone


def test_parity_with_c_oracle_2048(m, cache):
    import c_oracle as co
    raw = co.make_batch(2048, seed=20261)
    sets = [raw[320 * i:320 * i + 320] for i in range(2048)]
    bad = random.Random(3).sample(range(2048), 61)                                    # about 3 %
    sets = with_bad(sets, bad, 5)
    got = m.verifyEach(cache, b"".join(sets))
    want = [oracle_verdict(r) for r in sets]                                          # every one of them
    assert got == want
    assert [i for i, v in enumerate(got) if not v] == sorted(bad)


def test_every_hand_over_size(m, signed):
    import torch
    from test_vereach_plan import plan_each_lib
    pl = plan_each_lib()
    S = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    sizes = sorted({t + d for t in (pl.each_plan_engine_max(S), pl.each_plan_team_lines_max(S), pl.each_plan_team_clear_max(S)) for d in (-1, 0, 1)})
    c = m.BatchedBLSVerifierCache.init(max_sets=max(sizes), numThreads=4096)          # latency mode: the mode in which the executors change
    try:
        for n in sizes:
            bad = [0, n // 2, n - 1]
            sets = with_bad(signed[:n], bad, n)
            got = m.verifyEach(c, b"".join(sets))
            assert [i for i, v in enumerate(got) if not v] == bad, n                  # by construction
            rng = random.Random(n)
            for i in bad + rng.sample(sorted(set(range(n)) - set(bad)), 61):            # 64 distinct sets
                assert got[i] == oracle_verdict(sets[i]), (n, i)
    finally:
        c.close()


def test_scale_and_slicing(m, cache, signed):
    import c_oracle as co
    n = 65536
    small = m.BatchedBLSVerifierCache.init(max_sets=8192, numThreads=4096)
    try:
        from test_vereach_plan import plan_each_lib, slices
        bounds = set()
        for first, cnt in slices(plan_each_lib(), n, 8192)[1]:                        # the small context's slices, as the plan cuts them
            bounds |= {first, first + cnt - 1}
        bad = sorted(bounds)
        assert len(bad) == 16 and bad[0] == 0 and bad[-1] == n - 1
        assert slices(plan_each_lib(), n, 65536)[1] == [(0, n)]                       # one slice on the large one
        sets = with_bad(signed[:n], bad, 17)
        rec = b"".join(sets)
        v_small, gt_small = m.verifyEachValues(small, rec)
        v_big, gt_big = m.verifyEachValues(cache, rec)
        assert v_small == v_big
        assert [i for i, v in enumerate(v_big) if not v] == bad
        with_value = [i for i in bad if sets[i][:96] != bytes(96)]                  # corrupted sets: values that are not one (an infinity key leaves the oracle no value)
        assert len(with_value) >= 8
        for i in with_value + random.Random(23).sample(sorted(set(range(n)) - set(bad)), 32 - len(with_value)):
            want_ok, want_gt = co.aggregate_verify([sets[i][:96]], [sets[i][96:128]], sets[i][128:], gt=True)
            assert (v_big[i], gt_big[i]) == (want_ok, want_gt) and gt_small[i] == want_gt, i
    finally:
        small.close()


def test_batch_verify_locate(m, cache, signed):
    rnd = hashlib.sha256(b"locate").digest()
    sets = signed[:3000]
    before = m.verifyEachPasses(cache)
    assert m.batchVerifyLocate(cache, b"".join(sets), rnd) == (True, [True] * 3000)
    assert m.verifyEachPasses(cache) == before                                        # a passing batch pays for no per-set pass
    one = with_bad(sets, [1234], 1)
    ok, v = m.batchVerifyLocate(cache, b"".join(one), rnd)
    assert ok is False and [i for i, x in enumerate(v) if not x] == [1234]
    assert m.verifyEachPasses(cache) == before + 1
    swapped = list(sets)
    a, b = swapped[10], swapped[2000]
    swapped[10], swapped[2000] = a[:128] + b[128:], b[:128] + a[128:]                 # each bad on its own
    ok, v = m.batchVerifyLocate(cache, b"".join(swapped), rnd)
    assert ok is False and [i for i, x in enumerate(v) if not x] == [10, 2000]
    assert m.batchVerifyLocate(cache, b"", rnd) == (False, [])


def test_argument_validation(m, cache):
    with pytest.raises(ValueError):
        m.verifyEach(cache, bytes(319))
    with pytest.raises(ValueError):
        m.batchVerifyLocate(cache, bytes(641), bytes(32))
    with pytest.raises(ValueError):
        m.batchVerifyLocate(cache, bytes(640), bytes(31))
    assert m.verifyEach(cache, b"") == []


def test_per_set_call_leaves_the_batch_workspace_intact(m):
    """The per-set path runs in a pair store of its own: a batch's committed state survives a per-set call on the same context, fetch_stage
    shows no batch stages behind it (the last call left none), and the same batch verifies again to the same GT bytes."""
    import c_oracle as co
    rnd = hashlib.sha256(b"each beside batch").digest()
    rec = co.make_batch(8, seed=20262)
    ok, st = co.batch_verify(rec, rnd, 4, stages=True)
    assert ok
    sets = with_bad([rec[320 * i:320 * i + 320] for i in range(8)], [3], 1)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        assert m.batchVerifyParallel(c, rec, rnd) is True
        gt, state = c.fetch(4, 576), c.fetch(5, 576)
        assert gt == st["gt"]
        assert o_affine_g2(c.fetch(1, 288 * 8)[:288]) == st["H"][:192]
        assert m.verifyEach(c, b"".join(sets)) == [oracle_verdict(r) for r in sets] == [i != 3 for i in range(8)]
        assert c.fetch(5, 576) == state                                               # the batch's committed state
        assert c.fetch(0, 0) == b""                                                   # no tuples of a batch to show ...
        for what, nbytes in ((1, 288 * 8), (2, 144 * 8), (4, 576)):                   # ... no pairs, and no GT of the last call
            with pytest.raises(m.BlsGpuError):
                c.fetch(what, nbytes)
        assert m.batchVerifyParallel(c, rec, rnd) is True
        assert c.fetch(4, 576) == gt and c.fetch(5, 576) == state
        assert o_affine_g2(c.fetch(1, 288 * 8)[:288]) == st["H"][:192]
    finally:
        c.close()


def o_affine_g2(jac288):
    import bls12381_py as o
    from util import g2_jac_to_affine
    return o.g2_to_blst_affine(g2_jac_to_affine(jac288))
