"""Same-message pre-aggregation of many groups on the device (mi355_bls_combine_sets, mi355_bls_batch_verify_combined): MultiSignatureSet.combine
(bls_batch_verifier.nim:47-106, core :570-647) for k groups in one pass.  Records and status bytes are held bit-exact to
tests/golden/combine_sets.json and to the C restatement's combine; a group's record must not depend on its position, on its neighbours or on
how its members are addressed."""
import ctypes
import hashlib
import random

import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -3


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def C():
    from test_combsets_plan import plan_combsets_lib
    return plan_combsets_lib().plan_comb_agg_c()


def rnd_of(tag, g):
    return hashlib.sha256(b"%s %d" % (tag, g)).digest()


@pytest.fixture(scope="module")
def drawn(m, cache, C):
    """200 groups of 1 .. 2 C^2 + 3 members signed on the device, one message per group, and what the C restatement's combine gives for each.
    -> (records of all members, offsets, rnds, expected records); computed once, never changed."""
    import c_oracle as co
    rng = random.Random(20261017)
    lengths = [rng.randint(1, 2 * C * C + 3) for _ in range(200)]
    lengths[:4] = [1, 2, 5, 2 * C * C + 3]
    n = sum(lengths)
    sks = b"".join((int.from_bytes(hashlib.sha256(b"combine sets sk %d" % i).digest(), "little") >> 2 | 1).to_bytes(32, "little") for i in range(n))
    msgs = b"".join(hashlib.sha256(b"combine sets msg %d" % g).digest() * ln for g, ln in enumerate(lengths))
    ok, sets, _ = m.signSets(cache, sks, msgs)
    assert ok
    offsets = [0]
    for ln in lengths:
        offsets.append(offsets[-1] + ln)
    rnds = [rnd_of(b"combine sets rnd", g) for g in range(200)]
    want = []
    for g in range(200):
        recs = [sets[320 * i:320 * i + 320] for i in range(offsets[g], offsets[g + 1])]
        if len(recs) == 1:
            want.append(recs[0])
        else:
            pk, sg, _ = co.combine(rnds[g], b"".join(r[:96] for r in recs), b"".join(r[128:] for r in recs))
            want.append(pk + recs[0][96:128] + sg)
    return sets, offsets, rnds, want


def test_fixture_bit_exact_in_both_modes(m):
    import torch
    from util import golden
    from test_combsets_emu import fixture_inputs, indexed_inputs
    fx = golden("combine_sets")
    segs = fx["segments"]
    sets, offsets, rnds, want, status = fixture_inputs(fx)
    verdicts = [bool(s["verdict"]) for s in segs]
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            ok, rec, st = m.combineSets(c, sets, None, offsets, rnds)                                # the host form, members laid end to end
            assert st == status and ok is False, coop
            for s in range(len(segs)):
                assert rec[320 * s:320 * s + 320] == want[320 * s:320 * s + 320], (coop, segs[s]["kind"])
            assert m.verifyEach(c, rec) == verdicts, coop                                           # the records are ordinary SignatureSets
            for bad in (False, True):                                                               # the indexed form; one index past the table: status 3
                table, idx, ioffs, irnds, iwant, istatus = indexed_inputs(bad, fx)
                assert m.combineSets(c, table, idx, ioffs, irnds) == (False, iwant, istatus), (coop, bad)
            assert 3 in istatus
        # the device form: table and indices resident, offsets and random bytes on the host
        table, idx, ioffs, irnds, iwant, istatus = indexed_inputs(True, fx)
        dt = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
        di = torch.tensor(idx, dtype=torch.int64).to(torch.int32).cuda()                            # 32-bit indices
        out = torch.zeros(320 * len(segs), dtype=torch.uint8, device="cuda")
        ok, st = m.combineSets_device(c, dt.data_ptr(), len(table) // 320, di.data_ptr(), ioffs, irnds, out.data_ptr())
        torch.cuda.synchronize()
        assert (ok, st, bytes(out.cpu().numpy())) == (False, istatus, iwant)
        ds = torch.frombuffer(bytearray(sets), dtype=torch.uint8).cuda()
        ok, st = m.combineSets_device(c, ds.data_ptr(), len(sets) // 320, None, offsets, rnds, out.data_ptr())
        torch.cuda.synchronize()
        assert (ok, st, bytes(out.cpu().numpy())) == (False, status, want)
        assert m.verifyEach_device(c, out.data_ptr(), len(segs)) == verdicts
    finally:
        c.close()


def test_seeded_groups_equal_c_oracle_and_single_combine(m, cache, drawn):
    sets, offsets, rnds, want = drawn
    ok, rec, st = m.combineSets(cache, sets, None, offsets, rnds)
    assert ok is True and st == bytes(200)
    for g in range(200):
        assert rec[320 * g:320 * g + 320] == want[g], (g, offsets[g + 1] - offsets[g])
    for g in (1, 2, 3, 50, 199):                                                                    # the one-group call gives the same record
        recs = [sets[320 * i:320 * i + 320] for i in range(offsets[g], offsets[g + 1])]
        if len(recs) >= 2:
            one = m.MultiSignatureSet.init([r[:96] for r in recs], recs[0][96:128], [r[128:] for r in recs]).combine(cache, rnds[g])
            assert b"".join(one) == want[g], g


def test_permuting_the_groups_permutes_the_records(m, cache, drawn):
    sets, offsets, rnds, want = drawn
    perm = list(range(200))
    random.Random(5).shuffle(perm)
    # the same table, the groups in another order, every member through an index
    idx, poffs = [], [0]
    for g in perm:
        idx += list(range(offsets[g], offsets[g + 1]))
        poffs.append(len(idx))
    ok, rec, st = m.combineSets(cache, sets, idx, poffs, [rnds[g] for g in perm])
    assert ok is True and st == bytes(200)
    assert [rec[320 * j:320 * j + 320] for j in range(200)] == [want[g] for g in perm]
    # a range that starts late, contiguous
    ok, rec, st = m.combineSets(cache, sets, None, offsets[120:], rnds[120:])
    assert ok is True and rec == b"".join(want[120:])


def test_batch_verify_combined(m, cache, drawn):
    from util import golden
    from test_combsets_emu import fixture_inputs, table_records
    sets, offsets, rnds, want = drawn
    rnd = hashlib.sha256(b"combine sets batch").digest()
    k = 70
    assert k > cache.max_sets and offsets[k] > cache.max_sets                                       # groups and members both exceed max_sets
    sub, soffs, srnds = sets[:320 * offsets[k]], offsets[:k + 1], rnds[:k]
    assert m.batchVerifyCombined(cache, sub, None, soffs, srnds, rnd) is True
    assert m.batchVerifyParallel(cache, sub, rnd) is True                                           # the route without combine agrees
    assert m.batchVerifyParallel(cache, b"".join(want[:k]), rnd) is True
    at = offsets[40] + 1                                                                            # one bad member: its signature swapped for a neighbour's
    bad = sub[:320 * at + 128] + sub[320 * (at - 1) + 128:320 * at] + sub[320 * at + 320:]
    assert m.batchVerifyCombined(cache, bad, None, soffs, srnds, rnd) is False
    assert m.batchVerifyParallel(cache, bad, rnd) is False
    import torch
    d = torch.frombuffer(bytearray(sub), dtype=torch.uint8).cuda()
    assert m.batchVerifyCombined_device(cache, d.data_ptr(), offsets[k], None, soffs, srnds, rnd) is True
    d = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
    assert m.batchVerifyCombined_device(cache, d.data_ptr(), offsets[k], None, soffs, srnds, rnd) is False
    # every non-zero status ends the call with False
    fx = golden("combine_sets")
    tab = table_records(fx)
    good = [s for s in fx["segments"] if s["verdict"]][:6]

    def run(segs, patch=None):
        idx, foffs = [], [0]
        for s in segs:
            idx += s["members"]
            foffs.append(len(idx))
        if patch:
            idx[patch[0]] = patch[1]
        return m.batchVerifyCombined(cache, b"".join(tab), idx, foffs, [bytes.fromhex(s["rnd"]) for s in segs], rnd)
    assert run(good) is True
    by = {s["kind"]: s for s in fx["segments"]}
    for kind in ("empty", "cancel", "mixed", "inf_key", "wrong_signature", "inf_sig"):
        assert run(good[:3] + [by[kind]] + good[3:]) is False, kind
    assert run(good, patch=(2, len(tab) + 1)) is False                                              # status 3


def test_group_by_message_then_combined(m, cache, drawn):
    sets, offsets, rnds, _ = drawn
    members = [(g, i) for g in range(100, 140) for i in range(offsets[g], min(offsets[g + 1], offsets[g] + 6))]
    random.Random(9).shuffle(members)
    flat = b"".join(sets[320 * i:320 * i + 320] for _, i in members)
    idx, goffs = m.groupByMessage(flat)
    assert len(goffs) == 41 and sorted(idx) == list(range(len(members)))
    rnd = hashlib.sha256(b"combine sets grouped").digest()
    assert m.batchVerifyCombined(cache, flat, idx, goffs, [rnd_of(b"grouped", g) for g in range(40)], rnd) is True
    swapped = flat[:128] + flat[320 + 128:640] + flat[320:]                                         # member 0 carries member 1's signature
    assert m.batchVerifyCombined(cache, swapped, idx, goffs, [rnd_of(b"grouped", g) for g in range(40)], rnd) is False


def test_resources_return_to_baseline(m, drawn):
    sets, offsets, rnds, want = drawn
    L = m.lib()
    base = L.mi355_bls_debug_live_resources()
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    made = L.mi355_bls_debug_live_resources()
    ok, rec, st = m.combineSets(c, sets, list(range(offsets[20])), offsets[:21], rnds[:20])
    assert ok is True and rec == b"".join(want[:20])
    assert L.mi355_bls_debug_live_resources() > made                                                # the call's buffers have owners ...
    c.close()
    assert L.mi355_bls_debug_live_resources() == base                                               # ... and go with the context


def test_argument_errors(m, cache, drawn):
    sets = drawn[0][:320 * 8]
    L = m.lib()
    sz = ctypes.c_size_t
    rnds = bytes(64)
    rec, st = ctypes.create_string_buffer(640), ctypes.create_string_buffer(b"\x07\x07", 2)
    good = (sz * 3)(0, 3, 8)
    assert L.mi355_bls_combine_sets(cache._h, sets, 8, None, good, 2, rnds, rec, st) in (0, 1) and st.raw != b"\x07\x07"
    assert L.mi355_bls_combine_sets(cache._h, sets, 8, None, (sz * 3)(0, 5, 3), 2, rnds, rec, st) == ERR_ARG        # decreasing
    assert L.mi355_bls_combine_sets(cache._h, sets, 8, None, (sz * 3)(0, 3, 9), 2, rnds, rec, st) == ERR_ARG        # past the table, no indices
    for hole in (1, 4, 6, 7, 8):                                                                    # records, offsets, rnds, out, status
        args = [cache._h, sets, 8, None, good, 2, rnds, rec, st]
        args[hole] = None
        assert L.mi355_bls_combine_sets(*args) == ERR_ARG, hole
    assert L.mi355_bls_combine_sets(None, sets, 8, None, good, 2, rnds, rec, st) == ERR_ARG
    st2 = ctypes.create_string_buffer(b"\x07\x07", 2)
    assert L.mi355_bls_combine_sets(cache._h, sets, 8, None, good, 0, rnds, rec, st2) == 0 and st2.raw == b"\x07\x07"   # k = 0: 0, nothing written
    assert L.mi355_bls_combine_sets_device(cache._h, None, 8, None, good, 2, rnds, None, st, None) == ERR_ARG
    assert L.mi355_bls_batch_verify_combined(cache._h, sets, 8, None, good, 2, rnds, None) == ERR_ARG
    assert L.mi355_bls_batch_verify_combined(cache._h, sets, 8, None, good, 0, rnds, bytes(32)) == 0
    assert L.mi355_bls_batch_verify_combined(cache._h, sets, 8, None, (sz * 3)(0, 5, 3), 2, rnds, bytes(32)) == ERR_ARG
    assert L.mi355_bls_batch_verify_combined_device(cache._h, None, 8, None, good, 2, rnds, bytes(32), None) == ERR_ARG
    with pytest.raises(ValueError):
        m.combineSets(cache, sets, None, [0, 3, 8], bytes(32))                                      # 32 random bytes per group
    with pytest.raises(ValueError):
        m.combineSets(cache, sets, [0, 1], [0, 1], bytes(32))                                       # offsets[k] is not the length of idx
    assert m.combineSets(cache, sets, None, [0], b"") == (False, b"", b"")
