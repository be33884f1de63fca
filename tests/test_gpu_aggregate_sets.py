"""Per-set key aggregation on the device (mi355_bls_aggregate_sets, mi355_bls_fast_aggregate_verify_each, mi355_bls_batch_fast_aggregate_verify):
aggregateAll (blst_min_pubkey_sig_core.nim:179-195) for the key list of every set in one pass, then the existing verification paths on the
records.  Aggregates, status bytes and verdicts are held bit-exact to tests/golden/aggregate_sets.json and to the C restatement; a list's
record and verdict must not depend on its position, on its neighbours, on how the keys are supplied or on the slice it falls into."""
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
    c = m.BatchedBLSVerifierCache.init(max_sets=4096, numThreads=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def C():
    from test_aggsets_plan import plan_aggsets_lib
    return plan_aggsets_lib().aggsets_plan_c()


@pytest.fixture(scope="module")
def drawn(C):
    """300 key lists of 1 .. 2 C^2 + 3 keys from the C restatement's generator, one message and one signature (by the sum of the secret keys)
    each; about 5 % corrupted.  -> (pool of all keys, [(keys, msg, sig)], aggregates, verdicts, corrupted positions), all from c_oracle;
    computed once, never changed."""
    import c_oracle as co
    rng = random.Random(20261017)
    lengths = [rng.randint(1, 2 * C * C + 3) for _ in range(300)]
    segs, pool, at = [], [], 0
    for s, n in enumerate(lengths):
        pks, sk = co.make_pks(n, seed=1000 + at)
        msg = hashlib.sha256(b"aggregate sets msg %d" % s).digest()
        segs.append([pks, msg, co.sign(sk, msg)])
        pool.append(pks)
        at += n
    bad = sorted(rng.sample(range(300), 15))
    for j, s in enumerate(bad):
        pks, msg, sig = segs[s]
        if j % 3 == 0:
            segs[s][1] = bytes([msg[0] ^ 1]) + msg[1:]                          # wrong message
        elif j % 3 == 1:
            other = segs[(s + 1) % 300][0][:96]
            at_key = rng.randrange(len(pks) // 96)
            segs[s][0] = pks[:96 * at_key] + other + pks[96 * at_key + 96:]     # a key swapped for a neighbour's
        else:
            segs[s][2] = bytes(192)                                             # infinity signature
    segs = [tuple(x) for x in segs]
    aggs = [co.g1_sum(pks) for pks, _, _ in segs]
    verdicts = [co.fast_aggregate_verify(pks, msg, sig) for pks, msg, sig in segs]
    assert [s for s, v in enumerate(verdicts) if not v] == bad
    return b"".join(pool), segs, aggs, verdicts, bad


def lists_of(segs):
    return [s[0] for s in segs], b"".join(s[1] for s in segs), b"".join(s[2] for s in segs)


def run_each(m, cache, segs):
    """-> (records, status, verdicts) of the lists through aggregateSets and fastAggregateVerifyEach"""
    keys, msgs, sigs = lists_of(segs)
    _, rec, st = m.aggregateSets(cache, keys, msgs, sigs)
    return [rec[320 * i:320 * i + 320] for i in range(len(segs))], st, m.fastAggregateVerifyEach(cache, keys, msgs, sigs)


def test_fixture_bit_exact_in_both_modes(m):
    import torch
    from util import golden
    from test_aggsets_emu import fixture_inputs, indexed_inputs
    fx = golden("aggregate_sets")
    segs = fx["segments"]
    keys, offsets, msgs, sigs, want, status = fixture_inputs(fx)
    verdicts = [bool(s["verdict"]) for s in segs]
    rnd = hashlib.sha256(b"aggregate sets rnd").digest()
    good = [i for i, s in enumerate(segs) if s["verdict"]]
    as_lists = [bytes.fromhex(s["keys"]) for s in segs]

    def pick(which):
        return ([as_lists[i] for i in which], b"".join(msgs[32 * i:32 * i + 32] for i in which), b"".join(sigs[192 * i:192 * i + 192] for i in which))
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            assert m.aggregateSets(c, as_lists, msgs, sigs) == (False, want, status), coop                   # the host form, lists laid end to end
            assert m.aggregateSets(c, (keys, None, offsets), msgs, sigs) == (False, want, status), coop
            table, idx, ioffs, iwant, istatus = indexed_inputs(False, fx)
            assert m.aggregateSets(c, (table, idx, ioffs), msgs, sigs) == (False, iwant, istatus), coop      # the indexed form
            assert m.fastAggregateVerifyEach(c, (table, idx, ioffs), msgs, sigs) == verdicts, coop
            table, idx, ioffs, iwant, istatus = indexed_inputs(True, fx)
            assert 3 in istatus
            assert m.aggregateSets(c, (table, idx, ioffs), msgs, sigs) == (False, iwant, istatus), coop      # one index past the table: status 3
            bad_seg = fx["indexed"]["bad_index"]["segment"]
            assert m.fastAggregateVerifyEach(c, (table, idx, ioffs), msgs, sigs) == [v and i != bad_seg for i, v in enumerate(verdicts)], coop
            assert m.fastAggregateVerifyEach(c, as_lists, msgs, sigs) == verdicts, coop
            ok, rec, st = m.aggregateSets(c, *pick(good))
            assert ok is True and st == bytes(len(good)) and rec == b"".join(want[320 * i:320 * i + 320] for i in good)
            assert m.batchVerifyParallel(c, rec, rnd) is True
            assert m.batchFastAggregateVerify(c, *pick(good), rnd) is True, coop
            for kind in ("wrong_signature", "wrong_message", "empty", "p_negp"):                             # one bad list added: by the check, or by its status
                extra = [s["kind"] for s in segs].index(kind)
                assert m.batchFastAggregateVerify(c, *pick(good[:3] + [extra] + good[3:]), rnd) is False, (coop, kind)
            assert m.batchFastAggregateVerify(c, (table, idx, ioffs), msgs, sigs, rnd) is False
        # the device forms: everything resident, offsets on the host
        dev = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in (keys, msgs, sigs)]
        out = torch.zeros(320 * len(segs), dtype=torch.uint8, device="cuda")
        ok, st = m.aggregateSets_device(c, dev[0].data_ptr(), len(keys) // 96, None, offsets, dev[1].data_ptr(), dev[2].data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert (ok, st, bytes(out.cpu().numpy())) == (False, status, want)
        assert m.verifyEach_device(c, out.data_ptr(), len(segs)) == verdicts                                 # the records are ordinary SignatureSets
        table, idx, ioffs, iwant, istatus = indexed_inputs(True, fx)
        dt = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
        di = torch.tensor(idx, dtype=torch.int32).cuda()                                                   # 32-bit indices
        ok, st = m.aggregateSets_device(c, dt.data_ptr(), len(table) // 96, di.data_ptr(), ioffs, dev[1].data_ptr(), dev[2].data_ptr(), out.data_ptr())
        assert (ok, st, bytes(out.cpu().numpy())) == (False, istatus, iwant)
        assert m.fastAggregateVerifyEach_device(c, dev[0].data_ptr(), len(keys) // 96, None, offsets, dev[1].data_ptr(), dev[2].data_ptr()) == verdicts
        gk, gm, gs = pick(good)
        goffs = [0]
        for x in gk:
            goffs.append(goffs[-1] + len(x) // 96)
        dg = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in (b"".join(gk), gm, gs)]
        assert m.batchFastAggregateVerify_device(c, dg[0].data_ptr(), goffs[-1], None, goffs, dg[1].data_ptr(), dg[2].data_ptr(), rnd) is True
    finally:
        c.close()


def test_parity_with_c_oracle(m, cache, drawn):
    _, segs, aggs, verdicts, bad = drawn
    rec, st, got = run_each(m, cache, segs)
    assert st == bytes(300)
    for s in range(300):
        assert rec[s] == aggs[s] + segs[s][1] + segs[s][2], s
    assert got == verdicts
    assert [s for s, v in enumerate(got) if not v] == bad
    rnd = hashlib.sha256(b"aggregate sets parity").digest()
    valid = [segs[s] for s in range(300) if verdicts[s]]
    keys, msgs, sigs = lists_of(valid)
    assert m.batchFastAggregateVerify(cache, keys, msgs, sigs, rnd) is True
    keys, msgs, sigs = lists_of(valid[:100] + [segs[bad[0]]] + valid[100:])
    assert m.batchFastAggregateVerify(cache, keys, msgs, sigs, rnd) is False


def test_independence(m, cache, drawn):
    pool, segs, aggs, verdicts, bad = drawn
    which = sorted(set(range(40)) | set(bad[:6]))
    base = [segs[s] for s in which]
    rec0, st0, v0 = run_each(m, cache, base)
    assert v0 == [verdicts[s] for s in which] and [r[:96] for r in rec0] == [aggs[s] for s in which]
    rng = random.Random(5)
    perm = list(range(len(base)))
    rng.shuffle(perm)
    rec, st, v = run_each(m, cache, [base[p] for p in perm])                    # permuted
    assert [rec[perm.index(i)] for i in range(len(base))] == rec0 and [v[perm.index(i)] for i in range(len(base))] == v0
    mixed, at = [], []                                                          # other neighbours, of other lengths, empty ones among them
    for i, b in enumerate(base):
        for _ in range(rng.randrange(3)):
            o = segs[rng.randrange(100, 300)]
            n = rng.randrange(len(o[0]) // 96 + 1)
            mixed.append((o[0][:96 * n], o[1], o[2]))
        at.append(len(mixed))
        mixed.append(b)
    rec, st, v = run_each(m, cache, mixed)
    assert [rec[p] for p in at] == rec0 and [v[p] for p in at] == v0 and all(st[p] == 0 for p in at)
    # the same keys through indices into the pool of all keys
    where = {pool[96 * i:96 * i + 96]: i for i in range(len(pool) // 96)}
    idx, offsets = [], [0]
    for pks, _, _ in base:
        idx += [where[pks[96 * j:96 * j + 96]] for j in range(len(pks) // 96)]
        offsets.append(len(idx))
    _, msgs, sigs = lists_of(base)
    ok, rec, st = m.aggregateSets(cache, (pool, idx, offsets), msgs, sigs)
    assert [rec[320 * i:320 * i + 320] for i in range(len(base))] == rec0 and st == st0
    assert m.fastAggregateVerifyEach(cache, (pool, idx, offsets), msgs, sigs) == v0


def test_consistent_with_the_single_set_call(m, cache, drawn):
    _, segs, _, verdicts, bad = drawn
    which = list(range(13)) + bad[:3]
    sub = [segs[s] for s in which]
    _, _, v = run_each(m, cache, sub)
    assert v == [m.fastAggregateVerify(cache, pks, msg, sig) for pks, msg, sig in sub] == [verdicts[s] for s in which]


def test_slicing(m, cache, drawn):
    _, segs, _, verdicts, bad = drawn
    small = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4096)
    try:
        which = [s for s in range(300) if s not in bad][:small.max_sets - 2] + bad[:3]      # max_sets + 1 lists, bad ones in the last slice
        sub = [segs[s] for s in which]
        rec_s, st_s, v_s = run_each(m, small, sub)
        rec_b, st_b, v_b = run_each(m, cache, sub)
        assert (rec_s, st_s, v_s) == (rec_b, st_b, v_b) and v_b == [verdicts[s] for s in which] == [True] * (small.max_sets - 2) + [False] * 3
        rnd = hashlib.sha256(b"aggregate sets slices").digest()
        valid = [x for x, ok in zip(sub, v_b) if ok]
        while len(valid) <= small.max_sets:
            valid.append(valid[0])
        keys, msgs, sigs = lists_of(valid)
        assert m.batchFastAggregateVerify(small, keys, msgs, sigs, rnd) is True     # more records than max_sets: the batch path slices them
    finally:
        small.close()


def test_plan_boundaries(m, cache, drawn, C):
    import c_oracle as co
    pool = drawn[0]
    lengths = [C ** j + d for j in range(1, 5) for d in (-1, 0, 1)]
    assert sum(lengths) <= len(pool) // 96
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    k = len(lengths)
    msgs, sigs = bytes(32 * k), bytes(192 * k)
    ok, rec, st = m.aggregateSets(cache, (pool, None, offsets), msgs, sigs)
    assert ok is True and st == bytes(k)
    for s in range(k):
        assert rec[320 * s:320 * s + 96] == co.g1_sum(pool[96 * offsets[s]:96 * offsets[s + 1]]), lengths[s]
    rng = random.Random(70000)                                                  # one long list: six levels
    idx = [rng.randrange(len(pool) // 96) for _ in range(70000)]
    ok, rec, st = m.aggregateSets(cache, (pool, idx, [0, len(idx)]), bytes(32), bytes(192))
    assert ok is True and rec[:96] == co.g1_sum(b"".join(pool[96 * i:96 * i + 96] for i in idx))


def test_argument_errors(m, cache, drawn):
    L = m.lib()
    pool = drawn[0][:96 * 8]
    sz = ctypes.c_size_t
    msgs, sigs = bytes(64), bytes(384)
    rec, st = ctypes.create_string_buffer(640), ctypes.create_string_buffer(b"\x07\x07", 2)
    good = (sz * 3)(0, 3, 8)
    assert L.mi355_bls_aggregate_sets(cache._h, pool, 8, None, good, 2, msgs, sigs, rec, st) == 1 and st.raw == bytes(2)
    assert L.mi355_bls_aggregate_sets(cache._h, pool, 8, None, (sz * 3)(0, 5, 3), 2, msgs, sigs, rec, st) == ERR_ARG       # decreasing
    assert L.mi355_bls_aggregate_sets(cache._h, pool, 8, None, (sz * 3)(0, 3, 9), 2, msgs, sigs, rec, st) == ERR_ARG       # past the table, no indices
    for hole in (1, 4, 6, 7, 8, 9):                                              # keys, offsets, messages, signatures, records, status
        args = [cache._h, pool, 8, None, good, 2, msgs, sigs, rec, st]
        args[hole] = None
        assert L.mi355_bls_aggregate_sets(*args) == ERR_ARG, hole
    assert L.mi355_bls_aggregate_sets(None, pool, 8, None, good, 2, msgs, sigs, rec, st) == ERR_ARG
    st2 = ctypes.create_string_buffer(b"\x07\x07", 2)
    assert L.mi355_bls_aggregate_sets(cache._h, pool, 8, None, good, 0, msgs, sigs, rec, st2) == 0 and st2.raw == b"\x07\x07"   # k = 0: 0, nothing written
    out = ctypes.create_string_buffer(2)
    assert L.mi355_bls_fast_aggregate_verify_each(cache._h, pool, 8, None, (sz * 3)(0, 5, 3), 2, msgs, sigs, out) == ERR_ARG
    assert L.mi355_bls_fast_aggregate_verify_each(cache._h, pool, 8, None, good, 0, msgs, sigs, out) == 0
    assert L.mi355_bls_fast_aggregate_verify_each(cache._h, pool, 8, None, good, 2, msgs, sigs, None) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify(cache._h, pool, 8, None, (sz * 3)(0, 3, 9), 2, msgs, sigs, bytes(32)) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify(cache._h, pool, 8, None, good, 2, msgs, sigs, None) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify(cache._h, pool, 8, None, good, 0, msgs, sigs, bytes(32)) == 0
    for fn, tail in ((L.mi355_bls_aggregate_sets_device, (None, st, None)), (L.mi355_bls_fast_aggregate_verify_each_device, (out, None)),
                     (L.mi355_bls_batch_fast_aggregate_verify_device, (bytes(32), None))):
        assert fn(cache._h, None, 8, None, good, 2, None, None, *tail) == ERR_ARG                                         # null device pointers
    with pytest.raises(ValueError):
        m.aggregateSets(cache, [pool], bytes(64), bytes(192))                                                              # one message and signature per list
    with pytest.raises(ValueError):
        m.aggregateSets(cache, (pool, [0, 1], [0, 1]), bytes(32), bytes(192))                                              # offsets[k] is not the length of idx
    assert m.aggregateSets(cache, [], b"", b"") == (False, b"", b"")
