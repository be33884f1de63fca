"""Key aggregation by participation bits on the device (mi355_bls_aggregate_sets_bits, mi355_bls_fast_aggregate_verify_each_bits,
mi355_bls_batch_fast_aggregate_verify_bits): committees and one bit per committee position in, the records of aggregateSets out - the
participants summed (aggregateAll, blst_min_pubkey_sig_core.nim:179-195) or the absentees subtracted from the committee's aggregate
(subtractAll, :197-209).  Records, status bytes and verdicts are held bit-exact to tests/golden/aggregate_bits.json, to aggregateSets over
the expanded index lists and to the C restatement; the route taken is held to the fixture's prediction and never shows in a record."""
import ctypes
import hashlib
import random

import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -3
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
C2 = 2 * 64 + 3


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4096)      # 300 records: the verification passes slice
    yield c
    c.close()


def pack(flags):
    b = bytearray((len(flags) + 7) // 8)
    for i, v in enumerate(flags):
        b[i // 8] |= int(v) << (i % 8)
    return bytes(b)


@pytest.fixture(scope="module")
def drawn():
    """40 committees of 1 .. 2 * 64 + 3 keys drawn from one table of the C restatement's keys, and 300 sets on them with 5, 50, 95 or 100 %
    participation, a message and a signature by the sum of the participants' secret keys; 15 of them corrupted.  Everything the tests
    compare with comes from c_oracle; computed once, never changed."""
    import c_oracle as co
    rng = random.Random(20261019)
    n_table = 1500
    table, _ = co.make_pks(n_table, seed=77000)
    sks = []
    for i in range(n_table):
        sk = bytearray(hashlib.sha256(b"sk" + (77000 + i).to_bytes(8, "little")).digest())
        sk[31] &= 0x3f
        sk[0] |= 1
        sks.append(int.from_bytes(sk, "little"))
    lengths = [1, 7, 8, 9, 63, 64, 65, C2] + [rng.randint(1, C2) for _ in range(32)]
    idx, c_offsets = [], [0]
    for n in lengths:
        idx += rng.sample(range(n_table), n)
        c_offsets.append(len(idx))
    sets = []
    for s in range(300):
        c = rng.randrange(len(lengths))
        L, pct = lengths[c], rng.choice((5, 50, 95, 100))
        flags = [pct == 100 or rng.randrange(100) < pct for _ in range(L)]
        if not any(flags):
            flags[rng.randrange(L)] = True
        msg = hashlib.sha256(b"aggregate bits msg %d" % s).digest()
        sets.append([c, flags, msg, None])
    bad = sorted(rng.sample(range(300), 15))
    for s, (c, flags, msg, _) in enumerate(sets):
        members = [idx[c_offsets[c] + i] for i, v in enumerate(flags) if v]
        sets[s][3] = co.sign(sum(sks[t] for t in members) % R, msg)
    for j, s in enumerate(bad):
        c, flags, msg, sig = sets[s]
        if j % 3 == 0:
            sets[s][2] = bytes([msg[0] ^ 1]) + msg[1:]                          # wrong message
        elif j % 3 == 1 and len(flags) > 1:
            at = rng.randrange(len(flags))                                      # one position's bit flipped (never the only participant)
            if flags[at] and sum(flags) == 1:
                at = (at + 1) % len(flags)
            flags[at] = not flags[at]
        else:
            sets[s][3] = bytes(192)                                             # infinity signature
    out = []
    for c, flags, msg, sig in sets:
        members = [idx[c_offsets[c] + i] for i, v in enumerate(flags) if v]
        keys = b"".join(table[96 * t:96 * t + 96] for t in members)
        out.append({"committee": c, "flags": flags, "bits": pack(flags), "members": members, "msg": msg, "sig": sig, "agg": co.g1_sum(keys),
                    "verdict": co.fast_aggregate_verify(keys, msg, sig), "route": int(2 * sum(flags) > len(flags))})
    assert [s for s, d in enumerate(out) if not d["verdict"]] == bad
    return {"table": table, "idx": idx, "c_offsets": c_offsets, "lengths": lengths, "sets": out, "bad": bad}


@pytest.fixture(scope="module")
def bases(m, cache, drawn):
    """the committees' own aggregates as a host makes them once per epoch: the records of aggregateSets over the committees (stride 320)"""
    mcount = len(drawn["lengths"])
    ok, rec, st = m.aggregateSets(cache, (drawn["table"], drawn["idx"], drawn["c_offsets"]), bytes(32 * mcount), bytes(192 * mcount))
    assert ok is True and st == bytes(mcount)
    return rec


def run_bits(m, cache, drawn, sets, aggs=None, stride=320):
    com = (drawn["table"], drawn["idx"], drawn["c_offsets"])
    which, bits = [d["committee"] for d in sets], [d["bits"] for d in sets]
    msgs, sigs = b"".join(d["msg"] for d in sets), b"".join(d["sig"] for d in sets)
    _, rec, st = m.aggregateSetsBits(cache, com, which, bits, msgs, sigs, aggs, stride)
    return [rec[320 * i:320 * i + 320] for i in range(len(sets))], st, m.debug_aggregate_bits_routes(cache)


def test_fixture_bit_exact_in_both_modes(m):
    import torch
    from util import golden
    from test_aggbits_emu import as_records, fixture_inputs
    fx = golden("aggregate_bits")
    f = fixture_inputs(fx)
    k, excl = len(f["which"]), sum(f["routes"])
    com = (f["table"], f["idx"], f["c_offsets"])
    rnd = hashlib.sha256(b"aggregate bits rnd").digest()
    good = [i for i, v in enumerate(f["verdicts"]) if v]
    kinds = [s["kind"] for s in fx["sets"]]
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            for aggs, stride, routes in ((f["aggs"], 96, (k - excl, excl)), (as_records(f["aggs"]), 320, (k - excl, excl)), (None, 96, (k, 0))):
                got = m.aggregateSetsBits(c, com, f["which"], f["bits"], f["msgs"], f["sigs"], aggs, stride)
                assert got == (False, f["want"], f["status"]), (coop, stride, aggs is None)                 # the same bytes with and without bases
                assert m.debug_aggregate_bits_routes(c) == routes, (coop, stride)
                assert m.fastAggregateVerifyEachBits(c, com, f["which"], b"".join(f["bits"]), f["msgs"], f["sigs"], aggs, stride) == f["verdicts"], coop
                assert m.debug_aggregate_bits_routes(c) == routes
                g = fixture_inputs(fx, good)
                assert sum(g["routes"]) > 0
                assert m.aggregateSetsBits(c, com, g["which"], g["bits"], g["msgs"], g["sigs"], aggs, stride) == (True, g["want"], bytes(len(good)))
                assert m.batchFastAggregateVerifyBits(c, com, g["which"], g["bits"], g["msgs"], g["sigs"], rnd, aggs, stride) is True, coop
                for kind in ("wrong_signature", "wrong_message", "none_set", "p_negp_r_110", "oor_participating") if stride == 96 else ():
                    g = fixture_inputs(fx, good[:3] + [kinds.index(kind)] + good[3:])                         # one bad set added
                    assert m.batchFastAggregateVerifyBits(c, com, g["which"], g["bits"], g["msgs"], g["sigs"], rnd, aggs, stride) is False, (coop, kind)
        # the device forms: everything resident, the committee offsets and numbers on the host
        def dev(b):
            return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        d_table, d_msgs, d_sigs, d_aggs, d_recs = dev(f["table"]), dev(f["msgs"]), dev(f["sigs"]), dev(f["aggs"]), dev(as_records(f["aggs"]))
        d_bits = dev(b"\0" + b"".join(f["bits"]))[1:]                                                         # byte-aligned only
        assert d_bits.data_ptr() % 2 == 1
        d_idx = torch.tensor(f["idx"], dtype=torch.int32).cuda()
        out = torch.zeros(320 * k, dtype=torch.uint8, device="cuda")
        n_table = len(f["table"]) // 96
        for d_a, stride, routes in ((d_aggs.data_ptr(), 96, (k - excl, excl)), (d_recs.data_ptr(), 320, (k - excl, excl)), (None, 96, (k, 0))):
            out.zero_()
            ok, st = m.aggregateSetsBits_device(c, d_table.data_ptr(), n_table, d_idx.data_ptr(), f["c_offsets"], d_a, stride, f["which"], d_bits.data_ptr(),
                                                d_msgs.data_ptr(), d_sigs.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            assert (ok, st, bytes(out.cpu().numpy())) == (False, f["status"], f["want"]), stride
            assert m.debug_aggregate_bits_routes(c) == routes
            assert m.verifyEach_device(c, out.data_ptr(), k) == f["verdicts"]                                  # the records are ordinary SignatureSets
            assert m.fastAggregateVerifyEachBits_device(c, d_table.data_ptr(), n_table, d_idx.data_ptr(), f["c_offsets"], d_a, stride, f["which"],
                                                        d_bits.data_ptr(), d_msgs.data_ptr(), d_sigs.data_ptr()) == f["verdicts"]
        g = fixture_inputs(fx, good)
        dg = [dev(b) for b in (b"".join(g["bits"]), g["msgs"], g["sigs"])]
        for d_a in (d_aggs.data_ptr(), None):
            assert m.batchFastAggregateVerifyBits_device(c, d_table.data_ptr(), n_table, d_idx.data_ptr(), f["c_offsets"], d_a, 96, g["which"], dg[0].data_ptr(),
                                                         dg[1].data_ptr(), dg[2].data_ptr(), rnd) is True
    finally:
        c.close()


def test_parity_with_aggregate_sets_and_c_oracle(m, cache, drawn, bases):
    sets = drawn["sets"]
    # the existing call over the expanded index lists: not the code under test
    idx, offsets = [], [0]
    for d in sets:
        idx += d["members"]
        offsets.append(len(idx))
    msgs, sigs = b"".join(d["msg"] for d in sets), b"".join(d["sig"] for d in sets)
    ok, want, st_want = m.aggregateSets(cache, (drawn["table"], idx, offsets), msgs, sigs)
    assert ok is True and st_want == bytes(300)
    excl = sum(d["route"] for d in sets)
    assert 60 < excl < 240                                                       # both routes well used
    for aggs, routes in ((bases, (300 - excl, excl)), (None, (300, 0))):
        rec, st, got_routes = run_bits(m, cache, drawn, sets, aggs)
        assert st == bytes(300) and got_routes == routes
        for s, d in enumerate(sets):
            assert rec[s] == want[320 * s:320 * s + 320] == d["agg"] + d["msg"] + d["sig"], (s, aggs is None)
    com = (drawn["table"], drawn["idx"], drawn["c_offsets"])
    which, bits = [d["committee"] for d in sets], [d["bits"] for d in sets]
    got = m.fastAggregateVerifyEachBits(cache, com, which, bits, msgs, sigs, bases, 320)
    assert got == [d["verdict"] for d in sets]
    assert [s for s, v in enumerate(got) if not v] == drawn["bad"]
    rnd = hashlib.sha256(b"aggregate bits parity").digest()
    valid = [d for d in sets if d["verdict"]]
    for pick, verdict in ((valid, True), (valid[:100] + [sets[drawn["bad"][0]]] + valid[100:], False)):
        assert m.batchFastAggregateVerifyBits(cache, com, [d["committee"] for d in pick], [d["bits"] for d in pick], b"".join(d["msg"] for d in pick),
                                              b"".join(d["sig"] for d in pick), rnd, bases, 320) is verdict


def test_independence(m, cache, drawn, bases):
    sets = drawn["sets"]
    which = sorted(set(range(40)) | set(drawn["bad"][:6]))
    base = [sets[s] for s in which]
    rec0, st0, routes0 = run_bits(m, cache, drawn, base, bases)
    assert [r[:96] for r in rec0] == [d["agg"] for d in base] and st0 == bytes(len(base))
    assert routes0 == (len(base) - sum(d["route"] for d in base), sum(d["route"] for d in base)) and 0 < routes0[1] < len(base)
    rng = random.Random(5)
    perm = list(range(len(base)))
    rng.shuffle(perm)
    rec, st, _ = run_bits(m, cache, drawn, [base[p] for p in perm], bases)      # permuted
    assert [rec[perm.index(i)] for i in range(len(base))] == rec0
    mixed, at = [], []                                                          # other neighbours, on other committees
    for b in base:
        for _ in range(rng.randrange(3)):
            mixed.append(sets[rng.randrange(100, 300)])
        at.append(len(mixed))
        mixed.append(b)
    rec, st, _ = run_bits(m, cache, drawn, mixed, bases)
    assert [rec[p] for p in at] == rec0 and all(st[p] == 0 for p in at)
    for i in (0, 7, 19, len(base) - 1):                                         # alone
        rec, st, routes = run_bits(m, cache, drawn, [base[i]], bases)
        assert (rec, st) == ([rec0[i]], bytes(1)) and routes == (1 - base[i]["route"], base[i]["route"])


def test_argument_errors(m, cache, drawn):
    L = m.lib()
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    pool = drawn["table"][:96 * 12]
    offs, which = (sz * 3)(0, 9, 12), (u32 * 2)(1, 0)
    bits, msgs, sigs, aggs = b"\x05\xff\x01", bytes(64), bytes(384), bytes(192)
    rec, st = ctypes.create_string_buffer(640), ctypes.create_string_buffer(b"\x07\x07", 2)

    def call(**kw):
        a = dict(ctx=cache._h, keys=pool, n_table=12, idx=None, c_offsets=offs, m=2, aggs=None, stride=96, which=which, bits=bits, k=2, msgs=msgs, sigs=sigs,
                 rec=rec, st=st)
        a.update(kw)
        return L.mi355_bls_aggregate_sets_bits(*a.values())
    assert call() == 1 and st.raw == bytes(2)
    assert call(c_offsets=(sz * 3)(0, 9, 8)) == ERR_ARG                          # decreasing
    assert call(c_offsets=(sz * 3)(0, 9, 13)) == ERR_ARG                         # past the table, no indices
    assert call(which=(u32 * 2)(1, 2)) == ERR_ARG                                # a committee that is not there
    assert call(aggs=aggs, stride=95) == ERR_ARG and call(aggs=aggs, stride=98) == ERR_ARG and call(aggs=aggs, stride=0) == ERR_ARG
    assert call(aggs=aggs, stride=96) == 1                                       # all-zero bases: every set summed directly
    assert m.debug_aggregate_bits_routes(cache) == (2, 0)
    for hole in ("ctx", "keys", "c_offsets", "which", "bits", "msgs", "sigs", "rec", "st"):
        assert call(**{hole: None}) == ERR_ARG, hole
    st2 = ctypes.create_string_buffer(b"\x07\x07", 2)
    assert call(k=0, st=st2) == 0 and st2.raw == b"\x07\x07"                     # k = 0: 0, nothing written
    out = ctypes.create_string_buffer(2)
    head = (cache._h, pool, 12, None, offs, 2, None, 96)
    assert L.mi355_bls_fast_aggregate_verify_each_bits(*head, (u32 * 2)(1, 2), bits, 2, msgs, sigs, out) == ERR_ARG
    assert L.mi355_bls_fast_aggregate_verify_each_bits(*head, which, bits, 0, msgs, sigs, out) == 0
    assert L.mi355_bls_fast_aggregate_verify_each_bits(*head, which, bits, 2, msgs, sigs, None) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify_bits(*head, (u32 * 2)(2, 0), bits, 2, msgs, sigs, bytes(32)) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify_bits(*head, which, bits, 2, msgs, sigs, None) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify_bits(*head, which, bits, 0, msgs, sigs, bytes(32)) == 0
    dhead = (cache._h, None, 12, None, offs, 2, None, 96, which, None, 2, None, None)
    assert L.mi355_bls_aggregate_sets_bits_device(*dhead, None, st, None) == ERR_ARG                                     # null device pointers
    assert L.mi355_bls_fast_aggregate_verify_each_bits_device(*dhead, out, None) == ERR_ARG
    assert L.mi355_bls_batch_fast_aggregate_verify_bits_device(*dhead, bytes(32), None) == ERR_ARG


def test_destroy_returns_the_new_buffers(m, drawn):
    L = m.lib()
    L.mi355_bls_default_ctx_release()
    before = L.mi355_bls_debug_live_resources()
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        built = L.mi355_bls_debug_live_resources()
        sets = drawn["sets"][:20]
        rec, st, _ = run_bits(m, c, drawn, sets)
        assert [r[:96] for r in rec] == [d["agg"] for d in sets]
        assert L.mi355_bls_debug_live_resources() > built                      # the mode bytes among them
    finally:
        c.close()
    assert L.mi355_bls_debug_live_resources() == before
