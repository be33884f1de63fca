"""The host and the device form of the six grouped calls that have both (aggregate_sets, aggregate_sets_bits, combine_sets,
aggregate_signature_sets, recover_signature_sets, aggregate_verify_each) on the groups the host staging's guards exist for: k = 3 groups of
0, 1 and 9 members (AGG_C = 8: nine is the shortest group with two levels), addressed directly and through an index array that permutes
the table.  The host form's outputs and status bytes equal the device form's byte for byte; the device form's equal what each feature's own
test holds it to (the C restatement's g1_sum / combine / aggregate_verify, the golden groups of aggregate_signatures.json and
recover_signatures.json); an empty group's status is 1 (no member) and its verdict False.  A second call with more groups on the same
context follows every first one, so the workspace grows between calls."""
import hashlib
import random

import pytest

import aggsigs_cases as ac
import recover_cases as rc

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 9)
OFFS = [0, 0, 1, 10]
N = 10                              # positions of the three groups
BIG = 12                            # groups of the second call


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    yield c
    c.close()


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def dev_idx(idx):
    import torch
    return torch.tensor(idx, dtype=torch.int64).to(torch.int32).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device="cuda")


def permuted(rows, seed):
    """rows (a list of equal-sized byte strings) -> (the table with the rows in another order, idx with table[idx[i]] == rows[i])"""
    order = list(range(len(rows)))
    random.Random(seed).shuffle(order)
    idx = [0] * len(rows)
    for at, i in enumerate(order):
        idx[i] = at
    assert idx != list(range(len(rows)))
    return b"".join(rows[i] for i in order), idx


def offsets_of(lengths):
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + n)
    return offs


@pytest.fixture(scope="module")
def keyed():
    """96 keys and 12 valid records from the C restatement: computed once, never changed."""
    import c_oracle as co
    table, _ = co.make_pks(96, seed=7700)
    keys = [table[96 * i:96 * i + 96] for i in range(96)]
    rec = co.make_batch(BIG, seed=7800)
    recs = [rec[320 * i:320 * i + 320] for i in range(BIG)]
    return keys, recs


def addressings(rows, lengths, seed):
    """the two ways to address sum(lengths) rows: (table bytes, idx or None, offsets)"""
    n = sum(lengths)
    offs = offsets_of(lengths)
    table, idx = permuted(rows[:n], seed)
    return ((b"".join(rows[:n]), None, offs), (table, idx, offs))


BIG_LENGTHS = [3, 0, 1, 9, 2, 17, 1, 8, 5, 0, 4, 7]      # the second call: more groups, more members, more levels


def test_aggregate_sets(m, cache, keyed):
    import c_oracle as co
    keys, recs = keyed
    for lengths in (LENGTHS, BIG_LENGTHS):
        k = len(lengths)
        msgs, sigs = b"".join(r[96:128] for r in recs[:k]), b"".join(r[128:] for r in recs[:k])
        for table, idx, offs in addressings(keys, lengths, 11):
            ok_h, rec_h, st_h = m.aggregateSets(cache, (table, idx, offs), msgs, sigs)
            out = zeros(320 * k)
            d_t, d_i, d_m, d_s = dev(table), (dev_idx(idx) if idx else None), dev(msgs), dev(sigs)
            ok_d, st_d = m.aggregateSets_device(cache, d_t.data_ptr(), len(table) // 96, d_i.data_ptr() if idx else None, offs, d_m.data_ptr(), d_s.data_ptr(),
                                                out.data_ptr())
            rec_d = host(out)
            assert (ok_h, rec_h, st_h) == (ok_d, rec_d, st_d), (lengths, idx is not None)
            assert st_d == bytes(0 if n else 1 for n in lengths) and ok_d is False
            for g, n in enumerate(lengths):
                if n:
                    assert rec_d[320 * g:320 * g + 320] == co.g1_sum(b"".join(keys[offs[g]:offs[g + 1]])) + recs[g][96:], (lengths, g)


def bit_fields(lengths, committee_len):
    """the members of set s are the first lengths[s] positions of its committee"""
    return [bytes(sum(1 << b for b in range(8) if 8 * i + b < n) for i in range((committee_len + 7) // 8)) for n in lengths]


def test_aggregate_sets_bits(m, cache, keyed):
    """two committees; set s picks a prefix of committee s % 2 by its bits.  Without committee aggregates, then with them 320 bytes apart
    (the host form packs them with a pitched copy): a set of more than half of its committee is then the aggregate less the absentees."""
    import c_oracle as co
    keys, recs = keyed
    for lengths, clen in ((LENGTHS, 9), (BIG_LENGTHS, 17)):
        k = len(lengths)
        msgs, sigs = b"".join(r[96:128] for r in recs[:k]), b"".join(r[128:] for r in recs[:k])
        which, bits = [s % 2 for s in range(k)], bit_fields(lengths, clen)
        members = [keys[clen * which[s]:clen * which[s] + n] for s, n in enumerate(lengths)]
        aggs = b"".join(co.g1_sum(b"".join(keys[clen * c:clen * c + clen])) + b"\xa5" * 224 for c in range(2))
        for table, idx, offs in addressings(keys, (clen, clen), 12):
            for bases, stride in ((None, 96), (aggs, 320)):
                ok_h, rec_h, st_h = m.aggregateSetsBits(cache, (table, idx, offs), which, bits, msgs, sigs, bases, stride)
                routes_h = tuple(m.debug_aggregate_bits_routes(cache))
                out = zeros(320 * k)
                d_t, d_i, d_b, d_m, d_s = dev(table), (dev_idx(idx) if idx else None), dev(b"".join(bits)), dev(msgs), dev(sigs)
                d_a = dev(bases) if bases else None
                ok_d, st_d = m.aggregateSetsBits_device(cache, d_t.data_ptr(), len(table) // 96, d_i.data_ptr() if idx else None, offs,
                                                        d_a.data_ptr() if bases else None, stride, which, d_b.data_ptr(), d_m.data_ptr(), d_s.data_ptr(),
                                                        out.data_ptr())
                rec_d = host(out)
                assert (ok_h, rec_h, st_h, routes_h) == (ok_d, rec_d, st_d, tuple(m.debug_aggregate_bits_routes(cache))), (lengths, idx is not None, stride)
                assert st_d == bytes(0 if n else 1 for n in lengths)
                assert (routes_h[1] > 0) == (bases is not None), (lengths, stride)          # by exclusion only where a base is given
                for g, n in enumerate(lengths):
                    if n:
                        assert rec_d[320 * g:320 * g + 320] == co.g1_sum(b"".join(members[g])) + recs[g][96:], (lengths, g, stride)


def test_combine_sets(m, cache):
    import c_oracle as co
    for lengths in (LENGTHS, BIG_LENGTHS):
        k, n = len(lengths), sum(lengths)
        offs = offsets_of(lengths)
        rows = []
        for g, ln in enumerate(lengths):                                 # one message per group, a key of its own per member
            msg = hashlib.sha256(b"grouped host forms combine %d" % g).digest()
            for j in range(ln):
                sk = 7000 + 13 * (offs[g] + j)
                rows.append(co.sk_to_pk(sk) + msg + co.sign(sk, msg))
        rnds = [hashlib.sha256(b"grouped host forms rnd %d" % g).digest() for g in range(k)]
        table, idx = permuted(rows, 13)
        for sets, ix in ((b"".join(rows), None), (table, idx)):
            ok_h, rec_h, st_h = m.combineSets(cache, sets, ix, offs, rnds)
            out = zeros(320 * k)
            d_t, d_i = dev(sets), (dev_idx(ix) if ix else None)
            ok_d, st_d = m.combineSets_device(cache, d_t.data_ptr(), n, d_i.data_ptr() if ix else None, offs, rnds, out.data_ptr())
            rec_d = host(out)
            assert (ok_h, rec_h, st_h) == (ok_d, rec_d, st_d), (lengths, ix is not None)
            assert st_d == bytes(0 if ln else 1 for ln in lengths)
            for g, ln in enumerate(lengths):
                grp = rows[offs[g]:offs[g + 1]]
                if ln == 1:
                    assert rec_d[320 * g:320 * g + 320] == grp[0], (lengths, g)
                elif ln:
                    pk, sg, _ = co.combine(rnds[g], b"".join(r[:96] for r in grp), b"".join(r[128:] for r in grp))
                    assert rec_d[320 * g:320 * g + 320] == pk + grp[0][96:128] + sg, (lengths, g)


def golden_groups(fx, kinds):
    by_kind = {}
    for g in fx["groups"]:
        by_kind.setdefault(g["kind"], g)
    return [by_kind[kd] for kd in kinds]


def test_aggregate_signature_sets(m, cache):
    fx = ac.fixture()
    tab = ac.table_of(fx)
    for groups in (golden_groups(fx, ("empty", "len_1", "len_9")), fx["groups"]):
        lengths = [len(g["members"]) for g in groups]
        assert groups is fx["groups"] or tuple(lengths) == LENGTHS
        k, offs = len(groups), offsets_of(lengths)
        rows = [tab[i] for g in groups for i in g["members"]]
        w192, w96, status = (b"".join(bytes.fromhex(g["out192"]) for g in groups), b"".join(bytes.fromhex(g["out96"]) for g in groups),
                             bytes(g["status"] for g in groups))
        table, idx = permuted(rows, 14)
        for sigs, ix in ((b"".join(rows), None), (table, idx)):
            got_h = m.aggregateSignatureSets(cache, (sigs, ix, offs))
            o192, o96 = zeros(192 * k), zeros(96 * k)
            d_t, d_i = dev(sigs), (dev_idx(ix) if ix else None)
            ok_d, st_d = m.aggregateSignatureSets_device(cache, d_t.data_ptr(), len(rows), d_i.data_ptr() if ix else None, offs, o192.data_ptr(), o96.data_ptr())
            got_d = (ok_d, host(o192), host(o96), st_d)
            assert got_h == got_d, (k, ix is not None)
            assert got_d == (not any(status), w192, w96, status), (k, ix is not None)


def test_recover_signature_sets(m, cache):
    fx = rc.fixture()
    tab = rc.table_of(fx)
    for groups in (golden_groups(fx, ("edge_empty", "ref_1_of_1", "len_9")), fx["groups"]):
        lengths = [len(g["members"]) for g in groups]
        assert groups is fx["groups"] or tuple(lengths) == LENGTHS
        k, offs = len(groups), offsets_of(lengths)
        rows = [tab[i] for g in groups for i in g["members"]]
        ids = b"".join(bytes.fromhex(x) for g in groups for x in g["ids"])             # by position, never by index
        w192, w96, status = rc.expected(groups)
        table, idx = permuted(rows, 15)
        for sigs, ix in ((b"".join(rows), None), (table, idx)):
            got_h = m.recoverSignatureSets(cache, (sigs, ix, offs), ids)
            o192, o96 = zeros(192 * k), zeros(96 * k)
            d_t, d_i, d_ids = dev(sigs), (dev_idx(ix) if ix else None), dev(ids or b"\0")
            ok_d, st_d = m.recoverSignatureSets_device(cache, d_t.data_ptr(), len(rows), d_i.data_ptr() if ix else None, offs, d_ids.data_ptr(), o192.data_ptr(),
                                                       o96.data_ptr())
            got_d = (ok_d, host(o192), host(o96), st_d)
            assert got_h == got_d, (k, ix is not None)
            assert got_d == (not any(status), w192, w96, status), (k, ix is not None)


def test_aggregate_verify_each(m, cache):
    import c_oracle as co
    for lengths in (LENGTHS, BIG_LENGTHS):
        k, n = len(lengths), sum(lengths)
        offs = offsets_of(lengths)
        sks = [9000 + 17 * i for i in range(n)]
        keys = [co.sk_to_pk(s) for s in sks]
        msgs = [hashlib.sha256(b"grouped host forms aggv %d" % i).digest() for i in range(n)]
        sigs = []
        for g, ln in enumerate(lengths):
            parts = [co.sign(sks[i], msgs[i]) for i in range(offs[g], offs[g + 1])]
            sigs.append(co.g2_sum(b"".join(parts)) if ln else co.sign(5, b"nobody signed this"))
        if n > 1:
            sigs[lengths.index(max(lengths))] = sigs[lengths.index(1)]                  # one group under another group's signature
        want = [bool(ln) and co.aggregate_verify(keys[offs[g]:offs[g + 1]], msgs[offs[g]:offs[g + 1]], sigs[g]) for g, ln in enumerate(lengths)]
        assert True in want and want.count(False) >= 2
        table, idx = permuted(keys, 16)
        for tb, ix in ((b"".join(keys), None), (table, idx)):
            got_h = m.aggregateVerifyEach(cache, (tb, ix, offs), b"".join(msgs), b"".join(sigs))
            d_t, d_i, d_m, d_s = dev(tb), (dev_idx(ix) if ix else None), dev(b"".join(msgs)), dev(b"".join(sigs))
            got_d = m.aggregateVerifyEach_device(cache, d_t.data_ptr(), n, d_i.data_ptr() if ix else None, offs, d_m.data_ptr(), d_s.data_ptr())
            assert got_h == got_d == want, (lengths, ix is not None)
