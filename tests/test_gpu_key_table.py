"""GPU: the key table from the wire.  mi355_bls_deserialize_public_keys (k_deser_pks) on the adversarial key encodings of
tests/golden/deser_adversarial.json, hostile and valid lanes side by side, against the big-integer oracle and against the tuple decoder;
mi355_bls_admit_keys (both decoders, the survivor gather k_admit_records, the blinded batch check with locate over the survivors only, the
status merge and k_admit_zero_rows) against tests/golden/key_table.json in every wire form, through the host and the _device forms; the
route (a row that does not decode never sends the others to the per-pair pass); a small context; the edges."""
import ctypes
import hashlib

import pytest

import deser_cases as dc
import key_table_cases as kc

pytestmark = pytest.mark.gpu

N_VALID = 64
RND = (hashlib.sha256(b"key table rnd 0").digest(), hashlib.sha256(b"key table rnd 1").digest())


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=256, numThreads=4)
    yield c
    c.close()


def dev(b):
    import numpy as np
    import torch
    t = torch.from_numpy(np.frombuffer(b if b else b"\0", dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_out(nbytes, fill=0xee):
    import torch
    t = torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t, nbytes):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())[:nbytes]


@pytest.fixture(scope="module")
def key_batches():
    """per wire form: the adversarial key encodings with 64 valid keys spread between them, and the oracle's status and image of every row
    for KNOWN_ON_CURVE off and on - computed once, never modified"""
    import c_oracle as co
    rec = co.make_batch(N_VALID, seed=4243)
    pk48 = co.compress_sets(rec)[0]
    pk96 = co.serialize_sets(rec)[0]
    out = {}
    for unc in (False, True):
        kb, ks = (96 if unc else 48), (pk96 if unc else pk48)
        rows = kc.key_layout(unc, [ks[kb * i:kb * i + kb] for i in range(N_VALID)])
        n = len(rows)
        assert n % 64 and n > 64                                                  # more than one wave, the last one partial
        kinds = [nm is None for nm, _ in rows]
        assert sum(1 for a, b in zip(kinds[:64], kinds[1:64]) if a != b) >= 16     # hostile and valid lanes next to each other
        b = {"names": [nm for nm, _ in rows], "pk": b"".join(k for _, k in rows), "n": n}
        for known in (False, True):
            want = [kc.oracle_key(k, unc, known) for _, k in rows]
            b["st", known], b["img", known] = bytes(w[0] for w in want), b"".join(w[1] for w in want)
        assert set(b["st", False]) == {0, 1, 2, 3} and set(b["st", True]) == {0, 1, 3}
        out[unc] = b
    return out


@pytest.mark.parametrize("unc", (False, True))
@pytest.mark.parametrize("known", (False, True))
def test_decoder_against_the_oracle(m, cache, key_batches, unc, known):
    b = key_batches[unc]
    n = b["n"]
    ok, out, st = m.deserializePublicKeys(cache, b["pk"], pk_uncompressed=unc, known_on_curve=known)
    bad = [(k, b["names"][k], st[k], b["st", known][k]) for k in range(n) if st[k] != b["st", known][k]]
    assert not bad, bad
    for k in range(n):
        assert out[96 * k:96 * k + 96] == b["img", known][96 * k:96 * k + 96], (k, b["names"][k])
    assert ok is False
    d_pk, d_out = dev(b["pk"]), dev_out(96 * n + 4)
    ok_d, st_d = m.deserializePublicKeys_device(cache, d_pk.data_ptr(), n, d_out.data_ptr(), pk_uncompressed=unc, known_on_curve=known)
    got = host(d_out, 96 * n + 4)
    assert (ok_d, st_d, got[:96 * n]) == (False, st, out) and got[96 * n:] == b"\xee" * 4       # nothing written behind the table
    if known:                                                                     # the points outside G1 decode to their images, status 0
        off = [k for k in range(n) if b["st", False][k] == 2]
        assert len(off) >= 20 and all(st[k] == 0 and out[96 * k:96 * k + 96] != bytes(96) for k in off)
    # the valid keys alone: every status 0, the call returns 1; status and output may be left out
    valid = [k for k in range(n) if b["names"][k] is None]
    kb = 96 if unc else 48
    pk = b"".join(b["pk"][kb * k:kb * k + kb] for k in valid)
    assert m.deserializePublicKeys(cache, pk, pk_uncompressed=unc, known_on_curve=known) == (True, b"".join(out[96 * k:96 * k + 96] for k in valid), bytes(len(valid)))
    flags = (dc.PK_UNCOMPRESSED if unc else 0) | (dc.KNOWN_ON_CURVE if known else 0)
    L = m.lib()
    assert L.mi355_bls_deserialize_public_keys(cache._h, pk, len(valid), flags, None, None) == 1
    assert L.mi355_bls_deserialize_public_keys(cache._h, b["pk"], n, flags, None, None) == 0
    assert L.mi355_bls_deserialize_public_keys(cache._h, pk, len(valid), flags | dc.SIG_UNCOMPRESSED, None, None) < 0


@pytest.mark.parametrize("unc", (False, True))
def test_decoder_agrees_with_the_tuple_decoder(m, cache, key_batches, unc):
    import c_oracle as co
    b = key_batches[unc]
    n = b["n"]
    sig96 = co.compress_sets(co.make_batch(1, seed=12))[2]
    for known in (False, True):
        _, rec, st_t = m.deserializeSetsEx(cache, b["pk"], bytes(32 * n), sig96 * n, pk_uncompressed=unc, known_on_curve=known)
        _, out, st = m.deserializePublicKeys(cache, b["pk"], pk_uncompressed=unc, known_on_curve=known)
        assert st == st_t
        assert out == b"".join(rec[320 * k:320 * k + 96] for k in range(n))


@pytest.mark.parametrize("pku,sgu", dc.COMBOS)
def test_admission_against_the_fixture(m, cache, pku, sgu):
    kinds, pk, pr, status, table = kc.admit_inputs(pku, sgu)
    n = len(kinds)
    assert n >= 60 and set(status) == {0, 1, 2, 3, 4, 5, 8}
    d_pk, d_pr = dev(pk), dev(pr)
    for rnd in RND:                                                               # the statuses do not depend on the random bytes
        ok, out, st = m.admitKeys(cache, pk, pr, rnd, pk_uncompressed=pku, sig_uncompressed=sgu)
        bad = [(k, kinds[k], st[k], status[k]) for k in range(n) if st[k] != status[k]]
        assert not bad, bad
        for k in range(n):
            assert out[96 * k:96 * k + 96] == table[96 * k:96 * k + 96], (k, kinds[k])
        assert ok is False
        d_out = dev_out(96 * n + 4)
        ok_d, st_d = m.admitKeys_device(cache, d_pk.data_ptr(), d_pr.data_ptr(), n, rnd, d_out.data_ptr(), pk_uncompressed=pku, sig_uncompressed=sgu)
        got = host(d_out, 96 * n + 4)
        assert (ok_d, st_d, got[:96 * n]) == (False, status, table) and got[96 * n:] == b"\xee" * 4
    # the admitted rows alone are a table the call returns 1 for
    good = [k for k in range(n) if status[k] == 0]
    kb, pb = (96 if pku else 48), (192 if sgu else 96)
    gk, gp = b"".join(pk[kb * k:kb * k + kb] for k in good), b"".join(pr[pb * k:pb * k + pb] for k in good)
    assert m.admitKeys(cache, gk, gp, RND[0], pk_uncompressed=pku, sig_uncompressed=sgu) == (True, b"".join(table[96 * k:96 * k + 96] for k in good), bytes(len(good)))


def seeded_sks(n, tag=b"key table sk"):
    return [hashlib.sha256(tag + b" %d" % i).digest()[:31] + b"\x00" for i in range(n)]


@pytest.fixture(scope="module")
def proved(m, cache):
    """160 valid (key, proof) pairs from the device prover with their wire forms (deterministic keys): computed once, never modified"""
    n = 160
    ok, pks, proofs, st = m.popProve(cache, b"".join(seeded_sks(n)))
    assert ok and st == bytes(n)
    return {"n": n, "pk96": [pks[96 * i:96 * i + 96] for i in range(n)], "pk48": m.compressPublicKeys(cache, pks), "pr96": m.compressSignatures(cache, proofs)}


UNDECODABLE = (bytes(48), b"\xc0" + bytes(46) + b"\x01", b"\x9f" + b"\xff" * 47, b"\xe0" + bytes(47))      # no compressed bit | infinity with a payload | x >= p | infinity with the sign bit


def test_route_undecodable_rows_do_not_cost_the_per_pair_pass(m, cache, proved):
    n = 100
    pk, pr = list(proved["pk48"][:n]), list(proved["pr96"][:n])
    broken = [0, 17, 63, 64, 99]
    for j, i in enumerate(broken):
        pk[i] = UNDECODABLE[j % len(UNDECODABLE)]
    before = m.verifyEachPasses(cache)
    ok, out, st = m.admitKeys(cache, pk, pr, RND[0])
    assert ok is False and [i for i in range(n) if st[i]] == broken and all(st[i] == 1 for i in broken)
    assert out == b"".join(bytes(96) if i in broken else proved["pk96"][i] for i in range(n))
    assert m.verifyEachPasses(cache) == before                                    # the survivors passed as a batch: no per-pair pass
    # one survivor's proof is another key's: that row alone is refused, by exactly one per-pair pass
    pr[40] = proved["pr96"][41]
    ok, out, st = m.admitKeys(cache, pk, pr, RND[0])
    assert ok is False and [i for i in range(n) if st[i]] == sorted(broken + [40]) and st[40] == m.KEY_BAD_PROOF == 8
    assert out == b"".join(bytes(96) if i in broken + [40] else proved["pk96"][i] for i in range(n))
    assert m.verifyEachPasses(cache) == before + 1
    # the same through the device form: the refused row is zeroed in the caller's table
    d_pk, d_pr, d_out = dev(b"".join(pk)), dev(b"".join(pr)), dev_out(96 * n)
    assert m.admitKeys_device(cache, d_pk.data_ptr(), d_pr.data_ptr(), n, RND[1], d_out.data_ptr()) == (False, st)
    assert host(d_out, 96 * n) == out
    assert m.verifyEachPasses(cache) == before + 2


def test_small_capacity_and_the_table_feeds_aggregate_sets(m, cache, proved):
    import numpy as np
    n = 150
    pk, pr = list(proved["pk48"][:n]), list(proved["pr96"][:n])
    pk[5], pk[64] = UNDECODABLE[0], UNDECODABLE[2]
    pr[70] = proved["pr96"][71]
    pr[149] = b"\xc0" + bytes(95)                                                 # the infinity proof
    refused = {5: 1, 64: 1, 70: 8, 149: 8}
    want_st = bytes(refused.get(i, 0) for i in range(n))
    want_table = b"".join(bytes(96) if i in refused else proved["pk96"][i] for i in range(n))
    small = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        big = m.admitKeys(cache, pk, pr, RND[0])
        assert big == (False, want_table, want_st)
        assert m.admitKeys(small, pk, pr, RND[0]) == big and m.admitKeys(small, pk, pr, RND[1]) == big
        d_pk, d_pr, d_tab = dev(b"".join(pk)), dev(b"".join(pr)), dev_out(96 * n)
        assert m.admitKeys_device(small, d_pk.data_ptr(), d_pr.data_ptr(), n, RND[0], d_tab.data_ptr()) == (False, want_st)
        assert host(d_tab, 96 * n) == want_table
        # the device table as it stands is aggregateSets' key table: the same records as with the images popProve returned
        lists = [[0, 1, 2], [149 - 1, 3, 63, 65, 66], list(range(6, 60)), [100], [7, 7, 8]]
        assert not any(i in refused for lst in lists for i in lst)
        idx = [i for lst in lists for i in lst]
        offsets = [0]
        for lst in lists:
            offsets.append(offsets[-1] + len(lst))
        k = len(lists)
        msgs = b"".join(hashlib.sha256(b"key table msg %d" % g).digest() for g in range(k))
        sigs = b"".join(proved["pk96"][g] * 2 for g in range(k))                  # any 192 bytes: aggregateSets copies them into the records
        want = m.aggregateSets(small, (b"".join(proved["pk96"][:n]), idx, offsets), msgs, sigs)
        assert want[0] is True and want[2] == bytes(k)
        d_idx, d_ms, d_sg, d_rec = dev(np.asarray(idx, dtype=np.uint32).tobytes()), dev(msgs), dev(sigs), dev_out(320 * k)
        ok, st = m.aggregateSets_device(small, d_tab.data_ptr(), n, d_idx.data_ptr(), offsets, d_ms.data_ptr(), d_sg.data_ptr(), d_rec.data_ptr())
        assert (ok, host(d_rec, 320 * k), st) == want
    finally:
        small.close()


def test_edges(m, cache, proved):
    L = m.lib()
    # n == 0: 1, nothing written
    d_out = dev_out(96)
    st = ctypes.create_string_buffer(b"\xee" * 4, 4)
    assert L.mi355_bls_admit_keys_device(cache._h, None, None, 0, 0, RND[0], d_out.data_ptr(), st, None) == 1
    assert L.mi355_bls_admit_keys(cache._h, None, None, 0, 0, RND[0], None, st) == 1
    assert L.mi355_bls_deserialize_public_keys_device(cache._h, None, 0, 0, d_out.data_ptr(), st, None) == 1
    assert host(d_out, 96) == b"\xee" * 96 and st.raw == b"\xee" * 4
    # refused arguments
    pk, pr = proved["pk48"][0], proved["pr96"][0]
    out = ctypes.create_string_buffer(96)
    assert L.mi355_bls_admit_keys(cache._h, pk, pr, 1, dc.KNOWN_ON_CURVE, RND[0], out, st) < 0      # admission is the full check
    assert L.mi355_bls_admit_keys(cache._h, pk, pr, 1, 0, None, out, st) < 0
    assert L.mi355_bls_admit_keys(cache._h, pk, pr, 1, 0, RND[0], out, None) < 0
    assert L.mi355_bls_admit_keys(cache._h, pk, pr, 1, 8, RND[0], out, st) < 0
    assert st.raw == b"\xee" * 4
    # no survivors: every status non-zero, an all-zero table, no pairing work (no per-pair pass either)
    before = m.verifyEachPasses(cache)
    n = 70
    pks = [UNDECODABLE[i % 4] for i in range(n)]
    prs = list(proved["pr96"][:n])
    for i in range(0, n, 2):
        pks[i] = proved["pk48"][i]
        prs[i] = b"\x9f" + b"\xff" * 95 if i % 4 else b"\xc0" + bytes(94) + b"\x01"  # x.c1 >= p | infinity with a payload
    ok, table, stt = m.admitKeys(cache, pks, prs, RND[0])
    assert ok is False and table == bytes(96 * n) and stt == bytes(4 if i % 2 == 0 else 1 for i in range(n))
    assert m.verifyEachPasses(cache) == before
    # n = 1 and n = 65, valid, then with the last row refused
    for n in (1, 65):
        pks, prs = list(proved["pk48"][:n]), list(proved["pr96"][:n])
        assert m.admitKeys(cache, pks, prs, RND[0]) == (True, b"".join(proved["pk96"][:n]), bytes(n))
        assert m.deserializePublicKeys(cache, pks) == (True, b"".join(proved["pk96"][:n]), bytes(n))
        prs[n - 1] = proved["pr96"][n]
        assert m.admitKeys(cache, pks, prs, RND[1]) == (False, b"".join(proved["pk96"][:n - 1]) + bytes(96), bytes(n - 1) + b"\x08")
        pks[n - 1] = UNDECODABLE[1]
        assert m.admitKeys(cache, pks, prs, RND[1]) == (False, b"".join(proved["pk96"][:n - 1]) + bytes(96), bytes(n - 1) + b"\x01")
