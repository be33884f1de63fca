"""Threshold-signature recovery on the device (mi355_bls_recover_signature_sets): recover(signs, ids) of blst_recovery.nim:150-156 for every
group in one pass.  Images, wire forms and status bytes are held bit-exact to tests/golden/recover_signatures.json (the reference's
tests/secret_sharing.nim cases, the edge groups, the level edges of the sum and the chosen coefficients that drive the windowed
multiplication), in both context modes, in the host and the device form, contiguous and indexed; shares signed on the device recover to
signatures that verify; a call that crosses the plan's chunk boundary gives what the unchunked call gives.  The CPU half is
tests/test_recover_emu.py."""
import hashlib
import random

import pytest

import recover_cases as rc

pytestmark = pytest.mark.gpu

R = rc.R


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=2048, numThreads=4)
    yield c
    c.close()


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def test_fixture_bit_exact_in_both_modes_and_forms(m):
    import torch
    fx = rc.fixture()
    tab = rc.table_of(fx)
    sigs, ids, offsets, w192, w96, status = rc.contiguous_inputs(fx)
    lists = [b"".join(tab[i] for i in g["members"]) for g in fx["groups"]]
    idl = [[bytes.fromhex(x) for x in g["ids"]] for g in fx["groups"]]
    good = [i for i, g in enumerate(fx["groups"]) if g["status"] == 0]
    k = len(lists)
    assert {0, 1, 2, 6, 7} == set(status)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            assert m.recoverSignatureSets(c, lists, idl) == (False, w192, w96, status), coop
            assert m.recoverSignatureSets(c, (sigs, None, offsets), ids) == (False, w192, w96, status), coop
            assert m.recoverSignatureSets(c, lists, idl, want96=False) == (False, w192, None, status), coop          # either output pointer NULL
            assert m.recoverSignatureSets(c, lists, idl, want192=False) == (False, None, w96, status), coop
            for bad in (False, True):
                table, idx, iids, ioffs, i192, i96, ist = rc.indexed_inputs(bad, fx)
                assert m.recoverSignatureSets(c, (table, idx, ioffs), iids) == (False, i192, i96, ist), (coop, bad)
                assert (3 in ist) == bad
            g192, g96 = b"".join(w192[192 * i:192 * i + 192] for i in good), b"".join(w96[96 * i:96 * i + 96] for i in good)
            assert m.recoverSignatureSets(c, [lists[i] for i in good], [idl[i] for i in good]) == (True, g192, g96, bytes(len(good))), coop
            # the device forms: everything resident, offsets on the host
            d_s, d_ids = dev(sigs), dev(ids)
            for want192, want96 in ((True, True), (True, False), (False, True)):
                o192 = torch.full((192 * k,), 0x5a, dtype=torch.uint8, device="cuda")
                o96 = torch.full((96 * k,), 0x5a, dtype=torch.uint8, device="cuda")
                ok, st = m.recoverSignatureSets_device(c, d_s.data_ptr(), len(sigs) // 192, None, offsets, d_ids.data_ptr(), o192.data_ptr() if want192 else None,
                                                       o96.data_ptr() if want96 else None)
                assert (ok, st) == (False, status)
                assert host(o192) == (w192 if want192 else b"\x5a" * (192 * k)) and host(o96) == (w96 if want96 else b"\x5a" * (96 * k)), (coop, want192, want96)
            table, idx, iids, ioffs, i192, i96, ist = rc.indexed_inputs(True, fx)
            d_t, d_i, d_ii = dev(table), torch.tensor(idx, dtype=torch.int64).to(torch.int32).cuda(), dev(iids)
            o192, o96 = torch.zeros(192 * k, dtype=torch.uint8, device="cuda"), torch.zeros(96 * k, dtype=torch.uint8, device="cuda")
            ok, st = m.recoverSignatureSets_device(c, d_t.data_ptr(), len(table) // 192, d_i.data_ptr(), ioffs, d_ii.data_ptr(), o192.data_ptr(), o96.data_ptr())
            assert (ok, st, host(o192), host(o96)) == (False, ist, i192, i96), coop
    finally:
        c.close()


def test_chosen_coefficients_by_scalar(m, cache):
    """the groups whose first coefficient is a chosen scalar, one call per group: a windowing failure is named by its scalar"""
    fx = rc.fixture()
    chosen = [g for g in fx["groups"] if g["kind"].startswith("coeff_")]
    assert len(chosen) >= 12
    tab = rc.table_of(fx)
    failed = []
    for g in chosen:
        got = m.recoverSignatureSets(cache, [b"".join(tab[i] for i in g["members"])], [[bytes.fromhex(x) for x in g["ids"]]])
        if got != (True, bytes.fromhex(g["out192"]), bytes.fromhex(g["out96"]), b"\x00"):
            failed.append((g["kind"], g["coeff"]))
    assert failed == []


def le(x):
    return x.to_bytes(32, "little")


@pytest.fixture(scope="module")
def shares300(m, cache):
    """300 validators, each split 3-of-3 by a random polynomial over Fr (host side, Python integers); the device signs every share and,
    for comparison, every whole key.  -> (share signatures [900 x 192 B], ids [900 x 32 B], keys [300 x 96 B], messages, whole-key signatures);
    computed once, never changed"""
    rng = random.Random(20261019)
    share_sks, ids, master_sks, msgs = [], [], [], []
    for g in range(300):
        cfs = [rng.randrange(1, R) for _ in range(3)]
        xs = [rng.getrandbits(255) for _ in range(3)]
        assert len({x % R for x in xs}) == 3 and all(x % R for x in xs)
        for x in xs:
            y = 0
            for cf in reversed(cfs):
                y = (y * x + cf) % R
            assert y
            share_sks.append(le(y))
            ids.append(le(x))
        master_sks.append(le(cfs[0]))
        msgs.append(hashlib.sha256(b"duty %d" % g).digest())
    ok, recs, _ = m.signSets(cache, b"".join(share_sks + master_sks), b"".join([msgs[g] for g in range(300) for _ in range(3)] + msgs))
    assert ok
    rec = lambda i: recs[320 * i:320 * i + 320]          # noqa: E731
    return ([rec(i)[128:] for i in range(900)], ids, [rec(900 + g)[:96] for g in range(300)], msgs, [rec(900 + g)[128:] for g in range(300)])


def test_device_signed_shares_recover_and_verify(m, cache, shares300):
    sigs, ids, pks, msgs, whole = shares300
    offs = list(range(0, 901, 3))                                     # 900 members: 15 waves, the last one partial
    ok, o192, o96, st = m.recoverSignatureSets(cache, (b"".join(sigs), None, offs), b"".join(ids))
    assert (ok, st) == (True, bytes(300))
    assert o192 == b"".join(whole)                                     # the whole key's own signature, bit for bit
    assert m.compressSignatures(cache, o192) == [o96[96 * g:96 * g + 96] for g in range(300)]
    recs = b"".join(pks[g] + msgs[g] + o192[192 * g:192 * g + 192] for g in range(300))
    assert m.verifyEach(cache, recs) == [True] * 300
    s = list(sigs)
    s[3 * 7 + 1] = sigs[3 * 8 + 1]                                     # one share of group 7 is another group's
    ok, t192, _, st = m.recoverSignatureSets(cache, (b"".join(s), None, offs), b"".join(ids), want96=False)
    assert (ok, st) == (True, bytes(300))                              # a wrong share is not an error: it recovers another point
    recs = b"".join(pks[g] + msgs[g] + t192[192 * g:192 * g + 192] for g in range(300))
    assert m.verifyEach(cache, recs) == [g != 7 for g in range(300)]


def test_call_across_the_chunk_boundary(m, cache, shares300):
    """21 900 groups of 3 (65 700 members, past the plan's 65 536-member chunk: the second chunk starts at group 21 845) through an index
    array into the 900 shares: every group's output is what the unchunked 300-group call gives for it"""
    sigs, ids, _, _, whole = shares300
    reps = 73
    idx = list(range(900)) * reps
    offs = list(range(0, 900 * reps + 1, 3))
    ok, o192, o96, st = m.recoverSignatureSets(cache, (b"".join(sigs), idx, offs), b"".join(ids) * reps, want96=False)
    assert (ok, st) == (True, bytes(300 * reps)) and o96 is None
    assert o192 == b"".join(whole) * reps
