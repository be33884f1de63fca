"""Proofs of possession on the device (mi355_bls_pop_verify_each, mi355_bls_batch_pop_verify, mi355_bls_batch_pop_verify_locate,
mi355_bls_compress_public_keys, mi355_bls_pop_prove): popVerify = coreVerifyNoGroupCheck(pk, compress(pk), proof, DST_POP)
(bls_sig_min_pubkey.nim:60-74) for a table of keys in one pass.  Verdicts and values are held bit-exact to tests/golden/pop.json, the hashed
points and the prover to the C restatement; a pair's verdict must not depend on its position, its neighbours, the slice it falls into or the
hash-map executor its size selects."""
import ctypes
import hashlib
import random

import pytest

pytestmark = pytest.mark.gpu

N_PROVED = 1800          # at least one more than the largest row-form size of any device this runs on is checked where it is used


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def S():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def rows_max_n(S):
    """the largest n whose hash-map stage takes the row form, from the plan itself (csrc/plan.hpp hash_map_for)"""
    import util
    n = 1
    while util.slice_plan(n + 1, S)["hash_map"] == 0:
        n += 1
    assert util.latency_plan(n, S)["hash_map"] == "rows" and util.latency_plan(n + 1, S)["hash_map"] == "spread"
    assert ("rows", "spread", "plain")[util.slice_plan(130, S, coop=False)["hash_map"]] == "plain"
    return n


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=4096, numThreads=64)
    yield c
    c.close()


def seeded_sks(n, tag=b"pop sk"):
    return [hashlib.sha256(tag + b" %d" % i).digest()[:31] + b"\x00" for i in range(n)]


@pytest.fixture(scope="module")
def proved(m, cache, rows_max_n):
    """valid (key, proof) pairs from the device prover (deterministic keys): every larger test cuts its inputs from these"""
    n = max(N_PROVED, rows_max_n + 1)
    ok, pks, proofs, st = m.popProve(cache, b"".join(seeded_sks(n)))
    assert ok and st == bytes(n)
    return [pks[96 * i:96 * i + 96] for i in range(n)], [proofs[192 * i:192 * i + 192] for i in range(n)]


def with_bad(pks, proofs, n):
    """the first n pairs with another key's proof at 0, an infinity proof at n / 2 and an infinity key at n - 1"""
    pks, proofs = list(pks[:n]), list(proofs[:n])
    proofs[0] = proofs[1]
    proofs[n // 2] = bytes(192)
    pks[n - 1] = bytes(96)
    return pks, proofs, [0, n // 2, n - 1]


def o_affine_g2(jac288):
    import bls12381_py as o
    from util import g2_jac_to_affine
    return o.g2_to_blst_affine(g2_jac_to_affine(jac288))


def compress(pk96):
    import bls12381_py as o
    return o.g1_compress(o.g1_from_blst_affine(pk96))


def fixture_arrays():
    from util import golden
    fx = golden("pop")
    return fx, b"".join(bytes.fromhex(c["pk"]) for c in fx["cases"]), b"".join(bytes.fromhex(c["proof"]) for c in fx["cases"])


def test_fixture_bit_exact_in_both_modes(m):
    fx, pks, proofs = fixture_arrays()
    cases = fx["cases"]
    n = len(cases)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            ok, gts = m.popVerifyEachValues(c, pks, proofs)
            assert ok == [bool(x["verdict"]) for x in cases], coop
            assert [g.hex() for g in gts] == [x["gt"] for x in cases], coop
            assert m.popVerifyEach(c, pks, proofs) == ok
            assert [b.hex() for b in m.compressPublicKeys(c, pks)] == [x["compressed"] for x in cases], coop
            out = ctypes.create_string_buffer(n)
            assert m.lib().mi355_bls_pop_verify_each(c._h, pks, proofs, n, out) == 0       # not every pair verified
            assert list(out.raw) == [x["verdict"] for x in cases]
            good = [i for i in range(n) if cases[i]["verdict"]]
            gk, gp = b"".join(pks[96 * i:96 * i + 96] for i in good), b"".join(proofs[192 * i:192 * i + 192] for i in good)
            assert m.lib().mi355_bls_pop_verify_each(c._h, gk, gp, len(good), out) == 1
            before = out.raw
            assert m.lib().mi355_bls_pop_verify_each(c._h, gk, gp, 0, out) == 0            # n = 0: 0, nothing written
            assert out.raw == before
    finally:
        c.close()


def test_reference_vectors_through_the_deserialiser(m):
    """tests/eth2_vectors.nim:33-47 decoded by the existing wire-format decoder (a proof is a Signature on the wire; the message column is unused)"""
    fx, _, _ = fixture_arrays()
    ref = [x for x in fx["cases"] if x["reference"]]
    assert len(ref) == 3
    import bls12381_py as o
    pk48 = b"".join(bytes.fromhex(x["compressed"]) for x in ref)
    pr96 = b"".join(o.g2_compress(o.g2_from_blst_affine(bytes.fromhex(x["proof"]))) for x in ref)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            ok, rec, st = m.deserializeSets(c, pk48, bytes(96), pr96)
            assert ok and st == bytes(3)
            pks = [rec[320 * i:320 * i + 96] for i in range(3)]
            proofs = [rec[320 * i + 128:320 * i + 320] for i in range(3)]
            assert pks == [bytes.fromhex(x["pk"]) for x in ref] and proofs == [bytes.fromhex(x["proof"]) for x in ref]
            assert m.popVerifyEach(c, pks, proofs) == [True, True, True]
            assert m.popVerifyEach(c, pks[1:] + pks[:1], proofs) == [False, False, False]
    finally:
        c.close()


def test_prover_reproduces_the_reference_vectors(m, cache):
    import bls12381_py as o
    fx, _, _ = fixture_arrays()
    ref = [x for x in fx["cases"] if x["reference"]]
    sks = b"".join(int(x["sk"], 16).to_bytes(32, "little") for x in ref)
    ok, pks, proofs, st = m.popProve(cache, sks)
    assert ok and st == bytes(3)
    for i, x in enumerate(ref):
        assert o.g1_compress(o.g1_from_blst_affine(pks[96 * i:96 * i + 96])).hex() == x["compressed"]
        assert proofs[192 * i:192 * i + 192].hex() == x["proof"]
        assert o.g2_compress(o.g2_from_blst_affine(proofs[192 * i:192 * i + 192])) == o.g2_compress(o.pop_prove(int(x["sk"], 16)))


def test_prover_equals_c_oracle_and_refuses_bad_scalars(m, cache):
    import bls12381_py as o
    import c_oracle as co
    sks = seeded_sks(32, b"pop prover")
    ok, pks, proofs, st = m.popProve(cache, sks)
    assert ok and st == bytes(32)
    for i, sk in enumerate(sks):
        k = int.from_bytes(sk, "little")
        pk = pks[96 * i:96 * i + 96]
        assert pk == co.sk_to_pk(k)
        assert proofs[192 * i:192 * i + 192] == co.g2_mul(co.hash_to_g2(compress(pk), o.DST_POP), k), i
    bad = [sks[0], bytes(32), o.R.to_bytes(32, "little"), sks[1]]                       # sk == 0, sk == r
    ok, pks2, proofs2, st = m.popProve(cache, bad)
    assert ok is False and st == bytes([0, 1, 1, 0])
    assert pks2[96:288] == bytes(192) and proofs2[192:576] == bytes(384)
    assert (pks2[:96], proofs2[:192], pks2[288:], proofs2[576:]) == (pks[:96], proofs[:192], pks[96:192], proofs[192:384])


@pytest.mark.parametrize("form", ["rows", "spread", "plain"])
def test_every_hash_map_executor(m, S, rows_max_n, proved, form):
    import bls12381_py as o
    import c_oracle as co
    import util
    n = {"rows": rows_max_n, "spread": rows_max_n + 1, "plain": 130}[form]
    coop = form != "plain"
    assert ("rows", "spread", "plain")[util.slice_plan(n, S, coop=coop)["hash_map"]] == form
    threads = 64
    c = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=threads)
    try:
        c.set_cooperative(coop)
        pks, proofs, bad = with_bad(*proved, n)
        got = m.popVerifyEach(c, pks, proofs)
        assert [i for i, v in enumerate(got) if not v] == bad
        rnd = hashlib.sha256(b"pop executors " + form.encode()).digest()
        assert m.batchPopVerify(c, pks, proofs, rnd) is False
        good = [i for i in range(n) if i not in bad]
        gk, gp = [pks[i] for i in good], [proofs[i] for i in good]
        assert m.batchPopVerify(c, gk, gp, rnd) is True
        ng = len(good)
        H = c.fetch(1, 288 * ng)
        for j in sorted(random.Random(n).sample(range(ng), 14) + [0, ng - 1]):
            assert o_affine_g2(H[288 * j:288 * j + 288]) == co.hash_to_g2(compress(gk[j]), o.DST_POP), (form, j)
        r = c.fetch(0, 8 * ng)
        assert [int.from_bytes(r[8 * j:8 * j + 8], "little") for j in range(ng)] == o.blinding_scalars(rnd, ng, threads)
    finally:
        c.close()


def test_batch_value(m):
    import bls12381_py as o
    from util import fp12_from_bytes
    fx, pks, proofs = fixture_arrays()
    b = fx["batch"]
    idx, rnd = b["indices"], bytes.fromhex(b["rnd"])
    gk, gp = [pks[96 * i:96 * i + 96] for i in idx], [proofs[192 * i:192 * i + 192] for i in idx]
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=b["num_threads"])
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            assert m.batchPopVerify(c, gk, gp, rnd) is True
            assert c.fetch(4, 576).hex() == b["gt"]
            r = c.fetch(0, 8 * len(idx))
            assert [int.from_bytes(r[8 * j:8 * j + 8], "little") for j in range(len(idx))] == b["scalars"]
            sp = list(gp)
            sp[1], sp[4] = sp[4], sp[1]
            assert m.batchPopVerify(c, gk, sp, rnd) is False                                 # the blinding tells them apart ...
            ok, gts = m.popVerifyEachValues(c, [gk[1], gk[4]], [sp[1], sp[4]])
            assert ok == [False, False]
            assert o.f12mul(fp12_from_bytes(gts[0]), fp12_from_bytes(gts[1])) == o.F12_ONE      # ... although the unblinded product over the two is one
    finally:
        c.close()


def test_slicing(m, proved):
    import util
    from test_vereach_plan import plan_each_lib, slices
    n = 150
    bounds = set()
    for first, cnt in slices(plan_each_lib(), n, 64)[1]:                                     # the per-pair pass of the small context
        bounds |= {first, first + cnt - 1}
    L = util.plan_lib()
    ns, done = L.plan_shard_nslices(n, 64), 0
    assert ns == 3 and L.plan_shard_nslices(n, 256) == 1 and slices(plan_each_lib(), n, 256)[1] == [(0, n)]
    for s in range(ns):                                                                      # the batch pass's slices
        cnt = L.plan_shard_slice_count(n, done, ns, s)
        bounds |= {done, done + cnt - 1}
        done += cnt
    bad = sorted(bounds)
    assert bad[0] == 0 and bad[-1] == n - 1 and len(bad) >= 6
    pks, proofs = list(proved[0][:n]), list(proved[1][:n])
    for k, i in enumerate(bad):
        if k % 3 == 0:
            proofs[i] = proved[1][n + k]                                                     # another key's proof
        elif k % 3 == 1:
            proofs[i] = bytes(192)
        else:
            pks[i] = bytes(96)
    rnd = hashlib.sha256(b"pop slicing").digest()
    small, big = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=64), m.BatchedBLSVerifierCache.init(max_sets=256, numThreads=64)
    try:
        v_small, gt_small = m.popVerifyEachValues(small, pks, proofs)
        v_big, gt_big = m.popVerifyEachValues(big, pks, proofs)
        assert v_small == v_big and gt_small == gt_big
        assert [i for i, v in enumerate(v_big) if not v] == bad
        assert m.batchPopVerify(small, pks, proofs, rnd) is False and m.batchPopVerify(big, pks, proofs, rnd) is False
        assert m.batchPopVerifyLocate(small, pks, proofs, rnd) == (False, v_big)
        gk, gp = proved[0][:n], proved[1][:n]
        assert m.batchPopVerify(small, gk, gp, rnd) is True and m.batchPopVerify(big, gk, gp, rnd) is True
        assert small.fetch(4, 576) == big.fetch(4, 576)
    finally:
        small.close()
        big.close()


def test_locate(m, cache, proved):
    rnd = hashlib.sha256(b"pop locate").digest()
    pks, proofs = proved[0][:300], proved[1][:300]
    before = m.verifyEachPasses(cache)
    assert m.batchPopVerifyLocate(cache, pks, proofs, rnd) == (True, [True] * 300)
    assert m.verifyEachPasses(cache) == before                                               # a passing batch pays for no per-pair pass
    one = list(proofs)
    one[123] = proofs[124]
    ok, v = m.batchPopVerifyLocate(cache, pks, one, rnd)
    assert ok is False and [i for i, x in enumerate(v) if not x] == [123]
    assert m.verifyEachPasses(cache) == before + 1
    assert m.batchPopVerifyLocate(cache, b"", b"", rnd) == (False, [])


def test_position_and_neighbour_independence(m, cache, proved):
    rng = random.Random(7)
    pks, proofs = list(proved[0][:200]), list(proved[1][:200])
    bad = sorted(rng.sample(range(200), 40))
    for k, i in enumerate(bad):
        if k % 3 == 0:
            proofs[i] = proved[1][200 + k]
        elif k % 3 == 1:
            proofs[i] = bytes(192)
        else:
            pks[i] = bytes(96)
    alone = m.popVerifyEach(cache, pks, proofs)
    assert [i for i, v in enumerate(alone) if not v] == bad
    perm = list(range(200))
    rng.shuffle(perm)
    got = m.popVerifyEach(cache, [pks[p] for p in perm], [proofs[p] for p in perm])
    assert [got[perm.index(i)] for i in range(200)] == alone
    at = sorted(rng.sample(range(1200), 200))                                                # the same pairs among other neighbours
    mk, mp, it, k = [], [], iter(range(300, 1300)), 0
    for pos in range(1200):
        if k < 200 and pos == at[k]:
            mk.append(pks[k]); mp.append(proofs[k])
            k += 1
        else:
            j = next(it)
            mk.append(proved[0][j]); mp.append(proved[1][j])
    got = m.popVerifyEach(cache, mk, mp)
    assert [got[p] for p in at] == alone and sum(got) == 1200 - len(bad)


def device_bytes(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def test_device_forms_and_resources(m, proved):
    """create, use every new entry point (host and device forms, a sliced call among them), destroy: the resource count returns to where it was"""
    import torch
    torch.cuda.init()
    L = m.lib()
    start = L.mi355_bls_debug_live_resources()
    n = 100
    pks, proofs, bad = with_bad(*proved, n)
    rnd = hashlib.sha256(b"pop device forms").digest()
    c = m.BatchedBLSVerifierCache.init(max_sets=48, numThreads=16)
    try:
        assert L.mi355_bls_debug_live_resources() > start
        dk, dp = device_bytes(torch, b"".join(pks)), device_bytes(torch, b"".join(proofs))
        torch.cuda.synchronize()
        want = [i not in bad for i in range(n)]
        assert m.popVerifyEach(c, pks, proofs) == want
        assert m.popVerifyEach_device(c, dk.data_ptr(), dp.data_ptr(), n) == want
        assert m.popVerifyEachValues(c, pks, proofs)[0] == want
        assert m.batchPopVerify(c, pks, proofs, rnd) is False
        assert m.batchPopVerify_device(c, dk.data_ptr(), dp.data_ptr(), n, rnd) is False
        assert m.batchPopVerifyLocate(c, pks, proofs, rnd) == (False, want)
        assert m.batchPopVerifyLocate_device(c, dk.data_ptr(), dp.data_ptr(), n, rnd) == (False, want)
        gk, gp = device_bytes(torch, b"".join(proved[0][:n])), device_bytes(torch, b"".join(proved[1][:n]))
        torch.cuda.synchronize()
        assert m.batchPopVerify_device(c, gk.data_ptr(), gp.data_ptr(), n, rnd) is True
        assert m.batchPopVerifyLocate_device(c, gk.data_ptr(), gp.data_ptr(), n, rnd) == (True, [True] * n)
        comp = m.compressPublicKeys(c, pks)
        assert comp == [compress(k) for k in pks]
        dc = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
        m.compressPublicKeys_device(c, dk.data_ptr(), n, dc.data_ptr())
        assert bytes(dc.cpu().numpy()) == b"".join(comp)
        sks = b"".join(seeded_sks(n))
        dsk = device_bytes(torch, sks)
        opk, opr = torch.zeros(96 * n, dtype=torch.uint8, device="cuda"), torch.zeros(192 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ok, st = m.popProve_device(c, dsk.data_ptr(), n, opk.data_ptr(), opr.data_ptr())
        assert ok and st == bytes(n)
        assert bytes(opk.cpu().numpy()) == b"".join(proved[0][:n]) and bytes(opr.cpu().numpy()) == b"".join(proved[1][:n])
        assert m.popProve(c, sks)[1:3] == (b"".join(proved[0][:n]), b"".join(proved[1][:n]))
    finally:
        c.close()
    assert L.mi355_bls_debug_live_resources() == start


def test_an_ordinary_batch_after_a_pop_call(m, proved):
    """the PoP calls pass their tag with the call: the context's DST state is what it was"""
    import c_oracle as co
    rnd = hashlib.sha256(b"batch beside pop").digest()
    rec = co.make_batch(8, seed=20263)
    ok, st = co.batch_verify(rec, rnd, 4, stages=True)
    assert ok
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            assert m.popVerifyEach(c, proved[0][:8], proved[1][:8]) == [True] * 8
            assert m.batchPopVerify(c, proved[0][:8], proved[1][:8], rnd) is True
            assert m.batchVerifyParallel(c, rec, rnd) is True
            assert c.fetch(4, 576) == st["gt"]
            assert o_affine_g2(c.fetch(1, 288 * 8)[:288]) == st["H"][:192]
            assert m.verifyEach(c, rec) == [True] * 8
    finally:
        c.close()
