"""GPU: fromBytes on the encodings an attacker would pick (tests/golden/deser_adversarial.json, tests/golden/gen_deser_adversarial.py) - points of
small order and of every torsion subgroup of E(Fp) and E'(Fp2) outside G1 / G2, G2 points whose y has a zero component, coordinates at
and around p, flag-bit edges, a bad key with a bad signature.  k_deser's compiled bodies (the endomorphism membership tests, the sign
rules, the Fp2 square root) against the fixture's statuses and the C restatement (decode by square root, membership by [r]P), with hostile
and valid tuples side by side in every wave.  The CPU half, with the big-integer oracle computed live, is tests/test_deser_adversarial_emu.py."""
import ctypes

import pytest

import bls12381_py as o
import deser_cases as dc

pytestmark = pytest.mark.gpu

N_VALID = 64


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


@pytest.fixture(scope="module")
def batches():
    """per wire-form combination: the tuples (hostile rows and 64 valid tuples interleaved), the statuses the fixture records and the C
    restatement's result for KNOWN_ON_CURVE off and on - computed once, never modified"""
    import c_oracle as co
    fx = dc.fixture()
    rec = co.make_batch(N_VALID, seed=4242)
    pk48, _, sg96 = co.compress_sets(rec)
    pk96, sg192 = co.serialize_sets(rec)
    out = {}
    for pku, sgu in dc.COMBOS:
        kb, sb = (96 if pku else 48), (192 if sgu else 96)
        ks, ss = (pk96 if pku else pk48), (sg192 if sgu else sg96)
        valid = [(ks[kb * i:kb * i + kb], ss[sb * i:sb * i + sb]) for i in range(N_VALID)]
        tuples = dc.layout(fx, pku, sgu, valid)
        n = len(tuples)
        assert n % 64 and 128 < n <= 192                                      # three waves, the last one partial
        pk, ms, sg = (b"".join(t[j] for t in tuples) for j in (1, 2, 3))
        flags = (dc.PK_UNCOMPRESSED if pku else 0) | (dc.SIG_UNCOMPRESSED if sgu else 0)
        b = {"rows": [t[0] for t in tuples], "tuples": tuples, "pk": pk, "ms": ms, "sg": sg, "n": n, "flags": flags}
        for k, known in enumerate((False, True)):
            b["want", known] = bytes(0 if i is None else fx["rows"][i]["st"][k] for i in b["rows"])
            b["c", known] = co.deserialize_sets_ex(pk, ms, sg, flags | (dc.KNOWN_ON_CURVE if known else 0))
        b["nonmember"] = [i is not None and fx["rows"][i]["nonmember"] for i in b["rows"]]
        out[pku, sgu] = b
    # every wave holds hostile and valid lanes next to each other
    rows = out[False, False]["rows"]
    for w in range(0, len(rows), 64):
        kinds = [r is None for r in rows[w:w + 64]]
        assert sum(kinds) >= 8 and sum(1 for a, b in zip(kinds, kinds[1:]) if a != b) >= 16
    return out


def _check_records(b, known, out, st):
    pku, sgu = bool(b["flags"] & dc.PK_UNCOMPRESSED), bool(b["flags"] & dc.SIG_UNCOMPRESSED)
    for k, (_, pkb, msg, sgb) in enumerate(b["tuples"]):
        r = out[320 * k:320 * k + 320]
        if st[k] == 0:
            assert r == dc.oracle_record(pkb, pku, msg, sgb, sgu), (k, b["rows"][k])       # the big-integer decode, byte for byte
        else:
            assert r[:96] == bytes(96) and r[128:] == bytes(192), (k, b["rows"][k])         # a failed tuple leaves no point behind


@pytest.mark.parametrize("pku,sgu", dc.COMBOS)
@pytest.mark.parametrize("known", (False, True))
def test_statuses_and_records_every_wire_form(m, cache, batches, pku, sgu, known):
    b = batches[pku, sgu]
    ok, out, st = m.deserializeSetsEx(cache, b["pk"], b["ms"], b["sg"], pk_uncompressed=pku, sig_uncompressed=sgu, known_on_curve=known)
    ok_c, out_c, st_c = b["c", known]
    bad = [(k, b["rows"][k], st[k], b["want", known][k], st_c[k]) for k in range(b["n"]) if not st[k] == b["want", known][k] == st_c[k]]
    assert not bad, bad
    assert ok == ok_c and not ok
    assert out == out_c
    _check_records(b, known, out, st)


def test_no_point_outside_the_subgroups_is_accepted(m, cache, batches):
    """The invariant on its own: with KNOWN_ON_CURVE off, no tuple that holds a curve point with [r]P != infinity - key or signature, any
    family, any wire form - comes back with status 0."""
    total = 0
    for (pku, sgu), b in batches.items():
        _, _, st = m.deserializeSetsEx(cache, b["pk"], b["ms"], b["sg"], pk_uncompressed=pku, sig_uncompressed=sgu)
        accepted = [b["rows"][k] for k in range(b["n"]) if b["nonmember"][k] and st[k] == 0]
        assert not accepted, accepted
        total += sum(b["nonmember"])
    assert total >= 4 * 58


def test_compressed_form_through_the_other_entry_points(m, cache, batches):
    """deserializeSets, batchVerifyCompressed (verdict false, the same statuses) and the three _device entry points with the arrays in
    device memory"""
    import numpy as np
    import torch
    b = batches[False, False]
    n, want = b["n"], b["want", False]
    _, out_c, st_c = b["c", False]
    assert m.deserializeSets(cache, b["pk"], b["ms"], b["sg"]) == (False, out_c, st_c) and st_c == want
    rnd = o.sha256(b"adversarial")
    assert m.batchVerifyCompressed(cache, b["pk"], b["ms"], b["sg"], rnd) == (False, want)
    d_pk, d_ms, d_sg = (torch.from_numpy(np.frombuffer(b[k], dtype=np.uint8).copy()).cuda() for k in ("pk", "ms", "sg"))
    torch.cuda.synchronize()
    L = m.lib()
    out, st = ctypes.create_string_buffer(320 * n), ctypes.create_string_buffer(n)
    assert m._check(L.mi355_bls_deserialize_sets_device(cache._h, d_pk.data_ptr(), d_ms.data_ptr(), d_sg.data_ptr(), n, None, out, st)) == 0
    assert (out.raw, st.raw) == (out_c, want)
    for known in (False, True):
        out, st = ctypes.create_string_buffer(320 * n), ctypes.create_string_buffer(n)
        rc = L.mi355_bls_deserialize_sets_ex_device(cache._h, d_pk.data_ptr(), d_ms.data_ptr(), d_sg.data_ptr(), n, dc.KNOWN_ON_CURVE if known else 0, None, out, st)
        assert m._check(rc) == 0 and (out.raw, st.raw) == (b["c", known][1], b["want", known])
    st = ctypes.create_string_buffer(n)
    assert m._check(L.mi355_bls_batch_verify_compressed_device(cache._h, d_pk.data_ptr(), d_ms.data_ptr(), d_sg.data_ptr(), n, rnd, None, st)) == 0
    assert st.raw == want
    # the uncompressed forms from device memory too
    u = batches[True, True]
    d_pk, d_ms, d_sg = (torch.from_numpy(np.frombuffer(u[k], dtype=np.uint8).copy()).cuda() for k in ("pk", "ms", "sg"))
    torch.cuda.synchronize()
    out, st = ctypes.create_string_buffer(320 * u["n"]), ctypes.create_string_buffer(u["n"])
    rc = L.mi355_bls_deserialize_sets_ex_device(cache._h, d_pk.data_ptr(), d_ms.data_ptr(), d_sg.data_ptr(), u["n"], u["flags"], None, out, st)
    assert m._check(rc) == 0 and (out.raw, st.raw) == (u["c", False][1], u["want", False])


def test_compress_public_keys_on_boundary_images(m, cache):
    """k_compress_pks takes images without validating them (it loads, compresses, stores): for y at 1, (p - 1) / 2, (p + 1) / 2, p - 1 under
    x = 0, 1, p - 1 and others the sign bit is the integer rule y > p - y and the x bytes are canonical.  No curve point has y = (p +- 1) / 2,
    so the boundary of fp_is_lex_largest - shared with popVerify's message - is reached only this way."""
    import numpy as np
    import torch
    imgs = dc.compress_boundary_images()
    want = [dc.compress_boundary_expect(x, y) for x, y in imgs]
    assert {w[0] & 0xe0 for w in want} == {0x80, 0xa0}
    pks = b"".join(o.g1_to_blst_affine(p) for p in imgs)
    assert m.compressPublicKeys(cache, pks) == want
    dk = torch.from_numpy(np.frombuffer(pks, dtype=np.uint8).copy()).cuda()
    dout = torch.zeros(48 * len(imgs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    m.compressPublicKeys_device(cache, dk.data_ptr(), len(imgs), dout.data_ptr())
    torch.cuda.synchronize()
    assert bytes(dout.cpu().numpy()) == b"".join(want)
