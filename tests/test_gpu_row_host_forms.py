"""The host and the device form of the per-row calls (compressPublicKeys, compressSignatures, deserializeSignatures, deserializePublicKeys,
signSets, popProve, admitKeys, mi355_bls_deserialize_sets_ex, mi355_bls_batch_verify_compressed, and popVerifyEach as the consumer of the
staged key and proof columns) on ONE context of 64 sets, each at n = 0, 1, 64, 65 and then 3 rows, in that order: 64 is a full wave and exactly
the staging capacity; 65 adds a second workgroup with one live lane and is more than the staging buffers hold, so they grow and every column
(csrc/plan.hpp cols) moves; the 3 rows behind it run on the moved columns.  Since only the first 65-row call of the module's context grows it,
every host form also runs its 65 rows as the FIRST call of a fresh 64-set context and must give the same bytes.  At every n the host form's
outputs, status bytes and return value equal the device form's byte for byte, and the device form's equal what the feature's own test holds
them to (the C restatement's keys, signatures, proofs and decoder; the big-integer oracle's compression).  Where a call has a notion of a bad
row, every n > 0 runs a second time with one at the LAST position - an undecodable signature or key, a secret key of zero, a proof swapped
with the row before - and the call then returns 0 with status bytes that name that row (the swap: both rows)."""
import contextlib
import ctypes
import hashlib

import pytest

pytestmark = pytest.mark.gpu

NS = (0, 1, 64, 65, 3)
ROWS = 66                            # one more than the largest n: the single row of n = 1 takes row 1's proof as "another row's"
RND = hashlib.sha256(b"row host forms rnd").digest()
BAD_SIG96 = bytes(96)                # no compression bit: Signature.fromBytes refuses it (status 4)
BAD_KEY48 = bytes(48)                # likewise for PublicKey.fromBytes (status 1)


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


@contextlib.contextmanager
def fresh(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        yield c
    finally:
        c.close()


def dev(b):
    import torch
    t = torch.frombuffer(bytearray(b if b else b"\0"), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def dev_out(nbytes):
    import torch
    t = torch.full((nbytes + 4,), 0xee, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t, nbytes):
    """the first nbytes of a dev_out buffer; the four bytes behind them are as they were"""
    import torch
    torch.cuda.synchronize()
    b = bytes(t.cpu().numpy())
    assert b[nbytes:] == b"\xee" * 4
    return b[:nbytes]


def rows(b, unit, n):
    return [b[unit * i:unit * i + unit] for i in range(n)]


@pytest.fixture(scope="module")
def ref():
    """ROWS rows of everything the calls take and give, from the C restatement and the big-integer oracle: computed once, never changed"""
    import bls12381_py as o
    import c_oracle as co
    r = {}
    sks = [int.from_bytes(hashlib.sha256(b"row host forms sk %d" % i).digest()[:31] + b"\0", "little") for i in range(ROWS)]
    r["sk"] = [s.to_bytes(32, "little") for s in sks]
    r["msg"] = [hashlib.sha256(b"row host forms msg %d" % i).digest() for i in range(ROWS)]
    r["pk96"] = [co.sk_to_pk(s) for s in sks]
    r["sig192"] = [co.sign(s, mg) for s, mg in zip(sks, r["msg"])]
    r["rec"] = [k + mg + s for k, mg, s in zip(r["pk96"], r["msg"], r["sig192"])]
    r["pk48"] = [o.g1_compress(o.g1_from_blst_affine(k)) for k in r["pk96"]]          # as tests/test_gpu_pop.py compresses
    r["proof192"] = [co.g2_mul(co.hash_to_g2(c48, o.DST_POP), s) for c48, s in zip(r["pk48"], sks)]
    pk48, _, sig96 = co.compress_sets(b"".join(r["rec"]))
    assert rows(pk48, 48, ROWS) == r["pk48"]                                         # the two compressors of the oracles agree
    r["sig96"] = rows(sig96, 96, ROWS)
    r["proof96"] = rows(co.compress_sets(b"".join(k + bytes(32) + p for k, p in zip(r["pk96"], r["proof192"])))[2], 96, ROWS)
    wide = co.serialize_sets(b"".join(r["rec"]))
    r["pk96w"], r["sig192w"] = rows(wide[0], 96, ROWS), rows(wide[1], 192, ROWS)     # the uncompressed wire forms
    return r


def variants(n, has_bad=True):
    return (False, True) if n and has_bad else (False,)


def one_stage_only(cache):
    t = cache.timings()
    assert t["blinding"] == t["total"] > 0, t
    assert all(v == 0 for k, v in t.items() if k not in ("blinding", "total")), t


def test_compress_public_keys(m, cache, ref):
    for n in NS:
        keys = b"".join(ref["pk96"][:n])
        got_h = m.compressPublicKeys(cache, keys)
        d_in, d_out = dev(keys), dev_out(48 * n)
        m.compressPublicKeys_device(cache, d_in.data_ptr(), n, d_out.data_ptr())
        got_d = rows(host(d_out, 48 * n), 48, n)
        assert got_h == got_d == ref["pk48"][:n], n
        if n == 65:
            with fresh(m) as c2:
                assert m.compressPublicKeys(c2, keys) == got_h


def test_compress_signatures(m, cache, ref):
    for n in NS:
        sigs = b"".join(ref["sig192"][:n])
        got_h = m.compressSignatures(cache, sigs)
        d_in, d_out = dev(sigs), dev_out(96 * n)
        m.compressSignatures_device(cache, d_in.data_ptr(), n, d_out.data_ptr())
        got_d = rows(host(d_out, 96 * n), 96, n)
        assert got_h == got_d == ref["sig96"][:n], n
        if n == 65:
            with fresh(m) as c2:
                assert m.compressSignatures(c2, sigs) == got_h


@pytest.mark.parametrize("wide", (False, True))
def test_deserialize_signatures(m, cache, ref, wide):
    for n in NS:
        for bad in variants(n):
            wire = list(ref["sig192w" if wide else "sig96"][:n])
            if bad:
                wire[-1] = BAD_SIG96 * (2 if wide else 1)
            wire = b"".join(wire)
            got_h = m.deserializeSignatures(cache, wire, sig_uncompressed=wide)
            d_in, d_out = dev(wire), dev_out(192 * n)
            ok_d, st_d = m.deserializeSignatures_device(cache, d_in.data_ptr(), n, d_out.data_ptr(), sig_uncompressed=wide)
            assert got_h == (ok_d, host(d_out, 192 * n), st_d), (n, bad)
            want = ref["sig192"][:n - 1] + [bytes(192)] if bad else ref["sig192"][:n]
            assert got_h == (not bad, b"".join(want), bytes(n - 1) + b"\x04" if bad else bytes(n)), (n, bad)
            if n == 65:
                with fresh(m) as c2:
                    assert m.deserializeSignatures(c2, wire, sig_uncompressed=wide) == got_h


@pytest.mark.parametrize("wide", (False, True))
def test_deserialize_public_keys(m, cache, ref, wide):
    for n in NS:
        for bad in variants(n):
            wire = list(ref["pk96w" if wide else "pk48"][:n])
            if bad:
                wire[-1] = BAD_KEY48 * (2 if wide else 1)
            wire = b"".join(wire)
            got_h = m.deserializePublicKeys(cache, wire, pk_uncompressed=wide)
            d_in, d_out = dev(wire), dev_out(96 * n)
            ok_d, st_d = m.deserializePublicKeys_device(cache, d_in.data_ptr(), n, d_out.data_ptr(), pk_uncompressed=wide)
            assert got_h == (ok_d, host(d_out, 96 * n), st_d), (n, bad)
            want = ref["pk96"][:n - 1] + [bytes(96)] if bad else ref["pk96"][:n]
            assert got_h == (not bad, b"".join(want), bytes(n - 1) + b"\x01" if bad else bytes(n)), (n, bad)
            if n == 65:
                with fresh(m) as c2:
                    assert m.deserializePublicKeys(c2, wire, pk_uncompressed=wide) == got_h


def test_sign_sets(m, cache, ref):
    for n in NS:
        for bad in variants(n):
            sks = b"".join(ref["sk"][:n - 1] + [bytes(32)] if bad else ref["sk"][:n])
            msgs = b"".join(ref["msg"][:n])
            got_h = m.signSets(cache, sks, msgs)
            if n:
                one_stage_only(cache)
            d_sk, d_ms, d_out = dev(sks), dev(msgs), dev_out(320 * n)
            ok_d, st_d = m.signSets_device(cache, d_sk.data_ptr(), d_ms.data_ptr(), n, d_out.data_ptr())
            if n:
                one_stage_only(cache)
            assert got_h == (ok_d, host(d_out, 320 * n), st_d), (n, bad)
            ok, recs, st = got_h
            assert (ok, st) == (not bad, bytes(n - 1) + b"\x01" if bad else bytes(n)), (n, bad)
            good = n - 1 if bad else n
            assert recs[:320 * good] == b"".join(ref["rec"][:good]), (n, bad)
            if bad:                                                                  # publicFromSecret is false: a zeroed key and signature
                assert recs[320 * good:320 * good + 96] == bytes(96) and recs[320 * good + 128:] == bytes(192)
            if n == 65:
                with fresh(m) as c2:
                    assert m.signSets(c2, sks, msgs) == got_h


def test_pop_prove(m, cache, ref):
    for n in NS:
        for bad in variants(n):
            sks = b"".join(ref["sk"][:n - 1] + [bytes(32)] if bad else ref["sk"][:n])
            got_h = m.popProve(cache, sks)
            if n:
                one_stage_only(cache)
            d_sk, d_pk, d_pr = dev(sks), dev_out(96 * n), dev_out(192 * n)
            ok_d, st_d = m.popProve_device(cache, d_sk.data_ptr(), n, d_pk.data_ptr(), d_pr.data_ptr())
            if n:
                one_stage_only(cache)
            assert got_h == (ok_d, host(d_pk, 96 * n), host(d_pr, 192 * n), st_d), (n, bad)
            good = n - 1 if bad else n
            want_pk = ref["pk96"][:good] + [bytes(96)] * (n - good)
            want_pr = ref["proof192"][:good] + [bytes(192)] * (n - good)
            assert got_h == (not bad, b"".join(want_pk), b"".join(want_pr), bytes(good) + b"\x01" * (n - good)), (n, bad)
            if n == 65:
                with fresh(m) as c2:
                    assert m.popProve(c2, sks) == got_h


def swapped_proofs(proofs, n):
    """(the first n proofs with the last one swapped with the one before it - for n = 1, replaced by the next row's -, the rows that no longer verify)"""
    p = list(proofs[:n])
    if n == 1:
        p[0] = proofs[1]
        return p, [0]
    p[n - 2], p[n - 1] = p[n - 1], p[n - 2]
    return p, [n - 2, n - 1]


def test_admit_keys(m, cache, ref):
    for n in NS:
        for bad in variants(n):
            pk = b"".join(ref["pk48"][:n])
            proofs, refused = swapped_proofs(ref["proof96"], n) if bad else (ref["proof96"][:n], [])
            pr = b"".join(proofs)
            got_h = m.admitKeys(cache, pk, pr, RND)
            d_pk, d_pr, d_out = dev(pk), dev(pr), dev_out(96 * n)
            ok_d, st_d = m.admitKeys_device(cache, d_pk.data_ptr(), d_pr.data_ptr(), n, RND, d_out.data_ptr())
            assert got_h == (ok_d, host(d_out, 96 * n), st_d), (n, bad)
            table = b"".join(bytes(96) if i in refused else ref["pk96"][i] for i in range(n))
            assert got_h == (not bad, table, bytes(m.KEY_BAD_PROOF if i in refused else 0 for i in range(n))), (n, bad)
            if n == 65:
                with fresh(m) as c2:
                    assert m.admitKeys(c2, pk, pr, RND) == got_h


def test_pop_verify_each(m, cache, ref):
    for n in NS:
        for bad in variants(n):
            pk = b"".join(ref["pk96"][:n])
            proofs, refused = swapped_proofs(ref["proof192"], n) if bad else (ref["proof192"][:n], [])
            pr = b"".join(proofs)
            got_h = m.popVerifyEach(cache, pk, pr)
            d_pk, d_pr = dev(pk), dev(pr)
            got_d = m.popVerifyEach_device(cache, d_pk.data_ptr(), d_pr.data_ptr(), n)
            assert got_h == got_d == [i not in refused for i in range(n)], (n, bad)
            if n:                                                                    # the C call: 1 iff every pair verified
                out = ctypes.create_string_buffer(n)
                assert m.lib().mi355_bls_pop_verify_each(cache._h, pk, pr, n, out) == (0 if bad else 1)
            if n == 65:
                with fresh(m) as c2:
                    assert m.popVerifyEach(c2, pk, pr) == got_h


def wire_sets(ref, n, bad, flags):
    pk = b"".join(ref["pk96w" if flags & 1 else "pk48"][:n])
    sg = list(ref["sig192w" if flags & 2 else "sig96"][:n])
    if bad:
        sg[-1] = BAD_SIG96 * (2 if flags & 2 else 1)
    return pk, b"".join(ref["msg"][:n]), b"".join(sg)


@pytest.mark.parametrize("flags", (0, 3))            # 3: both columns at their widest, the signatures' ending with the row
def test_deserialize_sets_ex(m, cache, ref, flags):
    import c_oracle as co
    L = m.lib()
    for n in NS:
        for bad in variants(n):
            pk, ms, sg = wire_sets(ref, n, bad, flags)
            out_h, st_h = ctypes.create_string_buffer(b"\xee" * (320 * n + 4), 320 * n + 4), ctypes.create_string_buffer(b"\xee" * (n + 4), n + 4)
            rc_h = L.mi355_bls_deserialize_sets_ex(cache._h, pk, ms, sg, n, flags, out_h, st_h)
            if n:
                one_stage_only(cache)
            d_pk, d_ms, d_sg = dev(pk), dev(ms), dev(sg)
            out_d, st_d = ctypes.create_string_buffer(b"\xee" * (320 * n + 4), 320 * n + 4), ctypes.create_string_buffer(b"\xee" * (n + 4), n + 4)
            rc_d = L.mi355_bls_deserialize_sets_ex_device(cache._h, d_pk.data_ptr(), d_ms.data_ptr(), d_sg.data_ptr(), n, flags, None, out_d, st_d)
            if n:
                one_stage_only(cache)
            assert (rc_h, out_h.raw, st_h.raw) == (rc_d, out_d.raw, st_d.raw), (n, bad)
            assert out_d.raw[320 * n:] == b"\xee" * 4 and st_d.raw[n:] == b"\xee" * 4      # nothing written behind either
            assert rc_d == (0 if bad else 1) and st_d.raw[:n] == (bytes(n - 1) + b"\x04" if bad else bytes(n)), (n, bad)
            good = n - 1 if bad else n
            assert out_d.raw[:320 * good] == b"".join(ref["rec"][:good]), (n, bad)
            if n:
                ok_c, out_c, st_c = co.deserialize_sets_ex(pk, ms, sg, flags)
                assert (bool(rc_d), st_d.raw[:n], out_d.raw[:320 * good]) == (ok_c, st_c, out_c[:320 * good]), (n, bad)
            if flags == 0:                                                           # the form without flags forwards to this one
                out_p, st_p = ctypes.create_string_buffer(320 * n + 4), ctypes.create_string_buffer(n + 4)
                assert L.mi355_bls_deserialize_sets(cache._h, pk, ms, sg, n, out_p, st_p) == rc_h
                assert (out_p.raw[:320 * n], st_p.raw[:n]) == (out_h.raw[:320 * n], st_h.raw[:n]), (n, bad)
            if n == 65:
                with fresh(m) as c2:
                    out_f, st_f = ctypes.create_string_buffer(320 * n), ctypes.create_string_buffer(n)
                    assert L.mi355_bls_deserialize_sets_ex(c2._h, pk, ms, sg, n, flags, out_f, st_f) == rc_h
                    assert (out_f.raw, st_f.raw) == (out_h.raw[:320 * n], st_h.raw[:n]), bad


def test_batch_verify_compressed(m, cache, ref):
    import c_oracle as co
    L = m.lib()
    for n in NS:
        for bad in variants(n):
            pk, ms, sg = wire_sets(ref, n, bad, 0)
            st_h = ctypes.create_string_buffer(b"\xee" * (n + 4), n + 4)
            rc_h = L.mi355_bls_batch_verify_compressed(cache._h, pk, ms, sg, n, RND, st_h)
            if n:
                assert L.mi355_bls_last_deser_ms(cache._h) > 0
            d_pk, d_ms, d_sg = dev(pk), dev(ms), dev(sg)
            st_d = ctypes.create_string_buffer(b"\xee" * (n + 4), n + 4)
            rc_d = L.mi355_bls_batch_verify_compressed_device(cache._h, d_pk.data_ptr(), d_ms.data_ptr(), d_sg.data_ptr(), n, RND, None, st_d)
            if n:
                assert L.mi355_bls_last_deser_ms(cache._h) > 0
            assert (rc_h, st_h.raw) == (rc_d, st_d.raw), (n, bad)
            if n == 0:
                assert rc_d == 0 and st_d.raw == b"\xee" * 4                          # no sets: false, nothing written
                continue
            assert st_d.raw == (bytes(n - 1) + b"\x04" if bad else bytes(n)) + b"\xee" * 4, (n, bad)
            assert rc_d == (0 if bad else 1), (n, bad)
            if not bad:
                assert co.batch_verify(b"".join(ref["rec"][:n]), RND, 4) is True
            if n == 65:
                with fresh(m) as c2:
                    st_f = ctypes.create_string_buffer(n)
                    assert L.mi355_bls_batch_verify_compressed(c2._h, pk, ms, sg, n, RND, st_f) == rc_h and st_f.raw == st_h.raw[:n], bad
    # the records verify, so a valid signature under another row's message must not
    pk, ms, sg = wire_sets(ref, 3, False, 0)
    st = ctypes.create_string_buffer(3)
    assert L.mi355_bls_batch_verify_compressed(cache._h, pk, ms[32:] + ms[:32], sg, 3, RND, st) == 0 and st.raw == bytes(3)


def test_nothing_to_do(m, cache):
    """n = 0 at the C entry points themselves (the wrappers answer it without a call): the documented return value, nothing read or written"""
    L, h = m.lib(), cache._h
    st = ctypes.create_string_buffer(b"\xee" * 4, 4)
    d = dev_out(0)
    p = d.data_ptr()
    assert L.mi355_bls_compress_public_keys(h, None, 0, None) == 0 and L.mi355_bls_compress_public_keys_device(h, None, 0, p, None) == 0
    assert L.mi355_bls_compress_signatures(h, None, 0, None) == 0 and L.mi355_bls_compress_signatures_device(h, None, 0, p, None) == 0
    assert L.mi355_bls_deserialize_signatures(h, None, 0, 0, None, st) == 1 and L.mi355_bls_deserialize_signatures_device(h, None, 0, 0, p, st, None) == 1
    assert L.mi355_bls_deserialize_public_keys(h, None, 0, 0, None, st) == 1 and L.mi355_bls_deserialize_public_keys_device(h, None, 0, 0, p, st, None) == 1
    assert L.mi355_bls_sign_sets(h, None, None, 0, None, st) == 1 and L.mi355_bls_sign_sets_device(h, None, None, 0, p, None, st) == 1
    assert L.mi355_bls_pop_prove(h, None, 0, None, None, st) == 1 and L.mi355_bls_pop_prove_device(h, None, 0, p, p, None, st) == 1
    assert L.mi355_bls_admit_keys(h, None, None, 0, 0, RND, None, st) == 1 and L.mi355_bls_admit_keys_device(h, None, None, 0, 0, RND, p, st, None) == 1
    assert L.mi355_bls_deserialize_sets_ex(h, None, None, None, 0, 0, None, st) == 1
    assert L.mi355_bls_deserialize_sets_ex_device(h, None, None, None, 0, 0, None, None, st) == 1
    assert L.mi355_bls_deserialize_sets(h, None, None, None, 0, None, st) == 1 and L.mi355_bls_deserialize_sets_device(h, None, None, None, 0, None, None, st) == 1
    assert L.mi355_bls_batch_verify_compressed(h, None, None, None, 0, RND, st) == 0
    assert L.mi355_bls_batch_verify_compressed_device(h, None, None, None, 0, RND, None, st) == 0
    assert L.mi355_bls_pop_verify_each(h, None, None, 0, st) == 0 and L.mi355_bls_pop_verify_each_device(h, None, None, 0, st, None) == 0
    # the refusals the two forms of deserialize_sets share, in the same order: a null context, then n = 0, then a null array
    assert L.mi355_bls_deserialize_sets(None, None, None, None, 0, None, st) == L.mi355_bls_deserialize_sets_ex(None, None, None, None, 0, 0, None, st) < 0
    assert L.mi355_bls_deserialize_sets(h, None, b"\0" * 32, b"\0" * 96, 1, None, st) == L.mi355_bls_deserialize_sets_ex(h, None, b"\0" * 32, b"\0" * 96, 1, 0, None, st) < 0
    assert L.mi355_bls_deserialize_sets_ex(h, None, None, None, 0, 8, None, st) < 0                      # unknown flag bits come before n = 0
    assert st.raw == b"\xee" * 4 and host(d, 0) == b""
