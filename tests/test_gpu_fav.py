"""GPU parity: G1 aggregateAll and fastAggregateVerify (bls_sig_min_pubkey.nim:234-258) through the C ABI."""
import hashlib

import pytest

import bls12381_py as o
from util import g1_jac_to_affine, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    return m.BatchedBLSVerifierCache.init(max_sets=16384)


def test_aggregate_golden(m, cache):
    a = golden("msm")["aggregate"]
    pts = bytes.fromhex(a["points"])
    out = m.aggregateAll(cache, pts)
    assert o.g1_to_blst_affine(g1_jac_to_affine(out)).hex() == a["sum_affine"]
    for n in (1, 2, 63, 64, 65, 200):
        sub = pts[:96 * n]
        want = o.aggregate_g1([o.g1_from_blst_affine(sub[96 * i:96 * i + 96]) for i in range(n)])
        assert g1_jac_to_affine(m.aggregateAll(cache, sub)) == want
    assert m.aggregateAll(cache, b"") is None
    # P + (-P) + Q = Q ; doubling inside the reduction: P + P
    p = o.g1_from_blst_affine(pts[:96])
    q = o.g1_from_blst_affine(pts[96:192])
    buf = o.g1_to_blst_affine(p) + o.g1_to_blst_affine(o.g1_neg(p)) + o.g1_to_blst_affine(q)
    assert g1_jac_to_affine(m.aggregateAll(cache, buf)) == q
    assert g1_jac_to_affine(m.aggregateAll(cache, pts[:96] * 2)) == o.g1_add(p, p)
    assert g1_jac_to_affine(m.aggregateAll(cache, o.g1_to_blst_affine(p) + o.g1_to_blst_affine(o.g1_neg(p)))) is None


def test_fast_aggregate_verify_golden(m, cache):
    for v in golden("fav"):
        pks, msg = bytes.fromhex(v["pks"]), bytes.fromhex(v["msg"])
        assert m.fastAggregateVerify(cache, pks, msg, bytes.fromhex(v["sig"])) is True
        assert m.fastAggregateVerify(cache, pks, msg, bytes.fromhex(v["bad_sig"])) is False
        assert m.fastAggregateVerify(cache, pks, msg + b"x", bytes.fromhex(v["sig"])) is False
    assert m.fastAggregateVerify(cache, b"", b"m", bytes(192)) is False     # empty -> false


def test_fast_aggregate_verify_32768(m, cache):
    """Config 3 shape: 32 768 distinct keys, one message, aggregate signature (C restatement as generator
    and checker): same aggregate point bit-exactly, same verdicts."""
    import c_oracle as co
    n = 32768
    sks = [int.from_bytes(hashlib.sha256(b"fav" + i.to_bytes(4, "little")).digest(), "little") % o.R or 1 for i in range(n)]
    pks = b"".join(co.sk_to_pk(sk) for sk in sks)
    msg = b"Mr F was here"
    hm = co.hash_to_g2(msg, o.DST_SIG)
    sig = co.g2_mul(hm, sum(sks) % o.R)
    bad = co.g2_mul(hm, (sum(sks) + 1) % o.R)
    assert o.g1_to_blst_affine(g1_jac_to_affine(m.aggregateAll(cache, pks))) == co.g1_sum(pks)
    assert m.fastAggregateVerify(cache, pks, msg, sig) is True
    print("timings(ms):", cache.timings())
    assert m.fastAggregateVerify(cache, pks, msg, bad) is False
    assert co.fast_aggregate_verify(pks, msg, sig) is True and co.fast_aggregate_verify(pks, msg, bad) is False
    # dropping one key breaks it
    assert m.fastAggregateVerify(cache, pks[96:], msg, sig) is False
    # the same keys sharded over 1, 3 and 8 contexts (devices in a deployment): same verdicts, same GT value
    gt = cache.fetch(4, 576) if m.fastAggregateVerify(cache, pks, msg, sig) else None
    for ngpu in (1, 3, 8):
        caches = [m.BatchedBLSVerifierCache.init(max_sets=64) for _ in range(ngpu)]
        assert m.fastAggregateVerifyMulti(caches, pks, msg, sig) is True
        assert caches[0].fetch(4, 576) == gt
        assert m.fastAggregateVerifyMulti(caches, pks, msg, bad) is False
        assert m.fastAggregateVerifyMulti(caches, pks[96:], msg, sig) is False
        assert m.fastAggregateVerifyMulti(caches, pks[:96 * 2], msg, sig) is False          # 2 keys on 8 devices: empty shards
        for c in caches:
            c.close()
    # one process per GPU: per-rank partial key sums (aggregateAll), added, then the pairing check on the aggregate
    parts = [m.aggregateAll(cache, pks[96 * a:96 * b]) for a, b in ((0, 10000), (10000, 20001), (20001, n))]
    agg = m.p1s_add(cache, parts)
    assert m.verifyAggregate(cache, agg, msg, sig) is True and cache.fetch(4, 576) == gt
    assert m.verifyAggregate(cache, agg, msg, bad) is False
    assert m.verifyAggregate(cache, bytes(144), msg, sig) is False                        # aggregate at infinity


@pytest.mark.gpu
def test_one_message_hash_of_a_32_byte_message(m, cache):
    """k_hash_one takes 32-byte messages through the batch path's prepared-constants expand_message_xmd and every other length through the byte-wise
    absorber: both against the C restatement's hash (the signature is made from it), around the boundary."""
    import c_oracle as co
    sks = [int.from_bytes(hashlib.sha256(b"h32" + bytes([i])).digest(), "little") % o.R or 1 for i in range(5)]
    pks = b"".join(co.sk_to_pk(sk) for sk in sks)
    root = hashlib.sha256(b"a signing root").digest()
    for msg in (root, root[:31], root + b"\x00", b"", root * 3):
        hm = co.hash_to_g2(msg, o.DST_SIG)
        sig, bad = co.g2_mul(hm, sum(sks) % o.R), co.g2_mul(hm, (sum(sks) + 1) % o.R)
        assert m.fastAggregateVerify(cache, pks, msg, sig) is True, len(msg)
        assert m.fastAggregateVerify(cache, pks, msg, bad) is False, len(msg)
    assert m.fastAggregateVerify(cache, pks, root[:31] + bytes([root[31] ^ 1]), co.g2_mul(co.hash_to_g2(root, o.DST_SIG), sum(sks) % o.R)) is False


def test_hash_one_against_rfc9380_and_oracle(m):
    """k_hash_one (two SSWU maps side by side, addition and cofactor clearing on the lane-team engine) through mi355_bls_debug_hash_to_g2: the RFC 9380
    J.10.1 vector of the empty message (tests/test_oracle_kats.py says where it comes from) under the RFC's own DST, and messages of several lengths under
    the scheme's DSTs against the oracle (32 bytes: the prepared-constants path; other lengths: the byte-wise absorber)."""
    import ctypes
    from util import g2_jac_to_affine
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    out = ctypes.create_string_buffer(288)

    def h(msg, dst):
        assert m._check(m.lib().mi355_bls_debug_hash_to_g2(cache._h, msg, len(msg), dst, len(dst), out)) == 0
        return g2_jac_to_affine(out.raw)

    rfc = b"QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_"
    assert h(b"", rfc) == ((int("0141ebfbdca40eb85b87142e130ab689c673cf60f1a3e98d69335266f30d9b8d4ac44c1038e9dcdd5393faf5c41fb78a", 16),
                            int("05cb8437535e20ecffaef7752baddf98034139c38452458baeefab379ba13dff5bf5dd71b72418717047f5b0f37da03d", 16)),
                           (int("0503921d7f6a12805e72940b963c0cf3471c7b2a524950ca195d11062ee75ec076daf2d4bc358c4b190c0c98064fdd92", 16),
                            int("12424ac32561493f3fe3c260708a12b7c620e7be00099a974e259ddc7d1f6395c3c811cdd19f1e8dbf3e9ecfdcbab8d6", 16)))
    pop = b"BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
    for msg, dst in ((b"abc", rfc), (bytes(range(32)), o.DST_SIG), (bytes(range(48)), pop), (b"x" * 200, o.DST_SIG), (bytes(32), pop)):
        assert h(msg, dst) == o.hash_to_g2(msg, dst)
    cache.close()


# ---- k_hash_one over message and DST lengths (mi355_bls_debug_hash_to_g2 against the C restatement; a spread against the Python oracle too)
SWEEP_MSG_LENS = list(range(192)) + [255, 256, 257, 4031, 4032, 4033, 4095, 4096]
SWEEP_DST_LENS = list(range(1, 65))


def _hook(m, cache):
    import ctypes
    from util import g2_jac_to_affine
    out = ctypes.create_string_buffer(288)

    def h(msg, dst):
        assert m._check(m.lib().mi355_bls_debug_hash_to_g2(cache._h, msg, len(msg), dst, len(dst), out)) == 0
        return o.g2_to_blst_affine(g2_jac_to_affine(out.raw))
    return h


def test_hash_one_over_message_lengths(m):
    """Every message length 0 .. 191 (three cycles of the residues mod 64: with the 43-byte DST the SHA-256 padding edges sit at residues 8, 9,
    16, 17), the lengths around 256, around 4 032 (= 63 * 64: the edges of the last block that fits) and the limit 4 096 (a full d_msg)."""
    import c_oracle as co
    from util import ctr_bytes
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    h = _hook(m, cache)
    assert {n % 64 for n in SWEEP_MSG_LENS[:192]} == set(range(64)) and all(r + 64 * k in SWEEP_MSG_LENS for r in (8, 9, 16, 17) for k in range(3))
    data = ctr_bytes(b"hash_one", 4096)
    py = {0, 8, 9, 16, 17, 32, 72, 81, 137, 144, 191, 256, 4032, 4096}
    for n in SWEEP_MSG_LENS:
        msg = data[4096 - n:] if n else b""                 # a different window for every length
        got = h(msg, o.DST_SIG)
        assert got == co.hash_to_g2(msg, o.DST_SIG), n
        if n in py:
            assert got == o.g2_to_blst_affine(o.hash_to_g2(msg, o.DST_SIG)), n
    cache.close()


def test_hash_one_over_dst_lengths(m):
    """DST lengths 1 .. 64 with a 32-byte message (the prepared-constants path from 28 bytes on, the byte-wise absorber below: both sides of the
    switch are in the range) and with a 33-byte one (the absorber throughout)."""
    import c_oracle as co
    from util import ctr_bytes
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    h = _hook(m, cache)
    assert 27 in SWEEP_DST_LENS and 28 in SWEEP_DST_LENS
    tag = ctr_bytes(b"dst", 64)
    msg = ctr_bytes(b"dst_msg", 33)
    py = {1, 27, 28, 43, 55, 64}
    for dn in SWEEP_DST_LENS:
        for x in (msg[:32], msg):
            got = h(x, tag[:dn])
            assert got == co.hash_to_g2(x, tag[:dn]), (dn, len(x))
            if dn in py:
                assert got == o.g2_to_blst_affine(o.hash_to_g2(x, tag[:dn])), (dn, len(x))
    cache.close()


def test_hash_one_refuses_lengths_beyond_its_limits(m):
    import ctypes
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    out = ctypes.create_string_buffer(288)
    f = m.lib().mi355_bls_debug_hash_to_g2
    ERR_ARG = -3
    assert f(cache._h, bytes(32), 32, bytes(65), 0, out) == ERR_ARG
    assert f(cache._h, bytes(32), 32, bytes(65), 65, out) == ERR_ARG
    assert f(cache._h, bytes(4097), 4097, o.DST_SIG, len(o.DST_SIG), out) == ERR_ARG
    assert f(cache._h, bytes(4096), 4096, o.DST_SIG, len(o.DST_SIG), out) == 0
    with pytest.raises(m.BlsGpuError):
        m._check(f(cache._h, bytes(4097), 4097, o.DST_SIG, len(o.DST_SIG), out))
    cache.close()


def test_messages_at_the_4096_byte_limit_through_the_entry_points(m, cache):
    """fastAggregateVerify and verifyAggregate with messages of 4 095 and 4 096 bytes: the message fills d_msg up to the byte where the signature is
    staged (d_msg + 4096) - a valid signature verifies, the scalar-plus-one signature does not; 4 097 bytes are refused by all three entry points."""
    import c_oracle as co
    from util import ctr_bytes
    sks = [int.from_bytes(hashlib.sha256(b"lim" + bytes([i])).digest(), "little") % o.R or 1 for i in range(5)]
    pks = b"".join(co.sk_to_pk(sk) for sk in sks)
    agg = m.aggregateAll(cache, pks)
    data = ctr_bytes(b"limit", 4097)
    for n in (4095, 4096):
        msg = data[:n]
        hm = co.hash_to_g2(msg, o.DST_SIG)
        sig, bad = co.g2_mul(hm, sum(sks) % o.R), co.g2_mul(hm, (sum(sks) + 1) % o.R)
        assert co.fast_aggregate_verify(pks, msg, sig) is True and co.fast_aggregate_verify(pks, msg, bad) is False
        assert m.fastAggregateVerify(cache, pks, msg, sig) is True, n
        assert m.fastAggregateVerify(cache, pks, msg, bad) is False, n
        assert m.fastAggregateVerify(cache, pks, msg[:-1] + bytes([msg[-1] ^ 1]), sig) is False, n       # the last byte before the staged signature
        assert m.verifyAggregate(cache, agg, msg, sig) is True, n
        assert m.verifyAggregate(cache, agg, msg, bad) is False, n
    sig = co.g2_mul(co.hash_to_g2(data, o.DST_SIG), sum(sks) % o.R)
    for call in (lambda: m.fastAggregateVerify(cache, pks, data, sig), lambda: m.verifyAggregate(cache, agg, data, sig),
                 lambda: m.fastAggregateVerifyMulti([cache], pks, data, sig)):
        with pytest.raises(m.BlsGpuError) as e:
            call()
        assert "error -3" in str(e.value)
    assert m.fastAggregateVerify(cache, pks, data[:4096], co.g2_mul(co.hash_to_g2(data[:4096], o.DST_SIG), sum(sks) % o.R)) is True     # the context still works
