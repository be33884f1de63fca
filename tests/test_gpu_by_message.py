"""batchVerify by message (mi355_bls_batch_verify_by_message) through the C ABI: for every input the verdict and the final value
(fetch_stage 4, byte for byte) are mi355_bls_batch_verify's on the same context, sets and random bytes, and the verdict is the CPU oracle's
(tests/c_oracle.py).  Inputs come from the device signer.  Group shapes: one message for all, all distinct, sizes 1, 2, 7, 8, 9 interleaved
(either side of the level-0 item width of the group sums), one group whose members sit in three different waves; both modes; one chain
and four; one bad member of three kinds; the stages the pass leaves; an infinite group sum through the scalar hook; slices that cut
groups; a crowded table; messages that differ in one byte only; and a context that is left as an ordinary call leaves it."""
import hashlib
import struct

import pytest

import bls12381_py as o
from util import g2_jac_to_affine

pytestmark = pytest.mark.gpu

DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
RND = hashlib.sha256(b"by-message rnd").digest()
SIZES = (1, 2, 3, 64, 65, 130)
MODES = [pytest.param(True, id="latency"), pytest.param(False, id="throughput")]


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def co():
    import c_oracle
    return c_oracle


@pytest.fixture(scope="module")
def signer(m):
    cache = m.BatchedBLSVerifierCache.init(max_sets=4096, numThreads=4)
    yield cache
    cache.close()


def msg(tag):
    return hashlib.sha256(b"by-message %d" % tag).digest() if isinstance(tag, int) else tag


def sk(i):
    return (0x1234567 + 977 * i).to_bytes(32, "little")


_signed = {}


def sign(m, signer, tags, first_key=0):
    """records of len(tags) sets: set i signs msg(tags[i]) with key first_key + i"""
    key = (tuple(tags), first_key)
    if key not in _signed:
        ok, rec, _ = m.signSets(signer, [sk(first_key + i) for i in range(len(tags))], [msg(t) for t in tags])
        assert ok
        _signed[key] = rec
    return _signed[key]


def shape(name, n):
    if name == "one":
        return [0] * n
    if name == "distinct":
        return list(range(n))
    if name == "interleaved":                       # groups of 1, 2, 7, 8, 9 members, dealt round-robin, then distinct messages
        left, tags = {g: s for g, s in enumerate((1, 2, 7, 8, 9))}, []
        while len(tags) < n and any(left.values()):
            for g in sorted(left):
                if left[g] and len(tags) < n:
                    tags.append(g)
                    left[g] -= 1
        return tags + list(range(100, 100 + n - len(tags)))
    assert name == "waves"                          # message 0 at the first lane of every wave and at the last set; everything else distinct
    return [0 if (i % 64 == 0 or i == n - 1) else 1000 + i for i in range(n)]


SHAPES = ("one", "distinct", "interleaved", "waves")
_oracle = {}


def oracle_verdict(co, rec, rnd, nthreads):
    key = (hashlib.sha256(rec).digest(), rnd, nthreads)
    if key not in _oracle:
        _oracle[key] = co.batch_verify(rec, rnd, nthreads)
    return _oracle[key]


def groups_of(rec):
    """the distinct messages in first-appearance order and the members of each"""
    order, members = [], {}
    for i in range(len(rec) // 320):
        mm = rec[320 * i + 96:320 * i + 128]
        if mm not in members:
            order.append(mm)
            members[mm] = []
        members[mm].append(i)
    return order, members


def both(m, cache, rec, rnd, label, want=None):
    """the by-message call and the ordinary one on the same context: verdict and final value equal; -> (verdict, k)"""
    n = len(rec) // 320
    got = m.batchVerifyByMessage(cache, rec, rnd)
    gt = cache.fetch(4, 576)
    k = m.lastMessageGroups(cache)
    ref = m.batchVerifyParallel(cache, rec, rnd)
    assert got is ref, label
    assert gt == cache.fetch(4, 576), label
    if want is not None:
        assert got is want, label
    if n <= cache.max_sets:
        assert k == len(groups_of(rec)[0]), label
    return got, k


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("coop", MODES)
def test_verdict_and_final_value_over_sizes_and_shapes(m, co, signer, coop, nthreads):
    cache = m.BatchedBLSVerifierCache.init(max_sets=192, numThreads=nthreads)
    cache.set_cooperative(coop)
    try:
        for n in SIZES:
            for name in SHAPES:
                rec = sign(m, signer, shape(name, n))
                label = "n = %d, %s" % (n, name)
                got, k = both(m, cache, rec, RND, label, want=True)
                assert got is oracle_verdict(co, rec, RND, nthreads), label
        if 130 in SIZES:
            assert len(groups_of(sign(m, signer, shape("waves", 130)))[1][msg(0)]) == 4      # lanes 0 of three waves, and the last set
    finally:
        cache.close()


def bad_batches(m, signer):
    """64 sets in four groups of 16, dealt round-robin (set i signs message i % 4), and three ways to spoil one member"""
    tags = [i % 4 for i in range(64)]
    rec = sign(m, signer, tags)
    other = sign(m, signer, [t + 50 for t in tags])          # the same keys over other messages
    i, j = 21, 41                                             # both in group 1
    assert tags[i] == tags[j]
    sig = lambda r, a: r[320 * a + 128:320 * a + 320]
    wrong_msg = rec[:320 * i + 128] + sig(other, i) + rec[320 * i + 320:]
    swapped = bytearray(rec)
    swapped[320 * i + 128:320 * i + 320], swapped[320 * j + 128:320 * j + 320] = sig(rec, j), sig(rec, i)
    wrong_key = rec[:320 * i] + rec[320 * 7:320 * 7 + 96] + rec[320 * i + 96:]
    return rec, {"a signature over another message": wrong_msg, "two signatures swapped inside a group": bytes(swapped), "another valid key": wrong_key}


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("coop", MODES)
def test_one_bad_member(m, co, signer, coop, nthreads):
    good, bad = bad_batches(m, signer)
    cache = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=nthreads)
    cache.set_cooperative(coop)
    try:
        both(m, cache, good, RND, "good", want=True)
        for label, rec in bad.items():
            got, k = both(m, cache, rec, RND, label, want=False)
            assert k == 4
            assert oracle_verdict(co, rec, RND, nthreads) is False, label
    finally:
        cache.close()


_R2, _R3 = pow(o.MONT_R, 2, o.P), pow(o.MONT_R, 3, o.P)


def same_g1(jac144, aff96):
    """the Jacobian image (X, Y, Z) is the affine point (x, y), on the Montgomery images themselves; the all-zero affine image: Z = 0"""
    X, Y, Z, x, y = (int.from_bytes(b, "little") for b in (jac144[:48], jac144[48:96], jac144[96:144], aff96[:48], aff96[48:96]))
    assert max(X, Y, Z, x, y) < o.P
    if x == 0 and y == 0:
        return Z == 0
    z2 = Z * Z % o.P
    return Z != 0 and X * _R2 % o.P == x * z2 % o.P and Y * _R3 % o.P == y * z2 * Z % o.P


@pytest.mark.parametrize("coop", MODES)
def test_stage_outputs(m, co, signer, coop):
    n = 130
    rec = sign(m, signer, shape("interleaved", n))
    order, members = groups_of(rec)
    cache = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4)
    cache.set_cooperative(coop)
    try:
        assert m.batchVerifyByMessage(cache, rec, RND) is True
        k = m.lastMessageGroups(cache)
        assert k == len(order) < n
        r = struct.unpack("<%dQ" % n, cache.fetch(0, 8 * n))
        assert all(r)
        H = cache.fetch(1, 288 * k)
        with pytest.raises(m.BlsGpuError):
            cache.fetch(1, 288 * k - 1)
        for g, mm in enumerate(order):
            assert o.g2_to_blst_affine(g2_jac_to_affine(H[288 * g:288 * g + 288])) == co.hash_to_g2(mm, DST), g
        P = cache.fetch(2, 144 * k)
        for g, mm in enumerate(order):
            pts = b"".join(rec[320 * i:320 * i + 96] for i in members[mm])
            want = co.msm_g1(pts, b"".join(r[i].to_bytes(32, "little") for i in members[mm]))
            assert same_g1(P[144 * g:144 * g + 144], want), (g, members[mm])
        # the ordinary call's scalars are the same ones
        assert m.batchVerifyParallel(cache, rec, RND) is True
        assert struct.unpack("<%dQ" % n, cache.fetch(0, 8 * n)) == r
    finally:
        cache.close()


def neg_fp(b):
    v = int.from_bytes(b, "little")
    return ((o.P - v) % o.P).to_bytes(48, "little")


def negated(rec320):
    """(PK, m, S) -> (-PK, m, -S): a valid set again (the images are Montgomery forms: -a is p - a there too)"""
    pk, mm, sg = rec320[:96], rec320[96:128], rec320[128:320]
    return pk[:48] + neg_fp(pk[48:96]) + mm + sg[:96] + neg_fp(sg[96:144]) + neg_fp(sg[144:192])


@pytest.mark.parametrize("coop", MODES)
def test_an_infinite_group_sum_is_the_factor_one(m, co, signer, coop):
    base = sign(m, signer, [0, 1, 1, 1])                      # one set over message 0, and a valid group of three over message 1
    pair = base[:320] + negated(base[:320])
    assert co.core_verify(pair[320:416], msg(0), pair[448:640])
    unrelated = base[:128] + base[320 + 128:640] + negated(base[:320])      # S replaced by another key's signature
    cache = m.BatchedBLSVerifierCache.init(max_sets=8, numThreads=4)
    cache.set_cooperative(coop)
    try:
        for label, rec, scalars, want in (("alone", pair, [5, 5], True),
                                          ("beside a valid group", pair + base[320:], [0x1234567890abcdef] * 2 + [3, 7, 11], True),
                                          ("unrelated signature", unrelated, [5, 5], False),
                                          ("unrelated signature beside a valid group", unrelated + base[320:], [9, 9, 3, 7, 11], False)):
            n = len(scalars)
            got = m.debugBatchVerifyByMessageScalars(cache, rec, scalars)
            gt, k = cache.fetch(4, 576), m.lastMessageGroups(cache)
            assert k == len(groups_of(rec)[0]) < n, label
            P = cache.fetch(2, 144 * k)
            assert int.from_bytes(P[96:144], "little") == 0, label               # group 0: the sum of [r]PK and [r](-PK)
            ref = m.debugBatchVerifyScalars(cache, rec, scalars)
            assert got is ref is want, label
            assert gt == cache.fetch(4, 576), label
            assert co.batch_verify_scalars(rec, scalars)[0] is want, label
        with pytest.raises(m.BlsGpuError):
            m.debugBatchVerifyByMessageScalars(cache, pair, [5, 0])
    finally:
        cache.close()


def test_slices_that_cut_groups(m, co, signer):
    n = 200
    rec = sign(m, signer, [i // 35 for i in range(n)])         # groups of 35: one straddles each of the boundaries 50, 100, 150
    bad = rec[:320 * 120 + 128] + rec[320 * 121 + 128:320 * 121 + 320] + rec[320 * 120 + 320:]
    small, big = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4), m.BatchedBLSVerifierCache.init(max_sets=256, numThreads=4)
    try:
        for label, r, want in (("valid", rec, True), ("one signature replaced", bad, False)):
            got_s, _ = both(m, small, r, RND, label + ", four slices", want=want)
            gt_s = small.fetch(4, 576)
            assert m.lastMessageGroups(small) == 2                                # the last slice: sets 150 .. 199 of groups 4 and 5
            got_b, k = both(m, big, r, RND, label + ", one slice", want=want)
            assert k == 6 and gt_s == big.fetch(4, 576), label
            assert oracle_verdict(co, r, RND, 4) is want
    finally:
        small.close()
        big.close()


def test_a_crowded_table_in_throughput_mode(m, co, signer):
    tags = list(range(1100)) + list(reversed(range(1100)))
    rec = sign(m, signer, tags)
    cache = m.BatchedBLSVerifierCache.init(max_sets=2200, numThreads=4)
    cache.set_cooperative(False)
    try:
        seen = []
        for run in range(2):
            got, k = both(m, cache, rec, RND, "run %d" % run, want=True)
            assert k == 1100
            seen.append(cache.fetch(4, 576))
        assert seen[0] == seen[1]
        assert oracle_verdict(co, rec, RND, 4) is True
    finally:
        cache.close()


@pytest.mark.parametrize("byte", [0, 31])
def test_messages_that_differ_in_one_byte_are_never_merged(m, co, signer, byte):
    base = bytearray(msg(77))
    def variant(v):
        b = bytearray(base)
        b[byte] = v
        return bytes(b)
    tags = [variant(v) for v in range(40) for _ in range(1 + v % 3)]
    n = len(tags)
    rec = sign(m, signer, tags)
    sibling = sign(m, signer, [variant((t[byte] + 1) % 40) for t in tags])       # the same keys over the neighbouring messages
    i = 33
    bad = rec[:320 * i + 128] + sibling[320 * i + 128:320 * i + 320] + rec[320 * i + 320:]
    cache = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4)
    try:
        got, k = both(m, cache, rec, RND, "valid", want=True)
        assert k == 40
        got, k = both(m, cache, bad, RND, "a signature over the message one byte away", want=False)
        assert k == 40
        assert oracle_verdict(co, rec, RND, 4) is True and oracle_verdict(co, bad, RND, 4) is False
    finally:
        cache.close()


def test_the_context_is_left_as_an_ordinary_call_leaves_it(m, signer):
    L = m.lib()
    n = 65
    rec = sign(m, signer, shape("interleaved", n))
    live0 = L.mi355_bls_debug_live_resources()
    fresh = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4)
    assert m.batchVerifyParallel(fresh, rec, RND) is True
    stages = lambda c: [c.fetch(s, size) for s, size in ((0, 8 * n), (1, 288 * n), (4, 576))] + [g2_jac_to_affine(c.fetch(3, 288))]
    want = stages(fresh)      # (stage 3 as a point, and no stage 5: the order of additions inside a bucket is free, and the Miller product before the final exponentiation follows it)
    fresh.close()
    assert L.mi355_bls_debug_live_resources() == live0
    used = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4)
    assert m.batchVerifyByMessage(used, rec, RND) is True
    assert m.lastMessageGroups(used) < n
    assert m.batchVerifyParallel(used, rec, RND) is True
    assert stages(used) == want
    used.close()
    assert L.mi355_bls_debug_live_resources() == live0
