"""Batched aggregateVerify on the device (mi355_bls_aggregate_verify_each): aggregateVerify (bls_sig_min_pubkey.nim:127-199) for k groups of
(key, message) pairs under one aggregate signature each, in one pass.  Verdicts and 576-byte values are held bit-exact to
tests/golden/aggregate_verify_each.json, the verdicts to the C restatement and to the one-shot mi355_bls_aggregate_verify; a group's verdict and
value must not depend on its position, on the slices it falls into, on the executor or on how it is addressed.  The CPU half is
tests/test_aggveach_emu.py and tests/test_aggveach_plan.py."""
import ctypes
import hashlib
import random

import pytest

from util import golden

pytestmark = pytest.mark.gpu

ERR_ARG = -3
C = 8                                     # csrc/plan.hpp AGGV_C (tests/test_aggveach_plan.py reads it from the header's own library)
N_POOL = 1500


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=4096, numThreads=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(m, cache):
    """N_POOL signed sets with distinct keys and messages, made once -> [(pk96, msg32, sig192)]"""
    sks = b"".join(hashlib.sha256(b"aggregate_verify_each sk %d" % i).digest()[:31] + b"\0" for i in range(N_POOL))
    msgs = b"".join(hashlib.sha256(b"aggregate_verify_each msg %d" % i).digest() for i in range(N_POOL))
    ok, rec, _ = m.signSets(cache, sks, msgs)
    assert ok
    return [(rec[320 * i:320 * i + 96], rec[320 * i + 96:320 * i + 128], rec[320 * i + 128:320 * i + 320]) for i in range(N_POOL)]


class Group:
    def __init__(self, pks, msgs, sig, kind="valid"):
        self.pks, self.msgs, self.sig, self.kind = list(pks), list(msgs), sig, kind


def make_groups(m, cache, pool, members):
    """members: [[pool indices]] -> valid groups, their signatures aggregated on the device in one call"""
    idx, offs = [], [0]
    for g in members:
        idx += g
        offs.append(len(idx))
    _, s192, _, st = m.aggregateSignatureSets(cache, (b"".join(p[2] for p in pool), idx, offs), want96=False)
    assert not any(st)
    return [Group([pool[i][0] for i in g], [pool[i][1] for i in g], s192[192 * j:192 * j + 192]) for j, g in enumerate(members)]


def corrupt(g, kind, rng, pool):
    j = rng.randrange(len(g.pks))
    if kind == "swapped_messages" and len(g.pks) < 2:
        kind = "wrong_message"
    if kind == "wrong_message":
        g.msgs[j] = hashlib.sha256(g.msgs[j]).digest()
    elif kind == "missing_member":
        g.sig = pool[-1][2] if len(g.pks) == 1 else g.sig                 # a group of one: another set's signature
        if len(g.pks) > 1:
            g.pks.pop(j), g.msgs.pop(j)                                   # the signature aggregates one key more than the group lists
    elif kind == "swapped_messages":
        i = (j + 1) % len(g.pks)
        g.msgs[i], g.msgs[j] = g.msgs[j], g.msgs[i]
    elif kind == "infinity_public_key":
        g.pks[j] = bytes(96)
    elif kind == "infinity_signature":
        g.sig = bytes(192)
    g.kind = kind
    return g


def call(m, c, groups, values=True):
    keys, msgs, sigs = [b"".join(g.pks) for g in groups], b"".join(b"".join(g.msgs) for g in groups), b"".join(g.sig for g in groups)
    if values:
        return m.aggregateVerifyEachValues(c, keys, msgs, sigs)
    return m.aggregateVerifyEach(c, keys, msgs, sigs), None


def fixture_groups():
    out = []
    for g in golden("aggregate_verify_each")["groups"]:
        pk, ms = bytes.fromhex(g["pks"]), bytes.fromhex(g["msgs"])
        t = len(pk) // 96
        out.append(Group([pk[96 * j:96 * j + 96] for j in range(t)], [ms[32 * j:32 * j + 32] for j in range(t)], bytes.fromhex(g["sig"]), g["kind"]))
    return out


def raw_call(m, c, groups, out):
    L, sz = m.lib(), ctypes.c_size_t
    offs = [0]
    for g in groups:
        offs.append(offs[-1] + len(g.pks))
    keys = b"".join(b"".join(g.pks) for g in groups) or b"\0"
    return L.mi355_bls_aggregate_verify_each(c._h, keys, offs[-1], None, (sz * len(offs))(*offs), len(groups),
                                             b"".join(b"".join(g.msgs) for g in groups) or b"\0", b"".join(g.sig for g in groups) or b"\0", out)


def test_fixture_bit_exact_in_both_modes(m, small):
    fx, gs = golden("aggregate_verify_each")["groups"], fixture_groups()
    try:
        for coop in (True, False):
            small.set_cooperative(coop)
            v, gt = call(m, small, gs)
            assert v == [bool(g["verdict"]) for g in fx], coop
            assert [x.hex() for x in gt] == [g["gt"] for g in fx], coop
            out = ctypes.create_string_buffer(b"\x5a" * len(gs), len(gs))
            assert raw_call(m, small, gs, out) == 0 and out.raw == bytes(g["verdict"] for g in fx)         # a failing group: 0
            good = [g for g, f in zip(gs, fx) if f["verdict"]]
            assert len(good) >= 7 and raw_call(m, small, good, out) == 1 and out.raw[:len(good)] == b"\1" * len(good)
            out = ctypes.create_string_buffer(b"\x5a" * 4, 4)
            assert raw_call(m, small, [], out) == 0 and out.raw == b"\x5a" * 4                                # k == 0: 0, nothing written
    finally:
        small.set_cooperative(True)


SIZES = [1, 2, C - 1, C, C + 1, C * C + 1, 63, 64, 65]
KINDS = ["wrong_message", "missing_member", "swapped_messages", "infinity_public_key", "infinity_signature"]


@pytest.fixture(scope="module")
def sized(m, cache, pool):
    """three groups of every size of SIZES in a seeded order, about a fifth of them corrupted by a seeded choice of KINDS; the verdicts of the
    C restatement, computed once -> (groups, expected verdicts)"""
    import c_oracle as co
    rng = random.Random(4711)
    sizes = SIZES * 3
    rng.shuffle(sizes)
    members, at = [], 0
    for n in sizes:
        members.append([(at + j) % (N_POOL - 1) for j in range(n)])
        at += n
    gs = make_groups(m, cache, pool, members)
    bad = sorted(rng.sample(range(len(gs)), 6))
    for n, i in enumerate(bad):
        corrupt(gs[i], KINDS[n % len(KINDS)], rng, pool)
    want = [co.aggregate_verify(b"".join(g.pks), g.msgs, g.sig) for g in gs]
    return gs, want


def test_sizes_against_the_c_restatement_and_the_one_shot_call(m, cache, sized):
    gs, want = sized
    v, _ = call(m, cache, gs, values=False)
    assert v == want
    assert want.count(False) == 6 and [g.kind != "valid" for g in gs] == [not w for w in want]      # not all zero, not all one
    rng = random.Random(12)
    for i in rng.sample(range(len(gs)), 20):
        assert m.aggregateVerify(cache, gs[i].pks, gs[i].msgs, gs[i].sig) == v[i], (i, gs[i].kind)


def test_a_group_does_not_depend_on_its_neighbours(m, cache, pool, sized):
    gs, want = sized
    v0, gt0 = call(m, cache, gs)
    assert v0 == want
    rng = random.Random(99)
    others = [Group([pool[i][0]], [pool[i][1]], pool[(i + (i % 7 == 0)) % N_POOL][2]) for i in rng.sample(range(N_POOL), 500)]      # every seventh fails
    order = list(range(len(gs)))
    rng.shuffle(order)
    slots = sorted(rng.sample(range(len(gs) + 500), len(gs)))
    mixed, where = list(others), {}
    for s, i in zip(slots, order):
        mixed.insert(s, gs[i])
    for p, g in enumerate(mixed):
        where[id(g)] = p
    v, gt = call(m, cache, mixed)
    for i, g in enumerate(gs):
        assert (v[where[id(g)]], gt[where[id(g)]]) == (v0[i], gt0[i]), (i, g.kind)


def test_slices_and_the_carry(m, small, pool):
    members = [[0, 1, 2], [3], list(range(10, 160)), [200, 201], list(range(300, 364)), [400], list(range(401, 406))]
    big = m.BatchedBLSVerifierCache.init(max_sets=65536, numThreads=4)
    try:
        for wrong in (False, True):
            gs = make_groups(m, small, pool, members)
            if wrong:
                gs[2].msgs[140] = hashlib.sha256(b"a wrong message in the third part").digest()
            for coop in (True, False):
                small.set_cooperative(coop), big.set_cooperative(coop)
                v, gt = call(m, small, gs)
                assert v == [not (wrong and i == 2) for i in range(len(gs))], (wrong, coop)
                assert (v, gt) == call(m, big, gs), (wrong, coop)
    finally:
        small.set_cooperative(True)
        big.close()


def test_executors_agree(m, cache, pool):
    rng = random.Random(300)
    members = [[rng.randrange(N_POOL) for _ in range(rng.randint(1, 8))] for _ in range(300)]
    gs = make_groups(m, cache, pool, members)
    for i in rng.sample(range(300), 30):
        corrupt(gs[i], rng.choice(KINDS), rng, pool)
    try:
        cache.set_cooperative(True)
        a = call(m, cache, gs)
        cache.set_cooperative(False)
        b = call(m, cache, gs)
    finally:
        cache.set_cooperative(True)
    assert a == b and 0 < a[0].count(False) <= 30


def test_groups_of_one_equal_verify_each(m, cache, pool):
    sets = [list(p) for p in pool[:400]]
    for i in range(0, 400, 9):
        sets[i][2] = pool[i + 1][2]                                        # another set's signature
    sets[5][0], sets[6][2] = bytes(96), bytes(192)
    rec = b"".join(b"".join(s) for s in sets)
    want_v, want_gt = m.verifyEachValues(cache, rec)
    assert 300 < want_v.count(True) < 400
    assert call(m, cache, [Group([s[0]], [s[1]], s[2]) for s in sets]) == (want_v, want_gt)


def test_addressing(m, cache, pool):
    import torch
    # indices with repeats and one out of range: that group is 0, the others are unaffected
    table = b"".join(p[0] for p in pool[:64])
    members = [[3, 3, 5], [7], [], [9, 10, 9, 11], [63, 0]]
    idx, offs = [], [0]
    for g in members:
        idx += g
        offs.append(len(idx))
    _, s192, _, _ = m.aggregateSignatureSets(cache, (b"".join(p[2] for p in pool[:64]), idx, offs), want96=False)
    msgs = b"".join(pool[i][1] for i in idx)
    assert m.aggregateVerifyEach(cache, (table, idx, offs), msgs, s192) == [True, True, False, True, True]
    bad = list(idx)
    bad[3] = 64                                                            # group 1's only key: one past the table
    assert m.aggregateVerifyEach(cache, (table, bad, offs), msgs, s192) == [True, False, False, True, True]
    bad[3] = 0xffffffff
    assert m.aggregateVerifyEach(cache, (table, bad, offs), msgs, s192) == [True, False, False, True, True]
    # empty groups at the start, in the middle and at the end; by position into the table itself
    lens = [0, 0, 2, 0, 3, 1, 0]
    offs2 = [0]
    for n in lens:
        offs2.append(offs2[-1] + n)
    _, s2, _, st = m.aggregateSignatureSets(cache, (b"".join(p[2] for p in pool[:6]), None, offs2), want96=False)
    v, gt = m.aggregateVerifyEachValues(cache, (table, None, offs2), b"".join(p[1] for p in pool[:6]), s2)
    assert v == [n > 0 for n in lens] and all((x == bytes(576)) == (n == 0) for x, n in zip(gt, lens))
    # the device form, fed by aggregateSignatureSets_device's output buffer
    d_keys = torch.frombuffer(bytearray(table), dtype=torch.uint8).cuda()
    d_sigs = torch.frombuffer(bytearray(b"".join(p[2] for p in pool[:64])), dtype=torch.uint8).cuda()
    d_idx = torch.tensor(idx, dtype=torch.int32).cuda()
    d_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).cuda()
    d_out = torch.zeros(192 * len(members), dtype=torch.uint8, device="cuda")
    m.aggregateSignatureSets_device(cache, d_sigs.data_ptr(), 64, d_idx.data_ptr(), offs, d_out.data_ptr(), None)
    got = m.aggregateVerifyEach_device(cache, d_keys.data_ptr(), 64, d_idx.data_ptr(), offs, d_msgs.data_ptr(), d_out.data_ptr())
    assert got == [True, True, False, True, True]
    torch.cuda.synchronize()


def test_argument_errors(m, cache, pool):
    L, sz = m.lib(), ctypes.c_size_t
    keys, msgs, sigs = b"".join(p[0] for p in pool[:3]), b"".join(p[1] for p in pool[:3]), pool[0][2] + pool[1][2]
    out = ctypes.create_string_buffer(b"\x5a" * 2, 2)
    assert L.mi355_bls_aggregate_verify_each(cache._h, keys, 3, None, (sz * 3)(0, 2, 1), 2, msgs, sigs, out) == ERR_ARG       # decreasing offsets
    assert L.mi355_bls_aggregate_verify_each(cache._h, keys, 3, None, (sz * 3)(0, 1, 3), 2, msgs, sigs, None) == ERR_ARG      # NULL output
    assert L.mi355_bls_aggregate_verify_each(cache._h, keys, 2, None, (sz * 3)(0, 1, 3), 2, msgs, sigs, out) == ERR_ARG       # offsets[k] > n_table without idx
    assert L.mi355_bls_debug_aggregate_verify_each_gt(cache._h, keys, 3, None, (sz * 3)(0, 1, 3), 2, msgs, sigs, out, None) == ERR_ARG
    assert out.raw == b"\x5a" * 2
    assert L.mi355_bls_aggregate_verify_each(cache._h, keys, 3, None, (sz * 3)(0, 1, 2), 2, msgs, sigs, out) == 1 and out.raw == b"\1\1"
