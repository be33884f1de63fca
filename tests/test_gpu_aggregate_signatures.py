"""Per-group signature aggregation on the device (mi355_bls_aggregate_signature_sets), signature serialisation (mi355_bls_compress_signatures)
and signature-only decoding (mi355_bls_deserialize_signatures): aggregateAll on signatures (blst_min_pubkey_sig_core.nim:142-211) for every
group in one pass, finished and serialised.  Images, wire forms and status bytes are held bit-exact to tests/golden/aggregate_signatures.json
and to the C restatement; a group's outputs must not depend on its position or on how it is addressed.  The CPU half is
tests/test_aggsigs_emu.py."""
import ctypes
import hashlib
import random

import pytest

import aggsigs_cases as ac
import deser_cases as dc

pytestmark = pytest.mark.gpu

ERR_ARG = -3


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
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def test_fixture_bit_exact_in_both_modes_and_forms(m):
    import torch
    fx = ac.fixture()
    tab = ac.table_of(fx)
    sigs, offsets, w192, w96, status = ac.contiguous_inputs(fx)
    lists = [b"".join(tab[i] for i in g["members"]) for g in fx["groups"]]
    k = len(lists)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        for coop in (True, False):
            c.set_cooperative(coop)
            assert m.aggregateSignatureSets(c, lists) == (False, w192, w96, status), coop
            assert m.aggregateSignatureSets(c, (sigs, None, offsets)) == (False, w192, w96, status), coop
            assert m.aggregateSignatureSets(c, lists, want96=False) == (False, w192, None, status), coop          # either output pointer NULL
            assert m.aggregateSignatureSets(c, lists, want192=False) == (False, None, w96, status), coop
            for bad in (False, True):
                table, idx, ioffs, i192, i96, ist = ac.indexed_inputs(bad, fx)
                assert m.aggregateSignatureSets(c, (table, idx, ioffs)) == (False, i192, i96, ist), (coop, bad)
                assert (3 in ist) == bad
            good = status.index(1)                                                                                # the groups in front of the empty one
            assert m.aggregateSignatureSets(c, lists[:good]) == (True, w192[:192 * good], w96[:96 * good], bytes(good)), coop
            # the device forms: everything resident, offsets on the host
            d_s = dev(sigs)
            for want192, want96 in ((True, True), (True, False), (False, True)):
                o192 = torch.full((192 * k,), 0x5a, dtype=torch.uint8, device="cuda")
                o96 = torch.full((96 * k,), 0x5a, dtype=torch.uint8, device="cuda")
                ok, st = m.aggregateSignatureSets_device(c, d_s.data_ptr(), len(sigs) // 192, None, offsets, o192.data_ptr() if want192 else None,
                                                         o96.data_ptr() if want96 else None)
                assert (ok, st) == (False, status)
                assert host(o192) == (w192 if want192 else b"\x5a" * (192 * k)) and host(o96) == (w96 if want96 else b"\x5a" * (96 * k)), (coop, want192, want96)
            table, idx, ioffs, i192, i96, ist = ac.indexed_inputs(True, fx)
            d_t, d_i = dev(table), torch.tensor(idx, dtype=torch.int32).cuda()
            o192, o96 = torch.zeros(192 * k, dtype=torch.uint8, device="cuda"), torch.zeros(96 * k, dtype=torch.uint8, device="cuda")
            ok, st = m.aggregateSignatureSets_device(c, d_t.data_ptr(), len(table) // 192, d_i.data_ptr(), ioffs, o192.data_ptr(), o96.data_ptr())
            assert (ok, st, host(o192), host(o96)) == (False, ist, i192, i96), coop
    finally:
        c.close()


def test_argument_errors_and_no_groups(m, cache):
    L = m.lib()
    sigs, offsets, w192, _, _ = ac.contiguous_inputs()
    sz = ctypes.c_size_t
    out, st = ctypes.create_string_buffer(b"\x5a" * 384, 384), ctypes.create_string_buffer(b"\x5a" * 2, 2)
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 3, None, (sz * 3)(0, 2, 1), 2, out, None, st) == ERR_ARG          # decreasing offsets
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 1, None, (sz * 2)(0, 2), 1, out, None, st) == ERR_ARG             # offsets[k] > n_table without idx
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 3, None, (sz * 2)(0, 2), 1, None, None, st) == ERR_ARG            # both outputs NULL
    assert L.mi355_bls_aggregate_signature_sets(cache._h, None, 3, None, (sz * 2)(0, 2), 1, out, None, st) == ERR_ARG
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 3, None, None, 1, out, None, st) == ERR_ARG
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 3, None, (sz * 2)(0, 2), 1, out, None, None) == ERR_ARG
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 3, None, (sz * 1)(0), 0, out, out, st) == 0                      # k == 0: 0, nothing written
    assert out.raw == b"\x5a" * 384 and st.raw == b"\x5a" * 2
    assert L.mi355_bls_deserialize_signatures(cache._h, bytes(96), 1, dc.PK_UNCOMPRESSED, out, st) == ERR_ARG
    assert L.mi355_bls_deserialize_signatures(cache._h, bytes(96), 1, 8, out, st) == ERR_ARG
    iarr = (ctypes.c_uint32 * 2)(0, 0)
    assert L.mi355_bls_aggregate_signature_sets(cache._h, sigs, 1, iarr, (sz * 2)(0, 2), 1, out, None, st) == 1                   # the same offsets through indices
    assert st.raw[:1] == b"\x00" and out.raw[:192] != bytes(192)


@pytest.fixture(scope="module")
def drawn():
    """200 groups of 1 .. 2 C^2 + 3 signatures drawn (with repeats between groups) from 512 signatures of the C restatement's generator;
    -> (pool, [member indices], images by g2_sum, wire forms by compress_sets); computed once, never changed"""
    import c_oracle as co
    C = ac.fixture()["C"]
    rec = co.make_batch(512, seed=9090)
    pool = [rec[320 * i + 128:320 * i + 320] for i in range(512)]
    rng = random.Random(20261018)
    groups = [[rng.randrange(512) for _ in range(rng.randint(1, 2 * C * C + 3))] for _ in range(200)]
    groups[0], groups[1], groups[2] = groups[0][:1], (groups[1] * 200)[:2 * C * C + 3], (groups[2] * 200)[:C * C]      # the ends of the range, and a full C x C
    sums = [co.g2_sum(b"".join(pool[i] for i in g)) for g in groups]
    wire = co.compress_sets(b"".join(bytes(128) + s for s in sums))[2]
    return pool, groups, b"".join(sums), wire


def test_random_groups_against_c_oracle_any_position_any_addressing(m, cache, drawn):
    pool, groups, w192, w96 = drawn
    k = len(groups)
    lists = [b"".join(pool[i] for i in g) for g in groups]
    assert m.aggregateSignatureSets(cache, lists) == (True, w192, w96, bytes(k))                                  # contiguous
    idx, offs = [i for g in groups for i in g], [0]
    for g in groups:
        offs.append(offs[-1] + len(g))
    assert m.aggregateSignatureSets(cache, (b"".join(pool), idx, offs)) == (True, w192, w96, bytes(k))            # indexed into the pool
    rev = lambda b, u: b"".join(b[u * i:u * i + u] for i in reversed(range(k)))                                   # noqa: E731
    assert m.aggregateSignatureSets(cache, lists[::-1]) == (True, rev(w192, 192), rev(w96, 96), bytes(k))         # reversed group order
    some = [7, 150, 3, 199, 0, 1, 2]
    ok, o192, o96, st = m.aggregateSignatureSets(cache, [lists[i] for i in some])                                 # other neighbours
    assert (ok, st) == (True, bytes(len(some)))
    assert o192 == b"".join(w192[192 * i:192 * i + 192] for i in some) and o96 == b"".join(w96[96 * i:96 * i + 96] for i in some)
    assert m.compressSignatures(cache, w192) == [w96[96 * i:96 * i + 96] for i in range(k)]


@pytest.fixture(scope="module")
def adversarial():
    """the adversarial signature encodings per wire form, and what the C restatement's deserialize_sets_ex makes of them beside a fixed valid
    key: -> {unc: (names, wire bytes, {known: (all ok, images, status bytes)})}; computed once, never changed"""
    import c_oracle as co
    pk48 = co.compress_sets(co.make_batch(1, seed=7))[0]
    out = {}
    for unc in (False, True):
        encs = ac.adversarial_signatures(unc)
        n, sg = len(encs), b"".join(b for _, b in encs)
        res = {}
        for known in (False, True):
            ok, rec, st = co.deserialize_sets_ex(pk48 * n, bytes(32 * n), sg, (dc.SIG_UNCOMPRESSED if unc else 0) | (dc.KNOWN_ON_CURVE if known else 0))
            res[known] = (ok, b"".join(rec[320 * i + 128:320 * i + 320] for i in range(n)), st)
        out[unc] = ([nm for nm, _ in encs], sg, res)
    return out


@pytest.mark.parametrize("unc", (False, True))
@pytest.mark.parametrize("known", (False, True))
def test_deserialize_signatures_on_adversarial_encodings(m, cache, adversarial, unc, known):
    import torch
    names, sg, res = adversarial[unc]
    ok_c, img_c, st_c = res[known]
    n = len(names)
    assert n >= 40 and set(st_c) <= {0, 4, 5} and (known or {0, 4, 5} <= set(st_c)) and not ok_c
    ok, img, st = m.deserializeSignatures(cache, sg, sig_uncompressed=unc, known_on_curve=known)
    bad = [(names[i], st[i], st_c[i]) for i in range(n) if st[i] != st_c[i] or img[192 * i:192 * i + 192] != img_c[192 * i:192 * i + 192]]
    assert not bad, bad
    assert ok is False
    for i in range(n):
        assert (st[i] != 0) <= (img[192 * i:192 * i + 192] == bytes(192)), names[i]                               # zeroed on failure
    d_in, d_out = dev(sg), torch.full((192 * n,), 0x5a, dtype=torch.uint8, device="cuda")
    assert m.deserializeSignatures_device(cache, d_in.data_ptr(), n, d_out.data_ptr(), sig_uncompressed=unc, known_on_curve=known) == (False, st_c)
    assert host(d_out) == img_c
    good = [i for i in range(n) if st_c[i] == 0]
    unit = 192 if unc else 96
    ok, img, st = m.deserializeSignatures(cache, b"".join(sg[unit * i:unit * i + unit] for i in good), sig_uncompressed=unc, known_on_curve=known)
    assert (ok, st) == (True, bytes(len(good))) and img == b"".join(img_c[192 * i:192 * i + 192] for i in good)
    assert any(names[i] == "g2_inf" for i in good)                                                                # the infinity signature is allowed


def test_compress_signatures_on_adversarial_points_and_round_trip(m, cache, adversarial):
    import torch
    import bls12381_py as o
    import c_oracle as co
    imgs, names = [], []
    for unc in (False, True):
        nms, _, res = adversarial[unc]
        _, img, st = res[True]                                                                                     # every encoding that decodes: any subgroup
        for i, nm in enumerate(nms):
            if st[i] == 0 and img[192 * i:192 * i + 192] not in imgs:
                imgs.append(img[192 * i:192 * i + 192])
                names.append(nm)
    assert any("c0zero" in x for x in names) and any("c1zero" in x for x in names) and any("ord13" in x for x in names) and "g2_inf" in names
    n = len(imgs)
    want = co.compress_sets(b"".join(bytes(128) + b for b in imgs))[2]
    assert [want[96 * i:96 * i + 96] for i in range(n)] == [o.g2_compress(o.g2_from_blst_affine(b)) for b in imgs]
    got = m.compressSignatures(cache, imgs)
    assert [(names[i], got[i]) for i in range(n) if got[i] != want[96 * i:96 * i + 96]] == []
    d_in, d_out = dev(b"".join(imgs)), torch.zeros(96 * n, dtype=torch.uint8, device="cuda")
    m.compressSignatures_device(cache, d_in.data_ptr(), n, d_out.data_ptr())
    assert host(d_out) == want
    assert m.deserializeSignatures(cache, want, known_on_curve=True) == (True, b"".join(imgs), bytes(n))          # the round trip returns the images


def test_wire_signatures_to_verified_aggregates_on_the_device(m, cache):
    """8 committees of 3 .. 20 members who each sign their committee's message: wire signatures are decoded, aggregated per committee and
    verified against the committee keys without leaving the device"""
    import torch
    import c_oracle as co
    rng = random.Random(8)
    sizes = [3, 20] + [rng.randint(3, 20) for _ in range(6)]
    keys, offs, msgs, sigs = [], [0], [], []
    for g, n in enumerate(sizes):
        msg = hashlib.sha256(b"committee %d" % g).digest()
        for j in range(n):
            sk = int.from_bytes(hashlib.sha256(b"member %d %d" % (g, j)).digest(), "little") >> 3 | 1
            keys.append(co.sk_to_pk(sk))
            sigs.append(co.sign(sk, msg))
        msgs.append(msg)
        offs.append(offs[-1] + n)
    n_all, k = offs[-1], len(sizes)
    rnd = hashlib.sha256(b"aggregate signatures rnd").digest()
    d_keys, d_msgs = dev(b"".join(keys)), dev(b"".join(msgs))
    for swap in (False, True):
        s = list(sigs)
        if swap:
            s[offs[3] + 1], s[offs[5]] = s[offs[5]], s[offs[3] + 1]                                               # two members of different committees
        wire = co.compress_sets(b"".join(bytes(128) + x for x in s))[2]
        d_wire = dev(wire)
        d_sig = torch.zeros(192 * n_all, dtype=torch.uint8, device="cuda")
        assert m.deserializeSignatures_device(cache, d_wire.data_ptr(), n_all, d_sig.data_ptr()) == (True, bytes(n_all))
        d_agg, d_agg96 = torch.zeros(192 * k, dtype=torch.uint8, device="cuda"), torch.zeros(96 * k, dtype=torch.uint8, device="cuda")
        assert m.aggregateSignatureSets_device(cache, d_sig.data_ptr(), n_all, None, offs, d_agg.data_ptr(), d_agg96.data_ptr()) == (True, bytes(k))
        got = m.batchFastAggregateVerify_device(cache, d_keys.data_ptr(), n_all, None, offs, d_msgs.data_ptr(), d_agg.data_ptr(), rnd)
        assert got is (not swap)
        verdicts = m.fastAggregateVerifyEach_device(cache, d_keys.data_ptr(), n_all, None, offs, d_msgs.data_ptr(), d_agg.data_ptr())
        assert verdicts == [not (swap and g in (3, 5)) for g in range(k)]
        if not swap:
            agg = host(d_agg)
            assert agg == b"".join(co.g2_sum(b"".join(sigs[offs[g]:offs[g + 1]])) for g in range(k))
            assert host(d_agg96) == co.compress_sets(b"".join(bytes(128) + agg[192 * g:192 * g + 192] for g in range(k)))[2]


def test_resources_return_when_the_context_goes(m):
    L = m.lib()
    sigs, offsets, w192, w96, status = ac.contiguous_inputs()
    before = L.mi355_bls_debug_live_resources()
    c = m.BatchedBLSVerifierCache.init(max_sets=16, numThreads=4)
    assert L.mi355_bls_debug_live_resources() > before
    assert m.aggregateSignatureSets(c, (sigs, None, offsets)) == (False, w192, w96, status)
    k = len(status)
    assert m.compressSignatures(c, w192) == [w96[96 * i:96 * i + 96] for i in range(k)]                           # more than max_sets: the staging grows
    assert m.deserializeSignatures(c, w96) == (True, w192, bytes(k))
    c.close()
    assert L.mi355_bls_debug_live_resources() == before
