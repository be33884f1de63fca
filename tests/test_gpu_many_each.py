"""Per-batch verdicts for many batches in one device pass (mi355_bls_batch_verify_many_each / _locate): verdict b and the 576-byte value b equal
those of a separate batchVerify call on batch b with the same random bytes (verdicts also the C restatement's), whatever the batch's
position, its neighbours, the context's capacity (the slices, the single-batch path of a batch that fits no slice), the executor or where
the records live.  The CPU half is tests/test_manyeach_plan.py, tests/test_manyeach_emu.py and tests/test_cabi_many_each.py."""
import ctypes
import hashlib

import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -3
SIZES = [100, 1, 2, 3, 0, 7, 8, 9, 64, 65, 257, 513]      # across the 8 / 64 / 512 item-level boundaries and the serial-to-parallel dispatch at 3
NT = 7
FORGED = {0: "message", 8: "infinity_key", 10: "swapped_signatures"}


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def rnd_of(i):
    return hashlib.sha256(b"many each" + bytes([i])).digest()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=2048, numThreads=NT)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data(m, cache):
    """the valid batches, the forged list and, per batch of either, what batchVerify on that batch alone says: (verdict, value) - made once"""
    import c_oracle as co
    valid = [co.make_batch(n, seed=1300 + 19 * i) if n else b"" for i, n in enumerate(SIZES)]
    forged = list(valid)
    b = bytearray(valid[0])
    b[320 * 41 + 96 + 5] ^= 0x10                                       # a flipped message bit
    forged[0] = bytes(b)
    b = bytearray(valid[8])
    b[320 * 17:320 * 17 + 96] = bytes(96)                              # an infinity key
    forged[8] = bytes(b)
    b = bytearray(valid[10])
    i, j = 3, 200                                                      # two signatures of one batch swapped
    b[320 * i + 128:320 * i + 320], b[320 * j + 128:320 * j + 320] = valid[10][320 * j + 128:320 * j + 320], valid[10][320 * i + 128:320 * i + 320]
    forged[10] = bytes(b)
    rnds = [rnd_of(i) for i in range(len(SIZES))]
    cache.set_cooperative(True)

    def alone(rec, rnd):
        if not rec:
            return False, bytes(576)
        ok = m.batchVerify(cache, rec, rnd)
        return ok, cache.fetch(4, 576)
    ref_valid = [alone(r, rd) for r, rd in zip(valid, rnds)]
    ref_forged = [ref_valid[i] if i not in FORGED else alone(forged[i], rnds[i]) for i in range(len(SIZES))]
    return {"valid": valid, "forged": forged, "rnds": rnds, "ref_valid": ref_valid, "ref_forged": ref_forged}


def check_values(got, ref, skip=()):
    v, gt = got
    assert v == [r[0] for r in ref]
    for i, (g, r) in enumerate(zip(gt, ref)):
        if i not in skip:
            assert g == r[1], i


@pytest.mark.parametrize("coop", [True, False])
def test_level_boundaries_and_dispatch(m, cache, data, coop):
    import c_oracle as co
    cache.set_cooperative(coop)
    try:
        want = [bool(n) for n in SIZES]
        got = m.batchVerifyManyEach(cache, data["valid"], data["rnds"])
        print("valid:", got)
        assert got == want
        assert got == [r[0] for r in data["ref_valid"]]
        bad = m.batchVerifyManyEach(cache, data["forged"], data["rnds"])
        print("forged:", bad)
        assert bad == [w and i not in FORGED for i, w in enumerate(want)]
        assert bad == [r[0] for r in data["ref_forged"]]
        for lst, res in ((data["valid"], got), (data["forged"], bad)):
            assert res == [co.batch_verify(b, rd, NT if len(b) // 320 >= 3 else 0) if b else False for b, rd in zip(lst, data["rnds"])]
    finally:
        cache.set_cooperative(True)


@pytest.mark.parametrize("coop", [True, False])
def test_values_equal_stage_4_of_the_batch_alone(m, cache, data, coop):
    cache.set_cooperative(coop)
    try:
        check_values(m.batchVerifyManyEachValues(cache, data["valid"], data["rnds"]), data["ref_valid"])
        check_values(m.batchVerifyManyEachValues(cache, data["forged"], data["rnds"]), data["ref_forged"], skip=(8,))      # the infinity-key batch: verdict only
    finally:
        cache.set_cooperative(True)


def test_a_batch_does_not_depend_on_position_neighbours_capacity_or_residence(m, cache, data):
    import torch
    forged, rnds, ref = data["forged"], data["rnds"], data["ref_forged"]
    k = len(SIZES)
    # another order, and a subset with other neighbours
    for order in ([11, 4, 10, 0, 1, 9, 8, 2, 3, 7, 6, 5], [10, 1, 8, 4, 3]):
        check_values(m.batchVerifyManyEachValues(cache, [forged[i] for i in order], [rnds[i] for i in order]), [ref[i] for i in order],
                     skip=[p for p, i in enumerate(order) if i == 8])
    # a context of 300 sets: the slices fall differently and the batch of 513 takes the single-batch path
    small = m.BatchedBLSVerifierCache.init(max_sets=300, numThreads=NT)
    try:
        check_values(m.batchVerifyManyEachValues(small, forged, rnds), ref, skip=(8,))
        assert m.batchVerifyManyEach(small, data["valid"], rnds) == [bool(n) for n in SIZES]
        d = torch.frombuffer(bytearray(b"".join(forged)), dtype=torch.uint8).cuda()
        assert m.batchVerifyManyEach_device(small, d.data_ptr(), SIZES, rnds) == [r[0] for r in ref]
    finally:
        small.close()
    # device-resident records
    d = torch.frombuffer(bytearray(b"".join(forged)), dtype=torch.uint8).cuda()
    assert m.batchVerifyManyEach_device(cache, d.data_ptr(), SIZES, rnds) == [r[0] for r in ref]
    assert m.batchVerifyManyLocate_device(cache, d.data_ptr(), SIZES, rnds) == [r[0] for r in ref]
    assert len(ref) == k


def test_equal_rnds_cannot_cancel_across_batches_in_one_pass(m):
    """The two-batch cancelling forgery of tests/test_gpu_many.py, with EQUAL random bytes: sig_A[i] + D in one batch, sig_B[i] - D in the other.
    A shared product would be one; every batch is a product of its own here, so one pass rejects both."""
    import bls12381_py as o
    import c_oracle as co
    n, nt, i = 8, 4, 5
    a = bytearray(co.make_batch(n, seed=4100))
    b = bytearray(co.make_batch(n, seed=4200))
    d = o.g2_from_blst_affine(bytes(a[320 * 2 + 128:320 * 2 + 320]))
    sa = o.g2_from_blst_affine(bytes(a[320 * i + 128:320 * i + 320]))
    sb = o.g2_from_blst_affine(bytes(b[320 * i + 128:320 * i + 320]))
    a[320 * i + 128:320 * i + 320] = o.g2_to_blst_affine(o.g2_add(sa, d))
    b[320 * i + 128:320 * i + 320] = o.g2_to_blst_affine(o.g2_add(sb, o.g2_neg(d)))
    a, b = bytes(a), bytes(b)
    rnd = rnd_of(77)
    c = m.BatchedBLSVerifierCache.init(max_sets=256, numThreads=nt)
    try:
        assert co.batch_verify(a, rnd, nt) is False and co.batch_verify(b, rnd, nt) is False
        p0 = m.batchVerifyManyEachPasses(c)
        assert m.batchVerifyManyEach(c, [a, b], [rnd, rnd]) == [False, False]
        assert m.batchVerifyManyEachPasses(c) == p0 + 1
        va, vb = co.make_batch(n, seed=4100), co.make_batch(n, seed=4200)
        assert m.batchVerifyManyEach(c, [va, vb, b""], [rnd, rnd, rnd]) == [True, True, False]
        assert m.batchVerifyManyLocate(c, [a, b], [rnd, rnd]) == [False, False]       # no merged pass with equal rnds: the per-batch pass answers
    finally:
        c.close()


def test_locate_makes_the_per_batch_pass_only_when_the_merged_pass_fails(m, cache, data):
    valid, forged, rnds = data["valid"], data["forged"], data["rnds"]
    p0 = m.batchVerifyManyEachPasses(cache)
    assert m.batchVerifyManyLocate(cache, valid, rnds) == [bool(n) for n in SIZES]
    assert m.batchVerifyManyEachPasses(cache) == p0                       # the merged pass passed: no per-batch pass ran
    got = m.batchVerifyManyLocate(cache, forged, rnds)
    assert m.batchVerifyManyEachPasses(cache) == p0 + 1
    assert got == m.batchVerifyMany(cache, forged, rnds)
    assert got == [r[0] for r in data["ref_forged"]]


def test_degenerate_calls(m, cache, data):
    import torch
    L, sz = m.lib(), ctypes.c_size_t
    assert m.batchVerifyManyEach(cache, [], []) == [] and m.batchVerifyManyLocate(cache, [], []) == []
    assert m.batchVerifyManyEachValues(cache, [], []) == ([], [])
    out = ctypes.create_string_buffer(b"\xaa" * 3, 3)
    rnds = b"".join(data["rnds"][:3])
    for fn in (L.mi355_bls_batch_verify_many_each, L.mi355_bls_batch_verify_many_locate):
        assert fn(cache._h, b"\0", (sz * 1)(0), rnds, 0, out) == 0                        # k == 0
        out.raw = b"\xaa" * 3
        assert fn(cache._h, b"\0", (sz * 3)(0, 0, 0), rnds, 3, out) == 0 and out.raw == bytes(3)      # all batches empty
    assert m.batchVerifyManyEach(cache, [b"", b""], data["rnds"][:2]) == [False, False]
    # a context with a submitted batch pending
    rec = data["valid"][3]
    d = torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()
    cache.submit_device(d.data_ptr(), len(rec) // 320, data["rnds"][3])
    try:
        one = (sz * 1)(len(rec) // 320)
        assert L.mi355_bls_batch_verify_many_each(cache._h, rec, one, data["rnds"][3], 1, out) == ERR_ARG
        assert L.mi355_bls_batch_verify_many_locate(cache._h, rec, one, data["rnds"][3], 1, out) == ERR_ARG
        assert L.mi355_bls_batch_verify_many_each_device(cache._h, d.data_ptr(), one, data["rnds"][3], 1, out, None) == ERR_ARG
    finally:
        assert cache.wait() is True


def test_resources_return_with_the_context(m, data):
    L = m.lib()
    live0 = L.mi355_bls_debug_live_resources()
    c = m.BatchedBLSVerifierCache.init(max_sets=128, numThreads=NT)
    assert m.batchVerifyManyEachValues(c, data["forged"][:4], data["rnds"][:4])[0] == [False, True, True, True]
    assert L.mi355_bls_debug_live_resources() > live0
    c.close()
    assert L.mi355_bls_debug_live_resources() == live0
