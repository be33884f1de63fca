"""Blocking batch verification on a latency-mode context (the default) at both sides of every size where a stage hands over to another
executor (tests/util.py latency_plan: cofactor clearing at 4 S and 11 S, the side streams at 16 S, the tuple pairs' Miller lines at 4 S and
18 S, the SSWU map at 32 S; S = 4 x CU count): verdict, GT value, aggregated signature, blinding scalars and sampled H(m_i) / [r_i]PK_i against
the C restatement's results in tests/golden/latency_handover.json (tests/golden/gen_latency_handover.py), a defective batch per size, and
one context walked down and up the sizes (state a larger call leaves behind for a smaller one)."""
import hashlib

import pytest

import bls12381_py as o
from util import apply_defect, g1_jac_to_affine, g2_jac_to_affine, golden, latency_hand_overs, latency_plan

pytestmark = pytest.mark.gpu

FX = golden("latency_handover")
SIZES = [c["n"] for c in FX["cases"]]
RND = bytes.fromhex(FX["rnd"])
NT = FX["num_threads"]


def _case(n):
    return [c for c in FX["cases"] if c["n"] == n][0]


def _slots():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _check_plan():
    """The fixture's sizes must sit on both sides of every hand-over of THIS device's plan; a device with another CU count (a partition)
    would otherwise pass these tests away from the boundaries."""
    S = _slots()
    for stage, t in latency_hand_overs(S):
        assert t in SIZES and t + 1 in SIZES, ("the fixture's sizes miss the %s hand-over at %d sets for %d CUs (S = %d): regenerate "
                                               "tests/golden/latency_handover.json for this device" % (stage, t, S // 4, S), SIZES)
        assert latency_plan(t, S)[stage] != latency_plan(t + 1, S)[stage], (stage, t, S)


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def recs(m):
    """The fixture's 32 769 records rebuilt by the device signer from the generator's keys and messages (tests/test_gpu_sign.py pins the
    signer byte-exact): (device tensor, host bytes); every case's prefix checked against its digest."""
    import torch
    import bench
    _check_plan()
    N, seed = FX["records"], FX["seed"]
    sks = []
    for i in range(N):
        sk = bytearray(hashlib.sha256(b"sk" + (seed + i).to_bytes(8, "little")).digest())
        sk[31] &= 0x3f
        sk[0] |= 1
        sks.append(int.from_bytes(sk, "little"))
    msgs = [hashlib.sha256(b"msg" + str(i).encode()).digest() for i in range(N)]
    gen = m.BatchedBLSVerifierCache.init(max_sets=N)
    d = bench.sign_records(m, gen, torch.device("cuda", 0), range(N), sks=sks, msgs=msgs)
    gen.close()
    host = bytes(d.cpu().numpy())
    for c in FX["cases"]:
        assert hashlib.sha256(host[:320 * c["n"]]).hexdigest() == c["records_sha256"], ("records differ from the generator's", c["n"])
    return d, host


def test_sizes_sit_on_every_hand_over():
    _check_plan()


@pytest.mark.parametrize("n", SIZES)
def test_hand_over_size(m, recs, n):
    """A context of exactly n sets (the extra pairs in the last columns of the line store): the valid batch stage by stage, then the defective one."""
    _, host = recs
    c = _case(n)
    v = c["valid"]
    cache = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=NT)
    assert m.batchVerify(cache, host[:320 * n], RND) is v["verdict"] is True
    assert cache.fetch(4, 576).hex() == v["gt"]
    assert o.g2_to_blst_affine(g2_jac_to_affine(cache.fetch(3, 288))).hex() == v["aggsig"]
    assert hashlib.sha256(cache.fetch(0, 8 * n)).hexdigest() == v["r_sha256"]
    H, P = cache.fetch(1, 288 * n), cache.fetch(2, 144 * n)
    for i, h, p in v["samples"]:
        assert o.g2_to_blst_affine(g2_jac_to_affine(H[288 * i:288 * i + 288])).hex() == h, ("H", i)
        assert o.g1_to_blst_affine(g1_jac_to_affine(P[144 * i:144 * i + 144])).hex() == p, ("rPK", i)
    d = c["defect"]
    bad = bytearray(host[:320 * n])
    apply_defect(bad, d)
    assert m.batchVerify(cache, bytes(bad), RND) is d["verdict"] is False, d
    if d["gt"] is not None:
        assert cache.fetch(4, 576).hex() == d["gt"], d
    cache.close()


def test_ladder_on_one_context(m, recs):
    """One context of the largest size walked down every size and back up: the verdict and GT value at every stop.  At 11 265 and 16 384
    sets (the ends of the window where k_hash_clear's scratch and the fork stream's extra-pair lines share the line store) three calls in a row."""
    d, _ = recs
    cache = m.BatchedBLSVerifierCache.init(max_sets=max(SIZES), numThreads=NT)
    down = sorted(SIZES, reverse=True)
    shared = (FX["slots"] * 11 + 1, FX["slots"] * 16)
    for n in down + down[::-1]:
        want = _case(n)["valid"]["gt"]
        for k in range(3 if n in shared else 1):
            assert cache.verify_device(d.data_ptr(), n, RND) is True, (n, k)
            assert cache.fetch(4, 576).hex() == want, (n, k)
    cache.close()

