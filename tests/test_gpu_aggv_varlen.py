"""aggregateVerify on messages of many lengths (tests/util.py varlen_case): k_hash_var with full waves, several blocks and lengths that diverge
inside a wave; the slicing of aggregate_verify_impl cut by the pair cap and by the byte budget, with slices that mix the two hashing paths;
the one-message capacity refusal; a small call after a large one on the same context.  Verdict AND GT value against the C restatement's
results in tests/golden/aggv_varlen.json (tests/golden/gen_aggv_varlen.py), on the valid input and on every defect, bit for bit."""
import hashlib

import pytest

import bls12381_py as o
from util import VARLEN_CASES, VARLEN_LONG, VARLEN_PREFIXES, aggv_one_slice_cap, aggv_slice_plan, golden, varlen_case, varlen_defect

pytestmark = pytest.mark.gpu

FX = golden("aggv_varlen")
SIZES = [(name, n) for name in VARLEN_CASES for n in VARLEN_PREFIXES[name]]
IDS = ["%s-%d" % s for s in SIZES]


def _fx(name, n):
    return [c for c in FX["cases"] if c["name"] == name and c["n"] == n][0]


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def inputs(m):
    """name -> (public keys, messages): the keys rebuilt by the device signer (tests/test_gpu_sign.py pins it byte-exact) from the rule's secret
    keys, the messages from the rule; both checked against the generator's digests at every size."""
    import torch
    import bench
    out = {}
    for name in VARLEN_CASES:
        sks, msgs = varlen_case(name)
        gen = m.BatchedBLSVerifierCache.init(max_sets=len(sks))
        rec = bytes(bench.sign_records(m, gen, torch.device("cuda", 0), range(len(sks)), sks=sks, msgs=[bytes(32)] * len(sks)).cpu().numpy())
        gen.close()
        pks = [rec[320 * i:320 * i + 96] for i in range(len(sks))]
        for n in VARLEN_PREFIXES[name]:
            c = _fx(name, n)
            assert hashlib.sha256(b"".join(pks[:n])).hexdigest() == c["pks_sha256"], ("keys differ from the generator's", name, n)
            h = hashlib.sha256()
            for x in msgs[:n]:
                h.update(len(x).to_bytes(4, "little"))
                h.update(x)
            assert h.hexdigest() == c["msgs_sha256"], ("messages differ from the generator's", name, n)
        out[name] = (pks, msgs)
    return out


def _check_case(m, cache, inputs, name, n, verify=None, sig=None):
    """the valid input and every defect of the fixture: verdict and GT"""
    verify = verify or m.aggregateVerify
    c = _fx(name, n)
    pks, msgs = inputs[name][0][:n], inputs[name][1][:n]
    sig = sig or bytes.fromhex(c["aggsig"])
    assert verify(cache, pks, msgs, sig) is c["valid"]["verdict"] is True, (name, n)
    assert cache.fetch(4, 576).hex() == c["valid"]["gt"], (name, n)
    assert len(c["defects"]) >= 1
    for d in c["defects"]:
        assert d["gt"] is not None
        assert verify(cache, pks, varlen_defect(msgs, d), sig) is d["verdict"] is False, (name, n, d["kind"], d["index"])
        assert cache.fetch(4, 576).hex() == d["gt"], (name, n, d["kind"], d["index"])


def test_fixture_holds_every_case():
    assert sorted((c["name"], c["n"]) for c in FX["cases"]) == sorted(SIZES)
    for name in ("mixed", "wide"):
        kinds = {(d["kind"], d.get("byte")) for d in _fx(name, VARLEN_PREFIXES[name][0])["defects"]}
        assert kinds == {("shift", None), ("trail", 0), ("trail", 0x80), ("flip", None), ("swap", None)}


@pytest.mark.parametrize("name,n", SIZES, ids=IDS)
def test_one_slice_both_modes(m, inputs, name, n):
    """One-shot aggregateVerify on the smallest context that takes the input in one slice: latency mode (the default) and throughput mode."""
    L = [len(x) for x in inputs[name][1][:n]]
    cap = aggv_one_slice_cap(L)
    plan = aggv_slice_plan(L, cap)
    assert len(plan) == 1 and (cap == n or aggv_slice_plan(L, cap - 1) is None or len(aggv_slice_plan(L, cap - 1)) > 1)
    assert not plan[0][3]                                     # no case is all 32-byte: k_hash_var hashes every one of them
    cache = m.BatchedBLSVerifierCache.init(max_sets=cap)
    for coop in (True, False):
        cache.set_cooperative(coop)
        _check_case(m, cache, inputs, name, n)
    cache.close()


@pytest.mark.parametrize("name,n", [s for s in SIZES if s[0] in ("wave", "mixed")], ids=[i for i, s in zip(IDS, SIZES) if s[0] in ("wave", "mixed")])
def test_streaming(m, inputs, name, n):
    """ContextCoreAggregateVerify: init, one update per pair, finish."""
    cache = m.BatchedBLSVerifierCache.init(max_sets=aggv_one_slice_cap([len(x) for x in inputs[name][1][:n]]))
    _check_case(m, cache, inputs, name, n, verify=m.aggregateVerifyStreaming)
    cache.close()


@pytest.mark.parametrize("n", VARLEN_PREFIXES["wave"])
def test_aggregate_signature_overload(m, inputs, n):
    """The 288-byte Jacobian AggregateSignature, built by aggregateAllSignatures from the fixture's aggregate, a point and its negative (the
    sum goes through real additions: Z is not 1)."""
    from util import g2_jac_to_affine
    cache = m.BatchedBLSVerifierCache.init(max_sets=256)
    agg = bytes.fromhex(_fx("wave", n)["aggsig"])
    q = o.g2_mul(o.G2_GEN, 0x1234567)
    agg288 = m.aggregateAllSignatures(cache, [o.g2_to_blst_affine(q), agg, o.g2_to_blst_affine(o.g2_neg(q))])
    assert len(agg288) == 288 and o.g2_to_blst_affine(g2_jac_to_affine(agg288)) == agg
    _check_case(m, cache, inputs, "wave", n, sig=agg288)
    cache.close()


@pytest.mark.parametrize("name,cap", [("mixed", 64), ("mixed", 1000), ("wide", 64), ("wide", 1000), ("long", 256)])
def test_sliced(m, inputs, name, cap):
    """Contexts smaller than the input: the GT value of the one-slice run (the fixture's) bit for bit.  The slice plan is derived from the
    mirrored rule (tests/util.py aggv_slice_plan, tied to the source by tests/test_aggv_plan_mirror.py) and must show what the case is for."""
    n = VARLEN_PREFIXES[name][0]
    L = [len(x) for x in inputs[name][1]]
    plan = aggv_slice_plan(L, cap)
    assert plan is not None and len(plan) > 1
    cuts = [p[2] for p in plan]
    if name == "long":
        # eight messages of 20 000 bytes on a budget of 81 920: every slice but the last ends on the byte budget, far below the pair cap
        assert L.count(VARLEN_LONG) == 8 and cap * 320 == 81920
        assert all(c == "bytes" for c in cuts[:-1]) and all(b - a < cap for a, b, _, _ in plan), plan
    if (name, cap) == ("mixed", 64):
        # slices on the prepared-constants kernels (all 32-byte) and on k_hash_var, ends moved by the pair cap and by the byte budget
        assert any(p[3] for p in plan) and any(not p[3] for p in plan), plan
        assert "pairs" in cuts and "bytes" in cuts, cuts
        assert any(not p[3] and 32 in L[p[0]:p[1]] for p in plan)            # 32-byte messages inside a slice that is not all-32
    if cap == 1000:
        assert "bytes" in cuts
    cache = m.BatchedBLSVerifierCache.init(max_sets=cap)
    modes = (True, False) if (name, cap) == ("mixed", 64) else (True,)
    for coop in modes:
        cache.set_cooperative(coop)
        _check_case(m, cache, inputs, name, n)
    cache.close()


def test_one_message_beyond_the_staging_buffer_is_refused(m, inputs):
    """A 64-set context stages 64 * 320 = 20 480 bytes: 4 + 96 + 4 + len fits up to len = 20 376.  One byte more returns MI355_BLS_ERR_CAPACITY
    (m._check raises BlsGpuError), alone or behind slices that already ran; the next valid call on the context gives the fixture's verdict and
    GT; a message of exactly 20 376 bytes is verified (against the C restatement)."""
    import c_oracle as co
    from util import ctr_bytes
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    limit = 64 * 320 - 104
    assert aggv_slice_plan([limit], 64) == [(0, 1, "end", False)] and aggv_slice_plan([limit + 1], 64) is None
    pks, msgs = inputs["wave"][0][:3], list(inputs["wave"][1][:3])
    sks = varlen_case("wave")[0][:3]
    big = ctr_bytes(b"capacity", limit + 1)
    sig = bytes.fromhex(_fx("wave", 63)["aggsig"])                # any signature: the call is refused before the pairing
    for bad in ([big], msgs[:1] + [big] + msgs[2:], msgs[:2] + [big]):
        with pytest.raises(m.BlsGpuError) as e:
            m.aggregateVerify(cache, pks[:len(bad)], bad, sig)
        assert "error -2:" in str(e.value) and "staging buffer" in str(e.value), str(e.value)
        _check_case(m, cache, inputs, "one", 1)
    # the largest message that fits, between two short ones (three slices: it fills one alone)
    fit = msgs[:1] + [big[:limit]] + msgs[2:]
    assert [p[:2] for p in aggv_slice_plan([len(x) for x in fit], 64)] == [(0, 1), (1, 2), (2, 3)]
    agg = co.g2_sum(b"".join(co.sign(sk, x) for sk, x in zip(sks, fit)))
    want, gt = co.aggregate_verify(pks, fit, agg, gt=True)
    assert want is True
    assert m.aggregateVerify(cache, pks, fit, agg) is True and cache.fetch(4, 576) == gt
    flipped = fit[:1] + [fit[1][:-1] + bytes([fit[1][-1] ^ 0x80])] + fit[2:]
    wantf, gtf = co.aggregate_verify(pks, flipped, agg, gt=True)
    assert wantf is False
    assert m.aggregateVerify(cache, pks, flipped, agg) is False and cache.fetch(4, 576) == gtf
    cache.close()


def test_small_calls_after_a_large_one_on_the_same_context(m, inputs):
    """wide, then one, then wave on ONE context: offsets and messages the larger call left in the staging buffer must not reach the smaller."""
    L = [len(x) for x in inputs["wide"][1]]
    cache = m.BatchedBLSVerifierCache.init(max_sets=aggv_one_slice_cap(L))
    for name, n in (("wide", 4097), ("one", 1), ("wave", 65), ("wave", 63), ("wave", 64)):
        _check_case(m, cache, inputs, name, n)
    cache.close()
