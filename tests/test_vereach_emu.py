"""The per-set verification body (csrc/vereach.hpp: two-pair Horner over the 68 steps, final exponentiation, comparison with one) executed on the
CPU under the bounds tracker (tests/host_emu/vereach.cpp), for every set of tests/golden/verify_each.json: verdict and 576-byte value against
the big-int oracle (miller_loop + final_exp), against the C restatement's aggregateVerify of the one pair, and against the fixture.  The body
is tower arithmetic on one lane: it uses no team or row program, so there is no table to put through the interpreters."""
import ctypes
import os
import subprocess

import pytest

import bls12381_py as o
import c_oracle as co
from util import fp12_from_bytes, golden

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vereach():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_vereach.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libvereach.so"))
    L.emu_vereach_set.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return L


@pytest.fixture(scope="module")
def results(vereach):
    out = []
    for s in golden("verify_each")["sets"]:
        rec = bytes.fromhex(s["set"])
        b = ctypes.create_string_buffer(576)
        out.append((vereach.emu_vereach_set(rec, b), b.raw))
    return out


def test_fixture_has_every_kind():
    kinds = [s["kind"] for s in golden("verify_each")["sets"]]
    for k in ("valid", "wrong_message", "other_key", "swapped_pair", "infinity_signature", "infinity_public_key", "doubled_signature"):
        assert k in kinds
    assert kinds.count("swapped_pair") == 2 and kinds.count("valid") >= 5
    assert all(s["verdict"] == (s["kind"] == "valid") for s in golden("verify_each")["sets"])


def test_body_equals_fixture(results):
    for s, (ok, gt) in zip(golden("verify_each")["sets"], results):
        assert ok == s["verdict"], s["kind"]
        assert gt.hex() == s["gt"], s["kind"]


def test_body_equals_bigint_oracle(results):
    neg_g1 = o.g1_neg(o.G1_GEN)
    for s, (ok, gt) in zip(golden("verify_each")["sets"], results):
        rec = bytes.fromhex(s["set"])
        pk, msg, sig = o.g1_from_blst_affine(rec[:96]), rec[96:128], o.g2_from_blst_affine(rec[128:])
        v = o.final_exp(o.miller_loop([(pk, o.hash_to_g2(msg)), (neg_g1, sig)]))
        assert fp12_from_bytes(gt) == v, s["kind"]
        assert bool(ok) == (v == o.F12_ONE and pk is not None) == o.core_verify(pk, msg, sig), s["kind"]


def test_body_equals_c_oracle(results):
    for s, (ok, gt) in zip(golden("verify_each")["sets"], results):
        rec = bytes.fromhex(s["set"])
        assert bool(ok) == co.core_verify(rec[:96], rec[96:128], rec[128:]), s["kind"]
        if s["kind"] == "infinity_public_key":
            continue                                  # the restatement stops at the key (BLST_PK_IS_INFINITY) and leaves no value
        want_ok, want_gt = co.aggregate_verify([rec[:96]], [rec[96:128]], rec[128:], gt=True)
        assert (bool(ok), gt) == (want_ok, want_gt), s["kind"]
