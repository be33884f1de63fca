"""The per-group aggregateVerify bodies (csrc/aggveach.hpp: the level-0 line product, the product of partials, the Horner over dense step
values, the carry multiply, the verdict) executed on the CPU under the bounds tracker (tests/host_emu/aggveach.cpp) over the plan's own slices
and item tables, for every group of tests/golden/aggregate_verify_each.json: verdict and 576-byte value against the fixture, the big-int
oracle (miller_loop + final_exp) and the C restatement's aggregateVerify - at the committed item width, with the width forced to 2 (groups of
3, 5 and 9 pairs take two to four levels) and cut into slices of 2 pairs, where every longer group goes through the carry."""
import ctypes
import os
import subprocess

import pytest

import bls12381_py as o
import c_oracle as co
from util import fp12_from_bytes, golden

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("valid", "wrong_message", "missing_member", "swapped_messages", "cancelling_pair", "infinity_public_key", "infinity_signature",
         "repeated_pair")


def groups():
    return golden("aggregate_verify_each")["groups"]


def size(g):
    return len(g["pks"]) // 192


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggveach.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libaggveach.so"))
    sz = ctypes.c_size_t
    L.emu_aggveach.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(sz), sz, ctypes.c_char_p, ctypes.c_uint32, sz, ctypes.c_char_p,
                               ctypes.c_char_p]

    def run(C, cap):
        """the whole fixture as one call -> (slices walked, [(verdict, value)])"""
        gs = groups()
        offs = [0]
        for g in gs:
            offs.append(offs[-1] + size(g))
        pks, msgs = b"".join(bytes.fromhex(g["pks"]) for g in gs), b"".join(bytes.fromhex(g["msgs"]) for g in gs)
        sigs = b"".join(bytes.fromhex(g["sig"]) for g in gs)
        k = len(gs)
        v, gt = ctypes.create_string_buffer(k), ctypes.create_string_buffer(576 * k)
        ns = L.emu_aggveach(pks, msgs, (sz * (k + 1))(*offs), k, sigs, C, cap, v, gt)
        raw = gt.raw
        return ns, [(v.raw[i], raw[576 * i:576 * i + 576]) for i in range(k)]
    return run


@pytest.fixture(scope="module")
def plain(emu):
    return emu(8, 1 << 16)


def test_fixture_has_every_kind():
    gs = groups()
    kinds = [g["kind"] for g in gs]
    for k in KINDS:
        assert k in kinds
    assert {size(g) for g in gs if g["kind"] == "valid"} == {1, 2, 3, 5, 9}
    assert all(g["verdict"] == (g["kind"] in ("valid", "cancelling_pair", "repeated_pair")) for g in gs)
    assert os.path.getsize(os.path.join(HERE, "golden", "aggregate_verify_each.json")) < 1 << 20


def test_bodies_equal_fixture(plain):
    ns, res = plain
    assert ns == 1
    for g, (ok, gt) in zip(groups(), res):
        assert ok == g["verdict"], g["kind"]
        assert gt.hex() == g["gt"], g["kind"]


def test_bodies_equal_bigint_oracle(plain):
    neg_g1 = o.g1_neg(o.G1_GEN)
    for g, (ok, gt) in zip(groups(), plain[1]):
        pkb, mb = bytes.fromhex(g["pks"]), bytes.fromhex(g["msgs"])
        t = size(g)
        pks = [o.g1_from_blst_affine(pkb[96 * j:96 * j + 96]) for j in range(t)]
        msgs = [mb[32 * j:32 * j + 32] for j in range(t)]
        sig = o.g2_from_blst_affine(bytes.fromhex(g["sig"]))
        v = o.final_exp(o.miller_loop([(pk, o.hash_to_g2(m)) for pk, m in zip(pks, msgs)] + [(neg_g1, sig)]))
        assert fp12_from_bytes(gt) == v, g["kind"]
        assert bool(ok) == (v == o.F12_ONE and all(pk is not None for pk in pks)), g["kind"]


def test_bodies_equal_c_oracle(plain):
    for g, (ok, gt) in zip(groups(), plain[1]):
        pkb, mb = bytes.fromhex(g["pks"]), bytes.fromhex(g["msgs"])
        msgs = [mb[32 * j:32 * j + 32] for j in range(size(g))]
        want_ok, want_gt = co.aggregate_verify(pkb, msgs, bytes.fromhex(g["sig"]), gt=True)
        assert bool(ok) == want_ok, g["kind"]
        if g["kind"] == "infinity_public_key":
            continue                                  # the restatement stops at the key (update returns false) and leaves no value
        assert gt == want_gt, g["kind"]


def test_width_two_takes_more_levels_and_changes_nothing(emu, plain):
    ns, res = emu(2, 1 << 16)
    assert ns == 1 and res == plain[1]


def test_parts_of_two_pairs_through_the_carry(emu, plain):
    ns, res = emu(8, 2)
    assert ns > len(groups())                         # the groups of 3, 5 and 9 pairs were walked in two, three and five parts
    assert res == plain[1]
