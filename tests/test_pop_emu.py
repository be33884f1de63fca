"""popVerify's new arithmetic executed on the CPU under the bounds tracker (tests/host_emu/pop.cpp): G1 point compression (csrc/deser.hpp
g1_compress), the prepared-constants hash_to_field for 48-byte messages (csrc/h2c.hpp) and the PoP hash-map body end to end, against the
big-int oracle, for the keys of tests/golden/pop.json."""
import ctypes
import os
import subprocess

import pytest

import bls12381_py as o
from util import fp2_int, g2_jac_to_affine, golden

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pop():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_pop.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libpop.so"))
    cp, u32 = ctypes.c_char_p, ctypes.c_uint32
    L.emu_g1_compress.argtypes = [cp, cp]
    L.emu_g1_compress.restype = None
    L.emu_hash_to_field.argtypes = [cp, u32, cp, u32, cp]
    L.emu_hash_to_field.restype = None
    L.emu_hash_to_field_msg48.argtypes = [cp, cp, u32, cp]
    L.emu_pop_hash_to_field.argtypes = [cp, cp, u32, cp]
    L.emu_pop_hash_to_g2.argtypes = [cp, cp]
    return L


def _keys():
    """the fixture's keys as oracle points (None: the infinity key)"""
    return [o.g1_from_blst_affine(bytes.fromhex(c["pk"])) for c in golden("pop")["cases"]]


def _compress(L, pk):
    b = ctypes.create_string_buffer(48)
    L.emu_g1_compress(o.g1_to_blst_affine(pk), b)
    return b.raw


def _us(b):
    return [fp2_int(b[:96]), fp2_int(b[96:192])]


def test_fixture_has_every_kind():
    cases = golden("pop")["cases"]
    kinds = [c["kind"] for c in cases]
    for k in ("valid", "other_key_proof", "doubled_proof", "infinity_proof", "infinity_key", "swapped_proofs"):
        assert k in kinds
    assert kinds.count("swapped_proofs") == 2 and sum(c["reference"] for c in cases) == 3
    assert all(c["verdict"] == (c["kind"] == "valid") for c in cases)
    assert {bytes.fromhex(c["compressed"])[0] >> 5 & 1 for c in cases if c["kind"] != "infinity_key"} == {0, 1}      # both signs of y
    assert golden("pop")["batch"]["indices"] == [i for i, c in enumerate(cases) if c["verdict"]]


def test_compress_equals_oracle_and_fixture(pop):
    for c, pk in zip(golden("pop")["cases"], _keys()):
        assert _compress(pop, pk) == o.g1_compress(pk) == bytes.fromhex(c["compressed"]), c["kind"]


def test_compress_of_negated_keys_has_the_other_sign_bit(pop):
    for pk in _keys():
        if pk is None:
            continue
        neg = o.g1_neg(pk)
        got = _compress(pop, neg)
        assert got == o.g1_compress(neg)
        assert got[0] ^ _compress(pop, pk)[0] == 0x20 and got[1:] == _compress(pop, pk)[1:]


def test_compress_of_infinity(pop):
    assert _compress(pop, None) == bytes([0xc0]) + bytes(47) == o.g1_compress(None)


def test_prepared_form_equals_oracle_and_generic(pop):
    for c in golden("pop")["cases"]:
        msg = bytes.fromhex(c["compressed"])
        a, b = ctypes.create_string_buffer(192), ctypes.create_string_buffer(192)
        assert pop.emu_hash_to_field_msg48(msg, o.DST_POP, len(o.DST_POP), a) == 1
        pop.emu_hash_to_field(msg, 48, o.DST_POP, len(o.DST_POP), b)
        assert _us(a.raw) == _us(b.raw) == o.hash_to_field_fp2(msg, o.DST_POP), c["kind"]


@pytest.mark.parametrize("dst_len,prepared", [(27, False), (28, True), (43, True), (67, True), (68, False), (83, False), (12, False)])
def test_prepared_form_at_the_ends_of_its_range(pop, dst_len, prepared):
    """valid for 28 <= dst_len <= 67 (h2c.hpp: b_0 needs 12..67, b_i 28..83); outside it the lane takes the generic path"""
    dst = bytes((37 * i + 11) % 251 + 1 for i in range(dst_len))
    for c in golden("pop")["cases"][:4] + golden("pop")["cases"][7:8]:
        msg = bytes.fromhex(c["compressed"])
        a, b, d = ctypes.create_string_buffer(192), ctypes.create_string_buffer(192), ctypes.create_string_buffer(192)
        assert pop.emu_hash_to_field_msg48(msg, dst, dst_len, a) == int(prepared)
        pop.emu_hash_to_field(msg, 48, dst, dst_len, b)
        assert pop.emu_pop_hash_to_field(bytes.fromhex(c["pk"]), dst, dst_len, d) == int(prepared)       # which path the lane took
        want = o.hash_to_field_fp2(msg, dst)
        assert _us(b.raw) == _us(d.raw) == want
        if prepared:
            assert _us(a.raw) == want


def test_pop_hash_map_body_end_to_end(pop):
    for c, pk in zip(golden("pop")["cases"], _keys()):
        out = ctypes.create_string_buffer(288)
        assert pop.emu_pop_hash_to_g2(bytes.fromhex(c["pk"]), out) == 1
        assert g2_jac_to_affine(out.raw) == o.hash_to_g2(o.g1_compress(pk), o.DST_POP), c["kind"]
