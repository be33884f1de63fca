"""The key-table decoder (csrc/deser.hpp deserialize_public_key, a lane of k_deser_pks) and key admission's record gather (csrc/keytable.hpp, a
lane of k_admit_records) executed on the CPU under the bounds tracker (tests/host_emu/keytable.cpp): every key encoding of
tests/golden/deser_adversarial.json in both wire forms, with and without KNOWN_ON_CURVE, and the rows of tests/golden/key_table.json - status
and image byte-equal to the big-integer oracle; the key half of deserialize_tuple unchanged; the gather byte-equal to k_pop_records' body over
the same pairs laid out contiguously."""
import ctypes
import os
import subprocess

import pytest

import bls12381_py as o
import deser_cases as dc
import key_table_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_keytable.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libkeytable.so"))
    cp, sz, u32 = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32
    L.emu_deserialize_public_keys.argtypes = [cp, sz, u32, cp, cp]
    L.emu_tuple_key.argtypes = [cp, cp, u32, cp]
    L.emu_tuple_key.restype = ctypes.c_uint8
    L.emu_admit_records.argtypes = [cp, cp, ctypes.POINTER(u32), sz, cp]
    L.emu_pop_records.argtypes = [cp, cp, sz, cp]
    return L


def decode_keys(lib, pk, n, flags):
    out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    rc = lib.emu_deserialize_public_keys(pk, n, flags, out, st)
    return rc, out.raw, st.raw


def test_fixture_has_every_status_and_fits():
    fx = kc.fixture()
    rows = fx["rows"]
    assert {r["status"] for r in rows} == {0, 1, 2, 3, 4, 5, 8}
    assert {int(r["pk"]["c"][:2], 16) >> 5 & 1 for r in rows if r["status"] == 0} == {0, 1}       # both signs of y among the admitted keys
    kinds = [r["kind"] for r in rows]
    for k in ("pop_valid", "pop_other_key_proof", "pop_doubled_proof", "pop_infinity_proof", "pop_infinity_key", "pop_swapped_proofs"):
        assert k in kinds, k
    assert kinds[:12] == ["pop_" + c["kind"] for c in __import__("util").golden("pop")["cases"]]
    assert {k[4:] for k in kinds if k.startswith("key_")} == {nm for nm, _ in kc.adversarial_keys(False)} | {nm for nm, _ in kc.adversarial_keys(True)}
    for r in rows:
        assert (r["status"] == 0) == (r["image"] != bytes(96).hex()), r["kind"]
    by = {r["kind"]: r["status"] for r in rows}
    assert by["pop_infinity_proof"] == 8 and by["pop_infinity_key"] == 3 and by["proof_off_curve_c"] == by["proof_off_curve_u"] == 4
    assert by["proof_g2_xc1_p"] == by["proof_g2_xc0_p"] == by["proof_g2_inf_payload"] == 4 and by["proof_g2_ord13_0_pos"] == 5
    gold = os.path.join(HERE, "golden")
    assert os.path.getsize(os.path.join(gold, "key_table.json")) <= max(os.path.getsize(os.path.join(gold, n)) for n in os.listdir(gold) if n != "key_table.json")


@pytest.mark.parametrize("unc", (False, True))
@pytest.mark.parametrize("known", (False, True))
def test_decoder_on_adversarial_encodings(lib, unc, known):
    encs = kc.adversarial_keys(unc)
    n, unit = len(encs), (96 if unc else 48)
    assert n >= 30
    flags = (dc.PK_UNCOMPRESSED if unc else 0) | (dc.KNOWN_ON_CURVE if known else 0)
    pk = b"".join(b for _, b in encs)
    assert len(pk) == unit * n
    rc, out, st = decode_keys(lib, pk, n, flags)
    want = [kc.oracle_key(b, unc, known) for _, b in encs]
    for k, (nm, _) in enumerate(encs):
        assert st[k] == want[k][0], nm
        assert out[96 * k:96 * k + 96] == want[k][1], nm
    assert rc == int(not any(st))
    assert set(st) == ({0, 1, 3} if known else {0, 1, 2, 3})
    if known:                                                                 # the points outside G1 decode to their images
        off = [k for k, (_, b) in enumerate(encs) if kc.oracle_key(b, unc, False)[0] == 2]
        assert len(off) >= 20 and all(st[k] == 0 and out[96 * k:96 * k + 96] != bytes(96) for k in off)


@pytest.mark.parametrize("unc", (False, True))
def test_tuple_decoder_keeps_its_key_half(lib, unc):
    """deserialize_tuple now calls deserialize_public_key: beside a signature that decodes, its status and key are that function's"""
    import c_oracle as co
    sig96 = co.compress_sets(co.make_batch(1, seed=11))[2]
    encs = kc.adversarial_keys(unc)
    for known in (False, True):
        flags = (dc.PK_UNCOMPRESSED if unc else 0) | (dc.KNOWN_ON_CURVE if known else 0)
        _, out, st = decode_keys(lib, b"".join(b for _, b in encs), len(encs), flags)
        for k, (nm, b) in enumerate(encs):
            buf = ctypes.create_string_buffer(96)
            assert lib.emu_tuple_key(b, sig96, flags, buf) == st[k], nm
            assert buf.raw == out[96 * k:96 * k + 96], nm


@pytest.mark.parametrize("unc", (False, True))
def test_decoder_on_fixture_rows(lib, unc):
    kinds, pk, _, status, table = kc.admit_inputs(unc, False)
    n = len(kinds)
    rc, out, st = decode_keys(lib, pk, n, dc.PK_UNCOMPRESSED if unc else 0)
    unit = 96 if unc else 48
    for k in range(n):
        want_st, want_img = kc.oracle_key(pk[unit * k:unit * k + unit], unc, False)
        assert (st[k], out[96 * k:96 * k + 96]) == (want_st, want_img), kinds[k]
        # the admission status is the key's wherever the key fails, and an admitted key's row is the decoder's image
        assert (st[k] != 0) == (status[k] in (1, 2, 3)) and (st[k] == 0 or st[k] == status[k]), kinds[k]
        if status[k] == 0:
            assert out[96 * k:96 * k + 96] == table[96 * k:96 * k + 96], kinds[k]
    assert rc == 0


def test_record_gather_equals_pop_records_over_the_survivors(lib):
    kinds, pk, pr, status, _ = kc.admit_inputs(True, True)
    n = len(kinds)
    keys = b"".join(kc.oracle_key(pk[96 * k:96 * k + 96], True, False)[1] for k in range(n))
    proofs = []
    for k in range(n):
        ok, pt = dc.decode("sig", pr[192 * k:192 * k + 192], True)
        proofs.append(o.g2_to_blst_affine(pt) if ok and (pt is None or dc.in_subgroup("sig", pt)) else bytes(192))
    proofs = b"".join(proofs)
    surv = [k for k in range(n) if status[k] in (0, kc.KEY_BAD_PROOF)]        # both columns decode
    assert 10 <= len(surv) < n and surv != list(range(len(surv)))
    for lst in (surv, surv[::-1], [surv[0]], []):
        m = len(lst)
        got, want = ctypes.create_string_buffer(max(320 * m, 1)), ctypes.create_string_buffer(max(320 * m, 1))
        lib.emu_admit_records(keys, proofs, (ctypes.c_uint32 * max(m, 1))(*lst), m, got)
        lib.emu_pop_records(b"".join(keys[96 * k:96 * k + 96] for k in lst), b"".join(proofs[192 * k:192 * k + 192] for k in lst), m, want)
        assert got.raw == want.raw
        for j, k in enumerate(lst):
            assert got.raw[320 * j:320 * j + 320] == keys[96 * k:96 * k + 96] + bytes(32) + proofs[192 * k:192 * k + 192]
