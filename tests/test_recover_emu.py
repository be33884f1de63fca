"""The threshold-signature recovery executed on the CPU under the bounds tracker (tests/host_emu/recover.cpp): the scalar field of csrc/fr.hpp
against Python integers, curve.hpp jac_mul_256_w4 against the bit-serial jac_mul_256 on chosen scalars, csrc/recover.hpp's coefficient
against the Python Lagrange coefficients, and the whole call - chunk by chunk, level by level as the kernels walk it - against every group of
tests/golden/recover_signatures.json: images, wire forms and status bytes byte-equal, in the contiguous and in the indexed form."""
import ctypes
import os
import random
import subprocess

import pytest

import recover_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
R = rc.R
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_recover.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "librecover.so"))
    cp, u32 = ctypes.c_char_p, ctypes.c_uint32
    L.emu_fr_op.argtypes = [ctypes.c_int, cp, cp, cp]
    L.emu_fr_op.restype = None
    L.emu_mul_256_w4.argtypes = [cp, cp, cp, cp, cp]
    L.emu_recover_coeff.argtypes = [cp, u32, u32, u32, cp]
    L.emu_recover_coeff.restype = u32
    L.emu_recover_signature_sets.argtypes = [cp, SZ, ctypes.POINTER(u32), ctypes.POINTER(SZ), SZ, cp, SZ, cp, cp, cp, ctypes.POINTER(SZ)]
    L.recover_plan_chunk.restype = SZ
    return L


def le(x):
    return x.to_bytes(32, "little")


def fr_op(lib, op, a, b=0):
    out = ctypes.create_string_buffer(32)
    lib.emu_fr_op(op, le(a), le(b), out)
    return int.from_bytes(out.raw, "little")


def test_constants_are_the_python_integers(lib):
    r, rr, n0 = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)(), ctypes.c_uint32()
    lib.emu_fr_constants(r, rr, ctypes.byref(n0))
    val = lambda w: sum(int(x) << (32 * i) for i, x in enumerate(w))          # noqa: E731
    assert val(r) == R == int(rc.fixture()["r"], 16)
    assert val(rr) == pow(2, 512, R)
    assert n0.value == (-pow(R, -1, 1 << 32)) % (1 << 32)


def test_fr_against_python_integers(lib):
    rng = random.Random(20261018)
    special = [0, 1, R - 1, (1 << 256) % R]
    vals = special + [rng.randrange(R) for _ in range(24)]
    for a in vals:
        assert fr_op(lib, 4, a) == a
        assert fr_op(lib, 3, a) == pow(a, R - 2, R), hex(a)              # 0 -> 0
        assert fr_op(lib, 5, a) == int(a == 0)
        for b in vals:
            assert fr_op(lib, 0, a, b) == a * b % R, (hex(a), hex(b))
            assert fr_op(lib, 1, a, b) == (a + b) % R, (hex(a), hex(b))
            assert fr_op(lib, 2, a, b) == (a - b) % R, (hex(a), hex(b))
    for a in (R - 1, R, R + 1, 1 << 255, (1 << 256) - 1):                # fr_from_le32 takes any 256-bit value
        assert fr_op(lib, 4, a) == a % R, hex(a)
        assert fr_op(lib, 5, a) == int(a % R == 0)
        assert fr_op(lib, 0, a, a) == a * a % R


def chosen_scalars(fx):
    cs = [(g["kind"], int.from_bytes(bytes.fromhex(g["coeff"]), "little")) for g in fx["groups"] if g["kind"].startswith("coeff_")]
    names = {n for n, _ in cs}
    assert {"coeff_two", "coeff_all_8", "coeff_all_7", "coeff_all_9", "coeff_carry_chain", "coeff_one_digit", "coeff_r_minus_1",
            "coeff_accumulator_equals_entry"} <= names and sum(n.startswith("coeff_8_at_") for n in names) >= 3
    w4 = {k: int.from_bytes(bytes.fromhex(v), "little") for k, v in fx["w4"].items()}
    assert dict(cs)["coeff_accumulator_equals_entry"] == w4["double"] < R <= w4["cancel"]
    return cs + [("w4_cancel", w4["cancel"]), ("zero", 0), ("one", 1), ("final_carry", (1 << 256) - 1), ("r_plus_one", R + 1)]


def test_windowed_multiplication_equals_the_bit_serial_one(lib):
    import bls12381_py as o
    fx = rc.fixture()
    tab = rc.table_of(fx)
    base = tab[3]
    a, b, st = ctypes.create_string_buffer(192), ctypes.create_string_buffer(192), ctypes.create_string_buffer(2)
    rng = random.Random(7)
    scalars = chosen_scalars(fx) + [("random_%d" % i, rng.getrandbits(256)) for i in range(4)]
    for name, k in scalars:
        assert lib.emu_mul_256_w4(base, le(k), a, b, st) == 1, name
        assert st.raw == (bytes([2, 2]) if k % R == 0 else bytes(2)), name
    # two of them against the Python oracle as well: the all-8 scalar and the one that takes the doubling branch
    pt = o.g2_from_blst_affine(base)
    for name in ("coeff_all_8", "coeff_accumulator_equals_entry"):
        k = dict(scalars)[name]
        assert lib.emu_mul_256_w4(base, le(k), a, b, st) == 1 and a.raw == o.g2_to_blst_affine(o.g2_mul(pt, k)), name
    for name, k in scalars[:6] + scalars[-2:]:                           # the infinity base
        assert lib.emu_mul_256_w4(bytes(192), le(k), a, b, st) == 1 and st.raw == bytes([2, 2]) and a.raw == bytes(192), name


def test_coefficients_equal_the_python_lagrange_coefficients(lib):
    fx = rc.fixture()
    out = ctypes.create_string_buffer(32)
    seen = set()
    for g in fx["groups"]:
        ids = [int.from_bytes(bytes.fromhex(x), "little") for x in g["ids"]]
        n = len(ids)
        if n == 0 or (n > 9 and g["kind"] != "len_65"):
            continue
        pad = 3                                                          # the group does not start at position 0
        blob = bytes(32 * pad) + b"".join(le(x) for x in ids)
        for i in range(n):
            fl = lib.emu_recover_coeff(blob, pad, n, pad + i, out)
            got = int.from_bytes(out.raw, "little")
            xs = [x % R for x in ids]
            zero = n >= 2 and 0 in xs
            dup = n >= 2 and any(xs[j] == xs[i] for j in range(n) if j != i)
            assert fl == (2 if zero else 0) | (4 if dup else 0), (g["kind"], i)
            assert got == (1 if n == 1 else 0 if fl else rc.coefficient(ids, i)), (g["kind"], i)
            seen.add(fl)
    assert {0, 2, 4} <= seen


@pytest.fixture(scope="module")
def emu(lib):
    def run(sigs, idx, offsets, ids, chunk=0, want192=True, want96=True):
        k = len(offsets) - 1
        o192 = ctypes.create_string_buffer(192 * k) if want192 else None
        o96 = ctypes.create_string_buffer(96 * k) if want96 else None
        st = ctypes.create_string_buffer(k)
        iarr = (ctypes.c_uint32 * len(idx))(*idx) if idx is not None else None
        walked = SZ()
        r = lib.emu_recover_signature_sets(sigs, len(sigs) // 192, iarr, (SZ * (k + 1))(*offsets), k, ids, chunk or lib.recover_plan_chunk(), o192, o96, st,
                                           ctypes.byref(walked))
        return r, o192.raw if want192 else None, o96.raw if want96 else None, st.raw, walked.value
    return run


def test_fixture_has_every_kind():
    fx = rc.fixture()
    by = {g["kind"]: g for g in fx["groups"]}
    assert len(fx["groups"]) <= 45 and os.path.getsize(os.path.join(HERE, "golden", "recover_signatures.json")) < 1 << 20
    assert [by[n]["status"] for n in ("edge_empty", "edge_one_id_zero", "edge_zero_id", "edge_dup_595", "edge_dup_mod_r", "edge_result_infinity")] == [1, 0, 6, 7, 7, 2]
    assert by["edge_r_plus_3"]["out192"] == by["edge_3"]["out192"] != rc.INF192.hex() and by["edge_r_plus_3"]["ids"] != by["edge_3"]["ids"]
    assert by["edge_id_all_ones"]["ids"][0] == "ff" * 32 and 0 in by["edge_infinity_member"]["members"]
    assert {len(by["len_%d" % n]["members"]) for n in (8, 9, 64, 65)} == {8, 9, 64, 65}
    assert by["ref_3_of_3"]["ids"] == [(x << 224).to_bytes(32, "little").hex() for x in (1, 2, 3)]
    ref = [g for g in fx["groups"] if g["kind"].startswith("ref_")]
    assert sum(g["verify"] is True for g in ref) == 8 and sum(g["verify"] is False for g in ref) == 6 and all(g["status"] == 0 for g in ref)
    assert by["ref_2_of_3_all"]["out192"] == by["ref_1_of_1"]["out192"] == by["ref_rekeyed"]["out192"] == by["ref_2_of_3_reversed"]["out192"]
    for g in fx["groups"]:
        assert (g["status"] != 0) == (g["out192"] == rc.INF192.hex()) == (g["out96"] == rc.INF96.hex()), g["kind"]
    ix = fx["indexed"]
    assert len(set(ix["idx"])) < len(ix["idx"]) and ix["idx"] != sorted(ix["idx"]) and ix["bad_index"]["value"] >= len(rc.table_of(fx))


def test_whole_call_equals_fixture(emu):
    sigs, ids, offsets, w192, w96, status = rc.contiguous_inputs()
    r, o192, o96, st, walked = emu(sigs, None, offsets, ids)
    assert st == status and r == 0 and walked == 1
    for g in range(len(st)):
        assert o192[192 * g:192 * g + 192] == w192[192 * g:192 * g + 192], g
        assert o96[96 * g:96 * g + 96] == w96[96 * g:96 * g + 96], g
    good = [g for g in rc.fixture()["groups"] if g["status"] == 0]
    sigs, ids, offsets, w192, w96, status = rc.contiguous_inputs(groups=good)
    assert emu(sigs, None, offsets, ids)[:4] == (1, w192, w96, bytes(len(good)))


def test_indexed_form_bad_index_and_chunks(emu):
    # the indexed form, walked in chunks of 16 members: groups of 64 and 65 are chunks of their own, small groups share chunks
    for bad in (False, True):
        table, idx, ids, offsets, w192, w96, status = rc.indexed_inputs(bad)
        r, o192, o96, st, walked = emu(table, idx, offsets, ids, chunk=16)
        assert (r, o192, o96, st) == (0, w192, w96, status), bad
        assert 3 < walked < len(status)
    assert 3 in rc.indexed_inputs(True)[6]
    table, idx, ids, offsets, w192, w96, status = rc.indexed_inputs()
    assert emu(table, idx, offsets, ids, chunk=1, want96=False)[1:4] == (w192, None, status)          # every group a chunk; either output missing
    assert emu(table, idx, offsets, ids, chunk=70, want192=False)[1:4] == (None, w96, status)


def test_refused_offsets(emu):
    sigs, ids, _, _, _, _ = rc.contiguous_inputs()
    assert emu(sigs, None, [0, 2, 1], ids)[0] == -3
    assert emu(sigs[:192], None, [0, 2], ids)[0] == -3                   # offsets[k] past the table without indices
    assert emu(sigs[:192], [0, 0], [0, 2], bytes(64))[0] == 0            # through indices it runs: ids 0, 0 -> status 6
