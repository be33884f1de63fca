"""The short linear combinations executed on the CPU under the bounds tracker (tests/host_emu/lincomb.cpp): the base-X decomposition of
csrc/lincomb.hpp against Python integers, the psi-Straus walk and the shortened windowed walk against the bit-serial jac_mul_256 and against
the oracle's multiples on every chosen scalar, and the whole call - chunk by chunk, level by level as the kernels walk it - byte-equal to
tests/golden/lincomb.json: contiguous and indexed forms, both G2 routes, the chunk forced to 16 terms."""
import ctypes
import os
import random
import subprocess

import pytest

import lincomb_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
R, X = lc.R, lc.X
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_lincomb.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "liblincomb.so"))
    cp, u32 = ctypes.c_char_p, ctypes.c_uint32
    L.emu_lincomb_base_x.argtypes = [cp, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.emu_lincomb_base_x.restype = None
    L.emu_lincomb_x_abs.restype = ctypes.c_uint64
    L.emu_lincomb_mul.argtypes = [ctypes.c_int, cp, cp, u32, ctypes.c_int, cp, cp, cp]
    L.emu_lincomb_many.argtypes = [ctypes.c_int, cp, SZ, ctypes.POINTER(u32), ctypes.POINTER(SZ), SZ, cp, u32, ctypes.c_int, SZ, cp, cp, ctypes.POINTER(SZ)]
    return L


@pytest.fixture(scope="module")
def fx():
    return lc.fixture()


def le(x):
    return x.to_bytes(32, "little")


def chosen(fx, curve):
    return [(g["kind"], int.from_bytes(bytes.fromhex(g["terms"][0][1]), "little")) for g in fx[curve]["groups"] if g["kind"].startswith("k_")]


def test_fixture_has_every_kind(fx):
    assert os.path.getsize(os.path.join(HERE, "golden", "lincomb.json")) < 1 << 20
    assert int(fx["r"], 16) == R and int(fx["x_abs"], 16) == X and R == X ** 4 - X ** 2 + 1
    for curve in ("g1", "g2"):
        by = {g["kind"]: g for g in fx[curve]["groups"]}
        assert len(by) == len(fx[curve]["groups"]) <= 50
        assert [len(by["len_%d" % n]["terms"]) for n in (0, 1, 2, 3, 8, 9, 64, 65)] == [0, 1, 2, 3, 8, 9, 64, 65]
        assert [by[n]["status"] for n in ("len_0", "edge_s_and_minus_s", "edge_p_and_minus_p", "edge_zero_scalars", "edge_same_term_twice", "edge_zero_point")] == [1, 2, 2, 2, 0, 0]
        assert by["edge_same_term_twice"]["terms"][0] == by["edge_same_term_twice"]["terms"][1] and 0 in [t for t, _ in by["edge_zero_point"]["terms"]]
        ks = dict(chosen(fx, curve))
        want = {0, 1, 8, 9, 15, 16, int("8" * 64, 16), (1 << 256) - 1, R - 1, R, R + 1, 1 << 255}
        assert want <= set(ks.values()) and sum(n.startswith("k_8_at_") for n in ks) >= 3
        assert {g["nbits"] for g in fx[curve]["groups"] if g["kind"].startswith("nbits_")} == {1, 4, 5, 64, 255, 256}
        for g in fx[curve]["groups"]:
            assert (g["status"] != 0) == (g["out"] == bytes(lc.ROW[curve]).hex()), g["kind"]
            if g["kind"].startswith("nbits_"):                                   # scalars with high bits set: the mask has work to do
                assert g["terms"][0][1] == "ff" * 32 and all(int.from_bytes(bytes.fromhex(s), "little") >> g["nbits"] == (1 << 256 - g["nbits"]) - 1 for _, s in g["terms"])
    ks = dict(chosen(fx, "g2"))
    assert {X - 1, X, X + 1, X ** 2, X ** 3, X ** 3 + X ** 2 + X + 1, X ** 4 - 1} <= set(ks.values())
    assert lc.base_x(ks["k_digits_x_minus_1_below_r"])[:3] == [X - 1] * 3
    d = lc.base_x(ks["k_d0_eq_d2_d1_eq_d3"])
    assert d[0] == d[2] and d[1] == d[3] and d[0] != d[1]
    assert all(x == 16 ** 15 * 8 + 8 for x in lc.base_x(ks["k_digits_8_at_15_plus_8"]))
    out = [g for g in fx["g2"]["groups"] if g["kind"].startswith("edge_outside_g2")]
    assert len(out) == 2 and all(not g["psi"] and g["status"] == 0 for g in out) and all(g["psi"] for g in fx["g2"]["groups"] if g not in out)


def test_base_x_decomposition_against_python_integers(lib, fx):
    assert lib.emu_lincomb_x_abs() == X
    rng = random.Random(20261020)
    scalars = [k for _, k in chosen(fx, "g2")] + [rng.getrandbits(256) for _ in range(200)]
    out = (ctypes.c_uint64 * 4)()
    for k in scalars:
        for nbits in (256, 255, 64):
            m = k & ((1 << nbits) - 1)
            lib.emu_lincomb_base_x(le(k), nbits, out)
            d = [int(x) for x in out]
            assert all(x < X for x in d) and sum(x * X ** i for i, x in enumerate(d)) == m % R, (hex(k), nbits)
            assert d == lc.base_x(m)


def test_walks_equal_the_bit_serial_multiplication_and_the_oracle(lib, fx):
    import bls12381_py as o
    rng = random.Random(11)
    for curve, g2 in (("g1", 0), ("g2", 1)):
        row = lc.ROW[curve]
        tab = lc.table_of(fx, curve)
        base = tab[3]
        by = {g["kind"]: g for g in fx[curve]["groups"]}
        a, b, st = ctypes.create_string_buffer(row), ctypes.create_string_buffer(row), ctypes.create_string_buffer(2)
        scalars = chosen(fx, curve) + [("random_%d" % i, rng.getrandbits(256)) for i in range(3)]
        for route in ((0, 1) if g2 else (0,)):
            for name, k in scalars:
                assert lib.emu_lincomb_mul(g2, base, le(k), 256, route, a, b, st) == 1, (curve, route, name)
                assert st.raw == (bytes([2, 2]) if k % R == 0 else bytes(2)), name
                if name in by:                                               # ... and the oracle's multiple, as the fixture holds it
                    assert a.raw.hex() == by[name]["out"], (curve, route, name)
            for name, k in scalars[:4] + scalars[-1:]:                       # the infinity base
                assert lib.emu_lincomb_mul(g2, bytes(row), le(k), 256, route, a, b, st) == 1 and st.raw == bytes([2, 2]) and a.raw == bytes(row), name
            # the mask and the shortened walk: every nbits of the fixture and the window edges around them, over scalars with high bits set
            for nbits in (1, 3, 4, 5, 8, 9, 63, 64, 65, 252, 253, 255, 256):
                for k in ((1 << 256) - 1, ((1 << 256) - 1) ^ (1 << (nbits - 1)), int("8" * 64, 16), rng.getrandbits(256) | (1 << 255)):
                    assert lib.emu_lincomb_mul(g2, base, le(k), nbits, route, a, b, st) == 1, (curve, route, nbits, hex(k))
        if g2:                                                               # outside G2 the plain route is the integer multiple; the psi route is not
            outside = tab[-1]
            k = R + 5
            assert lib.emu_lincomb_mul(1, outside, le(k), 256, 0, a, b, st) == 1 and a.raw.hex() == by["edge_outside_g2"]["out"]
            assert a.raw == o.g2_to_blst_affine(o.g2_mul(o.g2_from_blst_affine(outside), k))
            assert lib.emu_lincomb_mul(1, outside, le(k), 256, 1, a, b, st) == 0


@pytest.fixture(scope="module")
def emu(lib):
    def run(g2, pts, idx, offsets, sc, nbits, psi=0, forced=0):
        row = 192 if g2 else 96
        k = len(offsets) - 1
        out, st = ctypes.create_string_buffer(row * k), ctypes.create_string_buffer(k)
        iarr = (ctypes.c_uint32 * max(len(idx), 1))(*idx) if idx is not None else None
        walked = SZ()
        r = lib.emu_lincomb_many(g2, pts, len(pts) // row, iarr, (SZ * (k + 1))(*offsets), k, sc, nbits, psi, forced, out, st, ctypes.byref(walked))
        return r, out.raw, st.raw, walked.value
    return run


ROUTES = [("g1", 0), ("g2", 0), ("g2", 1)]


@pytest.mark.parametrize("curve,psi", ROUTES)
def test_whole_call_equals_fixture(emu, fx, curve, psi):
    g2 = int(curve == "g2")
    row = lc.ROW[curve]
    for nbits in lc.nbits_values(fx, curve):
        groups = lc.groups_of(fx, curve, nbits, psi)
        pts, sc, offsets, want, status = lc.contiguous_inputs(fx, curve, groups)
        r, out, st, walked = emu(g2, pts, None, offsets, sc, nbits, psi)
        assert st == status and r == int(not any(status)) and walked == 1, nbits
        for g in range(len(st)):
            assert out[row * g:row * g + row] == want[row * g:row * g + row], (nbits, groups[g]["kind"])
    assert {0, 1, 2} <= {g["status"] for g in lc.groups_of(fx, curve, 255, psi)}


@pytest.mark.parametrize("curve,psi", ROUTES)
def test_indexed_form_bad_index_and_chunks(emu, fx, curve, psi):
    g2 = int(curve == "g2")
    groups = lc.groups_of(fx, curve, 255, psi)
    for bad in (False, True):
        table, idx, sc, offsets, want, status = lc.indexed_inputs(fx, curve, groups, bad)
        r, out, st, walked = emu(g2, table, idx, offsets, sc, 255, psi, forced=16)       # groups of 64 and 65 are chunks of their own
        assert (r, out, st) == (0, want, status), bad
        assert 3 < walked < len(status)
        assert emu(g2, table, idx, offsets, sc, 255, psi)[:3] == (0, want, status)
    assert 3 in lc.indexed_inputs(fx, curve, groups, True)[5]
    table, idx, sc, offsets, want, status = lc.indexed_inputs(fx, curve, groups)
    assert emu(g2, table, idx, offsets, sc, 255, psi, forced=1)[1:] == (want, status, len(status))      # every group a chunk


def test_refused_offsets(emu, fx):
    tab = lc.table_of(fx, "g1")
    assert emu(0, tab[1], None, [0, 2, 1], bytes(64), 255)[0] == -3
    assert emu(0, tab[1], None, [0, 2], bytes(64), 255)[0] == -3               # offsets[k] past the table without indices
    assert emu(0, tab[1], [0, 0], [0, 2], bytes(64), 255)[:3] == (0, bytes(96), bytes([2]))      # through indices it runs: zero scalars
