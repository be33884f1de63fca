"""The all-openings call executed on the CPU under the bounds tracker (tests/host_emu/fk20.cpp walks csrc/fk20.hpp's lane bodies, with those
of frntt.hpp and p1ntt.hpp between them, in the host call's order, the setup included): every case of tests/golden/fk20.json up to n = 16
byte for byte, forced passes, the Fr transform forced into two and three passes, the circulant layout against a Python list, the reversed setup, and h_(n-1) as an infinity that the complete
additions produce."""
import ctypes
import os
import subprocess

import pytest

import fk20_cases as kc
import frntt_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
R = kc.R
SZ = ctypes.c_size_t
U32, U64 = ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_fk20.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libfk20.so"))
    cp = ctypes.c_char_p
    L.emu_fk20.argtypes = [cp, SZ, cp, SZ, U32, SZ, U32, cp, cp, ctypes.POINTER(SZ), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(SZ)]
    L.emu_fk20_circ.argtypes = [cp, SZ, cp]
    L.emu_fk20_circ.restype = None
    L.emu_fk20_setup_src.argtypes = [U64, U64]
    L.emu_fk20_setup_src.restype = ctypes.c_int64
    L.emu_fk20_at.argtypes = [U32, U64]
    L.emu_fk20_at.restype = U64
    return L


def run_tiled(lib, setup, n, polys, flags, forced=0, tile=0):
    """tile: the log2 mi355_bls_debug_frntt_set_tile would set (0: the plan's own) -> (..., the passes the Fr transform took)"""
    k = len(polys) // (n * 32)
    out, st = ctypes.create_string_buffer(k * n * 96), ctypes.create_string_buffer(k)
    passes, z, fr_passes = SZ(), ctypes.c_int(), SZ()
    rc = lib.emu_fk20(setup, n, polys, k, flags, forced, tile, out, st, ctypes.byref(passes), ctypes.byref(z), ctypes.byref(fr_passes))
    return rc, out.raw, st.raw, passes.value, z.value, fr_passes.value


def run(lib, setup, n, polys, flags, forced=0):
    return run_tiled(lib, setup, n, polys, flags, forced)[:5]


def test_fixture_holds_what_the_tests_speak_of():
    assert os.path.getsize(os.path.join(HERE, "golden", "fk20.json")) < 200 << 10
    fx = kc.fixture()
    assert int(fx["r"], 16) == R and pow(kc.TAU, 64, R) != 1
    by = {c["name"]: c for c in fx["cases"]}
    for n in (1, 2, 4, 8, 16):
        c = by["n%d_k3" % n]
        assert (c["n"], c["k"]) == (n, 3) and sorted(c["out"]) == ["0", "2", "4"]
    assert (by["n64_k1"]["n"], by["n64_k1"]["k"]) == (64, 1) and sorted(by["n64_k1"]["out"]) == ["0", "4"]
    assert sorted(by["linear_n8"]["out"]) == ["0", "2", "4"] and kc.rows(bytes.fromhex(by["linear_n8"]["setup"]))[5] == bytes(96)
    c = by["special_n8"]
    n, v = 8, kc.coefficients(c)
    assert sorted(c["out"]) == ["0", "4"] and c["status"] == [0] * 6 + [2, 2]
    assert v[0] == [0] * n and v[1][0] and v[1][1:] == [0] * (n - 1) and v[2][:n - 1] == [0] * (n - 1) and v[2][n - 1] and v[3][n - 1] == 0 and all(v[3][:n - 1])
    assert sum(a * pow(fc.omega(n), 3 * j, R) for j, a in enumerate(v[4])) % R == 0
    assert sum(v[5][i + 3] * pow(kc.TAU, i, R) for i in range(n - 3)) % R == 0
    assert all(R <= a < 1 << 256 for a in v[6]) and v[7][2] == (1 << 256) - 1
    proofs, hs = kc.rows(bytes.fromhex(c["out"]["0"])), kc.rows(bytes.fromhex(c["out"]["4"]))
    assert proofs[:2 * n] == [bytes(96)] * (2 * n) and hs[:2 * n] == [bytes(96)] * (2 * n)          # the zero and the constant polynomial
    assert hs[5 * n + 2] == bytes(96) and hs[5 * n + 1] != bytes(96)                             # the hole in h
    assert proofs[4 * n + 3] != bytes(96)                                                     # a root of p is no root of its quotient
    for cs in fx["cases"]:                                                                    # h_(n-1) is infinity in every H output
        h_rows = kc.rows(bytes.fromhex(cs["out"]["4"]))
        assert all(h_rows[g * cs["n"] + cs["n"] - 1] == bytes(96) for g in range(cs["k"]))
    assert by["n1_k3"]["out"]["0"] == bytes(3 * 96).hex()                                      # n = 1: every output is infinity


def test_every_case_of_the_fixture_up_to_16(lib):
    for name, n, k, flags, setup, polys, want, status in kc.cases():
        if n > 16:
            continue
        rc, got, st, passes, z = run(lib, setup, n, polys, flags)
        assert passes == 1 and st == status and rc == sum(1 for b in status if b), (name, flags)
        assert z == 1, (name, flags)
        for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
            assert a == b, (name, flags, i)


def test_forced_passes_give_the_same_bytes(lib):
    for name, n, k, flags, setup, polys, want, status in kc.cases():
        if k == 3 and n in (1, 4):
            for forced in (1, 2):
                rc, got, st, passes, _ = run(lib, setup, n, polys, flags, forced)
                assert got == want and st == status and passes == -(-k // forced), (name, flags, forced)


def test_fr_transform_in_more_than_one_pass_gives_the_same_bytes(lib):
    """a tile of four elements: the 2n scalars of a polynomial take two passes at n = 8 and three at n = 16, in place in the scalar array as
    fk20_run drives them; by default every fixture case takes one"""
    seen = set()
    for name, n, k, flags, setup, polys, want, status in kc.cases():
        if name in ("n8_k3", "n16_k3", "special_n8"):
            assert run_tiled(lib, setup, n, polys, flags)[5] == 1
            rc, got, st, passes, z, fr_passes = run_tiled(lib, setup, n, polys, flags, tile=2)
            assert fr_passes == -(-(n.bit_length()) // 2) >= 2 and passes == 1, (name, flags)
            assert st == status and rc == sum(1 for b in status if b) and z == 1, (name, flags)
            for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
                assert a == b, (name, flags, i)
            seen.add((name, flags))
    assert len(seen) == 3 + 3 + 2


def test_h_last_is_infinity_out_of_the_complete_addition(lib):
    """entry n - 1 of the inverse transform is a sum of points that cancel - no lane writes a zero there: the emulation reports the Z the
    last DIT stage left in the workspace, and the H output shows it as the all-zero image"""
    c = kc.case("n8_k3")
    rc, got, _, _, z = run(lib, bytes.fromhex(c["setup"]), 8, bytes.fromhex(c["polys"]), kc.H)
    assert rc == 0 and z == 1
    h_rows = kc.rows(got)
    for g in range(3):
        assert h_rows[g * 8 + 7] == bytes(96) and all(r != bytes(96) for r in h_rows[g * 8:g * 8 + 7])


def test_circulant_layout_against_a_python_list(lib):
    for name in ("n1_k3", "n2_k3", "n4_k3", "n8_k3", "n16_k3", "n64_k1", "special_n8"):
        c = kc.case(name)
        n = c["n"]
        for row in kc.coefficients(c):
            out = ctypes.create_string_buffer(2 * n * 32)
            lib.emu_fk20_circ(fc.pack([row]), n, out)
            assert fc.images(out.raw) == kc.circulant([a % R for a in row]), name


def test_setup_is_reversed_and_zero_extended(lib):
    for n in (1, 2, 4, 8, 64):
        got = [lib.emu_fk20_setup_src(n, u) for u in range(2 * n)]
        assert got == [n - 2 - u for u in range(n - 1)] + [-1] * (n + 1)
    for m in range(0, 5):
        n = 1 << m
        assert [lib.emu_fk20_at(m, e) for e in range(3 * n)] == [g * 2 * n + j for g in range(3) for j in range(n)]
