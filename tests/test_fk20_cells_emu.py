"""The cell-proof call executed on the CPU under the bounds tracker (tests/host_emu/fk20cells.cpp walks csrc/fk20cells.hpp's lane bodies, with
those of fk20.hpp, frntt.hpp and p1ntt.hpp between them, in the host call's order, the setup included): every case of
tests/golden/fk20_cells.json byte for byte, forced passes, the cell == 1 handle against fk20_setup_create's, the slot-major order of the
handle, and what the fixture itself must hold.  Beyond the fixture (tests/fk20_levels_cases.py, expected images from the C oracle's [a]G of
tests/fk20_scalars.py's scalars): cells of 16 to 512 points, where the sum runs two and three levels, sums_n64 with equal, opposite and
infinite level-0 results, and the Fr transform forced into two passes."""
import ctypes
import os
import subprocess

import pytest

import fk20_cases as k1
import fk20_cells_cases as kc
import fk20_levels_cases as lc
import frntt_cases as fc
import g1_images as gi

HERE = os.path.dirname(os.path.abspath(__file__))
R = kc.R
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_fk20cells.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libfk20cells.so"))
    cp = ctypes.c_char_p
    L.emu_fk20c.argtypes = [cp, SZ, SZ, SZ, cp, SZ, U32, SZ, U32, cp, cp, ctypes.POINTER(SZ), ctypes.POINTER(SZ)]
    L.emu_fk20c_setup.argtypes = [cp, SZ, SZ, ctypes.c_int, cp]
    return L


def run_tiled(lib, setup, n, cell, ext, polys, flags, forced=0, tile=0):
    """tile: the log2 mi355_bls_debug_frntt_set_tile would set (0: the plan's own) -> (..., the passes the Fr transform took)"""
    k = len(polys) // (n * 32)
    q = n // cell
    per = q if flags & kc.H else q << ext
    out, st = ctypes.create_string_buffer(k * per * 96), ctypes.create_string_buffer(k)
    passes, fr_passes = SZ(), SZ()
    rc = lib.emu_fk20c(setup, n, cell, ext, polys, k, flags, forced, tile, out, st, ctypes.byref(passes), ctypes.byref(fr_passes))
    return rc, out.raw, st.raw, passes.value, fr_passes.value


def run(lib, setup, n, cell, ext, polys, flags, forced=0):
    return run_tiled(lib, setup, n, cell, ext, polys, flags, forced)[:4]


def handle(lib, srs, n, cell, plain=0):
    out = ctypes.create_string_buffer(2 * n * 96)
    assert lib.emu_fk20c_setup(srs, n, cell, plain, out) == 0
    return out.raw


def test_fixture_holds_what_the_tests_speak_of():
    assert os.path.getsize(os.path.join(HERE, "golden", "fk20_cells.json")) < 150 << 10            # near fk20.json's size: distinct images once
    fx = kc.fixture()
    assert int(fx["r"], 16) == R and kc.TAU == k1.TAU
    by = {c["name"]: c for c in fx["cases"]}
    for cell in (1, 2, 4, 8, 16):
        for ext in (0, 1):
            c = by["n16_l%d_x%d" % (cell, ext)]
            assert (c["n"], c["k"], c["cell"], c["ext"]) == (16, 3, cell, ext) and sorted(c["out"]) == ["0", "2", "4"]
            for f in ("0", "2", "4"):
                assert len(c["out"][f]) == 2 * 96 * 3 * kc.per_poly(c, int(f))
    # cell 1, ext 0 is the all-openings call on the same inputs: fk20.json's case, image for image
    old, new = k1.case("n16_k3"), by["n16_l1_x0"]
    assert (old["setup"], old["polys"]) == (new["setup"], new["polys"]) and old["out"] == new["out"]
    for ext in (0, 1):                                                       # l = 16: all infinity; l = 8: h_0 alone
        assert set(kc.rows(bytes.fromhex(by["n16_l16_x%d" % ext]["out"]["0"]))) == {kc.INF}
        hs = kc.rows(bytes.fromhex(by["n16_l8_x%d" % ext]["out"]["4"]))
        assert all(hs[2 * g] != kc.INF and hs[2 * g + 1] == kc.INF for g in range(3))
    c = by["wide_n16"]
    assert (c["n"], c["cell"], c["ext"], c["k"]) == (16, 4, 2, 2) and sorted(c["out"]) == ["0", "2"] and (16 // 4) << 2 > 2 * (16 // 4)
    c = by["n64_l8_x1"]
    assert (c["n"], c["cell"], c["ext"], c["k"]) == (64, 8, 1, 2) and sorted(c["out"]) == ["2", "4"]
    c = by["special_n16"]
    n, cell, v = 16, 4, kc.coefficients(c)
    big = (n // cell) << 1
    assert (c["cell"], c["ext"]) == (4, 1) and sorted(c["out"]) == ["0", "4"] and c["status"] == [0] * 5 + [2, 2]
    assert v[0] == [0] * n and all(v[1][:cell]) and v[1][cell:] == [0] * (n - cell) and v[2][:n - 1] == [0] * (n - 1) and v[2][n - 1]
    a = pow(fc.omega(big), 3, R)                                               # divisible by X^l - a: zero on the whole coset x^l = a
    assert all(sum(b * pow(fc.omega(cell * big), (3 + big * u) * j, R) for j, b in enumerate(v[3])) % R == 0 for u in range(cell))
    assert pow(pow(fc.omega(cell * big), 3, R), cell, R) == a
    assert sum(v[4][i + 2 * cell] * pow(kc.TAU, i, R) for i in range(n - 2 * cell)) % R == 0
    assert all(R <= b < 1 << 256 for b in v[5]) and v[6][2] == (1 << 256) - 1
    proofs, hs = kc.rows(bytes.fromhex(c["out"]["0"])), kc.rows(bytes.fromhex(c["out"]["4"]))
    assert set(proofs[:2 * big]) == {kc.INF} and set(hs[:2 * 4]) == {kc.INF}         # the zero polynomial and the one of degree < l
    assert hs[4 * 4 + 1] == kc.INF and hs[4 * 4] != kc.INF                           # the hole in h
    assert proofs[3 * big + 3] != kc.INF
    c = by["sums_n16"]
    s = kc.rows(bytes.fromhex(c["setup"]))
    assert (c["cell"], c["ext"], c["k"]) == (4, 1, 3) and sorted(c["out"]) == ["0", "2", "4"]
    assert all(s[4 * u + 1] == s[4 * u] for u in range(4)) and s[8] == s[9] == kc.INF and kc.INF not in s[:8] + s[10:]
    assert all(s[4 * u + 3][:48] == s[4 * u + 2][:48] and s[4 * u + 3][48:] != s[4 * u + 2][48:] for u in range(4))      # the same x, the other y
    v = kc.coefficients(c)
    assert all(p[4 * u] == p[4 * u + 1] and p[4 * u + 2] == p[4 * u + 3] for p in v for u in range(4))
    assert all(v[0]) and all(v[1][4 * u] and not v[1][4 * u + 2] for u in range(4)) and all(v[2][4 * u + 2] and not v[2][4 * u] for u in range(4))
    assert all(set(kc.rows(bytes.fromhex(c["out"][f]))[-kc.per_poly(c, int(f)):]) == {kc.INF} for f in c["out"])          # polynomial 2: all infinity
    assert kc.INF not in kc.rows(bytes.fromhex(c["out"]["0"]))[:2 * 8]
    for cs in fx["cases"]:                                                      # h_(q-1) is infinity in every H output
        if "4" in cs["out"]:
            q = cs["n"] // cs["cell"]
            h_rows = kc.rows(bytes.fromhex(cs["out"]["4"]))
            assert all(h_rows[g * q + q - 1] == kc.INF for g in range(cs["k"]))


def test_every_case_of_the_fixture(lib):
    for name, n, k, cell, ext, flags, setup, polys, want, status in kc.cases():
        rc, got, st, passes = run(lib, setup, n, cell, ext, polys, flags)
        assert passes == 1 and st == status and rc == sum(1 for b in status if b), (name, flags)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
            assert a == b, (name, flags, i)


def test_forced_passes_give_the_same_bytes(lib):
    for name, n, k, cell, ext, flags, setup, polys, want, status in kc.cases():
        if name in ("n16_l4_x1", "n16_l1_x0", "special_n16"):
            for forced in (1, 2):
                rc, got, st, passes = run(lib, setup, n, cell, ext, polys, flags, forced)
                assert got == want and st == status and passes == -(-k // forced), (name, flags, forced)


def test_cell_1_handle_is_the_all_openings_handle(lib):
    for name in ("n16_l1_x0", "n64_l8_x1"):
        c = kc.case(name)
        srs = bytes.fromhex(c["setup"])
        assert handle(lib, srs, c["n"], 1) == handle(lib, srs, c["n"], 1, plain=1)
    one = kc.rows(bytes.fromhex(kc.case("n16_l1_x0")["setup"]))[:1]
    assert handle(lib, one[0], 1, 1) == handle(lib, one[0], 1, 1, plain=1) == bytes(192)


def test_handle_is_slot_major_over_the_sub_setups(lib):
    """the handle for cells of l points holds, at slot l + v, slot `slot` of the all-openings handle of the sub-setup S_(l u + v); l = 64 is
    the cell whose terms the sum adds in two full levels"""
    for n, cell in ((16, 4), (128, 64)):
        srs = kc.rows(bytes.fromhex(kc.case("n16_l4_x1")["setup"])) if n == 16 else kc.rows(gi.multiples_of_g_cpu(lc.srs_scalars(n)))
        q = n // cell
        got = kc.rows(handle(lib, b"".join(srs), n, cell))
        for v in range(cell):
            sub = kc.rows(handle(lib, b"".join(srs[v::cell]), q, 1, plain=1))
            assert [got[slot * cell + v] for slot in range(2 * q)] == sub, (n, v)
        # and it is no trivial array (q = 2: s^ of a sub-setup is its one point S_v, the transform four copies of it - l distinct images)
        assert len(set(got)) > n if q > 2 else len(set(got)) == cell and kc.INF not in got


def test_refused_by_the_plan(lib):
    c = kc.case("n16_l4_x1")
    srs, polys = bytes.fromhex(c["setup"]), bytes.fromhex(c["polys"])
    out, st = ctypes.create_string_buffer(3 * 16 * 4 * 96), ctypes.create_string_buffer(3)
    for cell, ext in ((0, 0), (3, 0), (32, 0), (4, 29)):
        assert lib.emu_fk20c(srs, 16, cell, ext, polys, 3, 0, 0, 0, out, st, None, None) == -1, (cell, ext)


def expect(got, want_scalars, what):
    """the rows of `got` against [a]G of the expected scalars, row by row"""
    want = gi.multiples_of_g_cpu(list(want_scalars))
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
        assert a == b, (what, i)


@pytest.mark.parametrize("n,cell,ext,k,flag_values", lc.SHAPES, ids=["n%d_l%d_x%d" % c[:3] for c in lc.SHAPES])
def test_sums_of_two_and_three_levels(lib, n, cell, ext, k, flag_values):
    """l >= 16: the levels at strides 8 and 64 store in place in the product array, the last one into the workspace"""
    srs = gi.multiples_of_g_cpu(lc.srs_scalars(n))
    rows, status = lc.polynomials(n, cell, ext, k)
    for flags in flag_values:
        rc, got, st, passes = run(lib, srs, n, cell, ext, lc.pack(rows), flags)
        assert (rc, st, passes) == (1, status, 1), flags
        expect(got, lc.expected(n, cell, ext, k, flags), (n, cell, ext, flags))


def test_forced_passes_and_a_forced_tile_behind_a_two_level_sum(lib):
    n, cell, ext, k = lc.FORCED
    srs = gi.multiples_of_g_cpu(lc.srs_scalars(n))
    rows, status = lc.polynomials(n, cell, ext, k)
    for flags in lc.ALL:
        whole = run(lib, srs, n, cell, ext, lc.pack(rows), flags)
        expect(whole[1], lc.expected(n, cell, ext, k, flags), flags)
        for forced in (1, 2):
            assert run(lib, srs, n, cell, ext, lc.pack(rows), flags, forced) == whole[:3] + (-(-k // forced),), (flags, forced)
        assert run_tiled(lib, srs, n, cell, ext, lc.pack(rows), flags, tile=2) == whole + (2,), flags          # 2q = 8 scalars in tiles of four


def test_fr_transform_in_two_passes_gives_the_same_bytes(lib):
    """a tile of four elements: the 2q = 8 or 16 scalars of a vector take two passes, in place in the scalar array as fk20_cells_run drives
    them; by default every fixture case takes one"""
    seen = set()
    for name, n, k, cell, ext, flags, setup, polys, want, status in kc.cases():
        if name in ("n16_l4_x1", "wide_n16", "n64_l8_x1", "special_n16"):
            assert run_tiled(lib, setup, n, cell, ext, polys, flags)[4] == 1
            rc, got, st, passes, fr_passes = run_tiled(lib, setup, n, cell, ext, polys, flags, tile=2)
            assert fr_passes == 2 and passes == 1 and st == status and rc == sum(1 for b in status if b), (name, flags)
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
                assert a == b, (name, flags, i)
            seen.add((name, flags))
    assert len(seen) == 3 + 2 + 2 + 2


@pytest.mark.parametrize("name", sorted(lc.sums_n64()))
def test_sums_n64(lib, name):
    """n = 64, l = 16, no SRS: the second level adds two equal results (a doubling), two opposite ones, a result and infinity, and two
    infinities - each in every slot (tests/fk20_levels_cases.py sums_n64)"""
    n, cell, ext = lc.SUMS
    s, polys, kinds = lc.sums_n64()[name]
    setup = gi.multiples_of_g_cpu(s)
    for flags in lc.ALL:
        want = lc.sums_expected(name, flags)
        rc, got, st, passes = run(lib, setup, n, cell, ext, lc.pack(polys), flags)
        assert (rc, st, passes) == (0, bytes(len(polys)), 1), flags
        expect(got, want, (name, flags))
        per = len(want) // len(polys)
        for g, kind in enumerate(kinds):                                      # the structure, on the images that came out
            mine = kc.rows(got)[g * per:(g + 1) * per]
            assert (set(mine) == {kc.INF}) == (kind == "infinity"), (name, flags, g)
            if kind == "finite":
                assert [i for i, r in enumerate(mine) if r == kc.INF] == ([per - 1] if flags & kc.H else []), (name, flags, g)
