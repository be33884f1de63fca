"""The proofs of all cells of k polynomials on the device (mi355_bls_fk20_open_cells_many, host and device form): every case of
tests/golden/fk20_cells.json byte for byte with its status bytes and return count, cell 1 / ext 0 against mi355_bls_fk20_open_all_many on
the same inputs, the cell == 1 handle, the output on a caller's stream, k = 5 in three passes, k = 0, and every refusal of the C entry
points that needs a context - a cells handle given to open_all_many among them.  The CPU half is tests/test_fk20_cells_emu.py."""
import ctypes
import functools

import pytest

import fk20_cells_cases as kc
import fk20_levels_cases as lc
import g1_images as gi

pytestmark = pytest.mark.gpu
ROW = kc.ROW
GUARD = 96


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setups(m, cache):
    """one handle per distinct (setup, cell) of the fixture, made by the host form; released at the end"""
    made = {}

    @functools.lru_cache(maxsize=None)
    def get(images, cell):
        made[images, cell] = m.fk20_setup_create_cells(cache, images, cell)
        return made[images, cell]
    yield get
    for s in made.values():
        m.fk20_setup_destroy(s)


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def both_forms(m, cache, setup, polys, ext, flags=0, stream=0):
    """the host form and the device form (a 0xaa guard band behind the output; the polynomials untouched) -> (count, images, status)"""
    import torch
    n = setup.n
    k = len(polys) // (32 * n)
    size = k * m.fk20_cells_rows(setup, ext, flags) * ROW
    rc, out, st = m.fk20OpenCellsMany(cache, setup, polys, ext, flags)
    d_polys = dev(polys)
    d_out = torch.full((size + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc_d, st_d = m.fk20OpenCellsMany_device(cache, setup, d_polys.data_ptr(), k, d_out.data_ptr(), ext, flags, stream=stream)
    ho = host(d_out)
    assert len(out) == size and ho[size:] == b"\xaa" * GUARD and host(d_polys) == polys
    assert (rc_d, st_d, ho[:size]) == (rc, st, out)
    return rc, out, st


def test_every_case_of_the_fixture(m, cache, setups):
    for name, n, k, cell, ext, flags, setup, polys, want, status in kc.cases():
        rc, got, st = both_forms(m, cache, setups(setup, cell), polys, ext, flags)
        assert st == status and rc == sum(1 for b in status if b), (name, flags)
        assert len(got) == len(want), (name, flags)
        for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
            assert a == b, (name, flags, i)


def test_cell_1_ext_0_is_open_all_many(m, cache, setups):
    """the same inputs through both calls, and through each call with the other's cell == 1 handle: the same bytes"""
    c = kc.case("n16_l1_x0")
    srs, polys = bytes.fromhex(c["setup"]), bytes.fromhex(c["polys"])
    plain = m.fk20_setup_create(cache, srs)
    try:
        for flags in (0, kc.BITREV, kc.H):
            old = m.fk20OpenAllMany(cache, plain, polys, flags)
            assert old[1] == bytes.fromhex(c["out"][str(flags)])
            assert m.fk20OpenCellsMany(cache, setups(srs, 1), polys, 0, flags) == old
            assert m.fk20OpenCellsMany(cache, plain, polys, 0, flags) == old
            assert m.fk20OpenAllMany(cache, setups(srs, 1), polys, flags) == old
    finally:
        m.fk20_setup_destroy(plain)


def test_setup_made_from_device_memory_gives_the_same_proofs(m, cache):
    c = kc.case("n16_l4_x1")
    d_srs = dev(bytes.fromhex(c["setup"]))
    s = m.fk20_setup_create_cells_device(cache, d_srs.data_ptr(), 16, 4)
    try:
        assert host(d_srs) == bytes.fromhex(c["setup"]) and (s.n, s.cell) == (16, 4)
        for f in ("0", "2", "4"):
            assert both_forms(m, cache, s, bytes.fromhex(c["polys"]), 1, int(f))[1] == bytes.fromhex(c["out"][f])
    finally:
        m.fk20_setup_destroy(s)


def test_output_on_a_callers_stream(m, cache, setups):
    """the device form on a stream of the caller's, the setup made on that stream too: the same bytes; the call returns with its pass done"""
    import torch
    st = torch.cuda.Stream()
    for name, flags in (("n16_l4_x1", 0), ("wide_n16", kc.BITREV), ("n64_l8_x1", kc.H)):
        c = kc.case(name)
        d_srs = dev(bytes.fromhex(c["setup"]))
        torch.cuda.synchronize()
        s = m.fk20_setup_create_cells_device(cache, d_srs.data_ptr(), c["n"], c["cell"], stream=st.cuda_stream)
        try:
            got = both_forms(m, cache, s, bytes.fromhex(c["polys"]), c["ext"], flags, stream=st.cuda_stream)
            assert got == (0, bytes.fromhex(c["out"][str(flags)]), bytes(c["k"])), name
        finally:
            m.fk20_setup_destroy(s)


def test_five_polynomials_in_three_passes(m, cache, setups):
    """k = 5 with the pass hook at 2: passes of 2, 2 and 1; images and status bytes land at their polynomials"""
    c = kc.case("special_n16")
    s = setups(bytes.fromhex(c["setup"]), 4)
    pick = (5, 1, 6, 3, 4)                                                     # status 2, 0 | 2, 0 | 0
    per = 16 * 32
    polys = b"".join(bytes.fromhex(c["polys"])[g * per:(g + 1) * per] for g in pick)
    try:
        m.debug_fk20_set_pass(cache, 2)
        for f in (0, kc.H):
            size = kc.per_poly(c, f) * ROW
            want = b"".join(bytes.fromhex(c["out"][str(f)])[g * size:(g + 1) * size] for g in pick)
            assert both_forms(m, cache, s, polys, 1, f) == (2, want, bytes([2, 0, 2, 0, 0])), f
    finally:
        m.debug_fk20_set_pass(cache, 0)


def test_k_zero_touches_nothing(m, cache, setups):
    import torch
    s = setups(bytes.fromhex(kc.case("n16_l4_x1")["setup"]), 4)
    L, h = m.lib(), cache._h
    out = ctypes.create_string_buffer(b"\x5a" * ROW, ROW)
    assert L.mi355_bls_fk20_open_cells_many(h, s._h, bytes(32), 0, 1, 0, out, None) == 0 and out.raw == b"\x5a" * ROW
    assert L.mi355_bls_fk20_open_cells_many(h, None, None, 0, 99, 99, None, None) == 0            # k == 0 touches nothing, looks at nothing
    d = torch.full((4 * ROW,), 0x5a, dtype=torch.uint8, device="cuda")
    assert L.mi355_bls_fk20_open_cells_many_device(h, s._h, d.data_ptr(), 0, 1, 0, d.data_ptr(), None, None) == 0 and host(d) == b"\x5a" * 4 * ROW
    assert m.fk20OpenCellsMany(cache, s, b"", 1) == (0, b"", b"")


def test_edges_cell_n_and_n_1(m, cache):
    """cell == n: q = 1 and every output is infinity, on every extension; n == 1 likewise"""
    c = kc.case("n16_l16_x1")
    srs, polys = bytes.fromhex(c["setup"]), bytes.fromhex(c["polys"])
    for images, n, ext in ((srs, 16, 0), (srs, 16, 3), (srs[:96], 1, 0), (srs[:96], 1, 2)):
        s = m.fk20_setup_create_cells(cache, images, n)
        try:
            p = polys[:2 * n * 32]
            assert both_forms(m, cache, s, p, ext, 0) == (0, bytes(2 * ROW << ext), bytes(2)), (n, ext)
            assert both_forms(m, cache, s, p, ext, kc.H) == (0, bytes(2 * ROW), bytes(2)), (n, ext)
        finally:
            m.fk20_setup_destroy(s)


def test_argument_errors_with_a_context(m, cache, setups):
    """MI355_BLS_ERR_ARG (-3) from the C entry points themselves; nothing is written and no handle is made"""
    import torch
    L, h = m.lib(), cache._h
    srs = bytes.fromhex(kc.case("n16_l4_x1")["setup"])
    s = setups(srs, 4)
    polys = bytes(16 * 32)
    out = ctypes.create_string_buffer(b"\x5a" * 8 * ROW, 8 * ROW)
    for case in (dict(setup=None), dict(polys=None), dict(out=None), dict(flags=1), dict(flags=8), dict(flags=0x80000002), dict(ext=29), dict(ext=64),
                 dict(ext=(1 << 64) - 1), dict(ext=29, flags=kc.H)):
        a = dict(setup=s._h, polys=polys, flags=0, out=out, ext=1)
        a.update(case)
        assert L.mi355_bls_fk20_open_cells_many(h, a["setup"], a["polys"], 1, a["ext"], a["flags"], a["out"], None) == -3, case
    d = torch.full((ROW * 8 + 8,), 0x5a, dtype=torch.uint8, device="cuda")
    dp = torch.zeros((32 * 16 + 8,), dtype=torch.uint8, device="cuda")
    before = host(d)
    P, Q = dp.data_ptr(), d.data_ptr()
    call = lambda pi, po, setup=s._h, flags=0, ext=1: L.mi355_bls_fk20_open_cells_many_device(h, setup, pi, 1, ext, flags, po, None, None)      # noqa: E731
    assert call(P + 1, Q) == -3 and call(P, Q + 2) == -3 and call(None, Q) == -3 and call(P, None) == -3 and call(P, Q, setup=None) == -3
    assert call(P, Q, flags=16) == -3 and call(P, Q, ext=29) == -3
    hd = ctypes.c_void_p()
    for n, cell in ((0, 1), (3, 1), (6, 2), ((1 << 31) + 1, 1), (1 << 32, 1), (16, 0), (16, 3), (16, 6), (16, 32), (8, 16), (1, 2)):
        assert L.mi355_bls_fk20_setup_create_cells(h, ctypes.byref(hd), srs, n, cell) == -3 and not hd.value, (n, cell)
        assert L.mi355_bls_fk20_setup_create_cells_device(h, ctypes.byref(hd), Q, n, cell, None) == -3 and not hd.value, (n, cell)
    assert L.mi355_bls_fk20_setup_create_cells(h, None, srs, 16, 4) == -3 and L.mi355_bls_fk20_setup_create_cells(h, ctypes.byref(hd), None, 16, 4) == -3
    assert L.mi355_bls_fk20_setup_create_cells_device(h, ctypes.byref(hd), None, 16, 4, None) == -3
    assert L.mi355_bls_fk20_setup_create_cells_device(h, ctypes.byref(hd), Q + 1, 1, 1, None) == -3 and not hd.value
    assert host(d) == before and out.raw == b"\x5a" * 8 * ROW
    assert call(P + 4, Q + 4) == 0 and host(d)[4:4 + 8 * ROW] == bytes(8 * ROW)                   # aligned to 4 bytes, not to 16; the zero polynomial


def test_a_cells_handle_is_refused_by_open_all_many(m, cache, setups):
    import torch
    L, h = m.lib(), cache._h
    c = kc.case("n16_l4_x1")
    s = setups(bytes.fromhex(c["setup"]), 4)
    out = ctypes.create_string_buffer(b"\x5a" * 16 * ROW, 16 * ROW)
    assert L.mi355_bls_fk20_open_all_many(h, s._h, bytes(16 * 32), 1, 0, out, None) == -3 and out.raw == b"\x5a" * 16 * ROW
    assert b"made for cells" in L.mi355_bls_last_error()
    d = torch.full((16 * ROW,), 0x5a, dtype=torch.uint8, device="cuda")
    dp = torch.zeros((16 * 32,), dtype=torch.uint8, device="cuda")
    assert L.mi355_bls_fk20_open_all_many_device(h, s._h, dp.data_ptr(), 1, 0, d.data_ptr(), None, None) == -3 and host(d) == b"\x5a" * 16 * ROW
    with pytest.raises(Exception):
        m.fk20OpenAllMany(cache, s, bytes(16 * 32))
    assert L.mi355_bls_fk20_open_all_many(h, s._h, None, 0, 0, None, None) == 0                  # k == 0 still looks at nothing
    assert both_forms(m, cache, s, bytes.fromhex(c["polys"]), 1, 0)[1] == bytes.fromhex(c["out"]["0"])      # and the handle still serves its own call


def test_a_busy_context_is_refused(m, setups):
    """a context with a submitted batch that has not been waited for: -3 before anything is launched, the output untouched"""
    import json
    import os
    import torch
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch.json")))
    case = [c for c in g["cases"] if c["name"] == "n3"][0]
    srs = bytes.fromhex(kc.case("n16_l4_x1")["setup"])
    s = setups(srs, 4)
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        L = m.lib()
        recs = dev(bytes.fromhex(case["sets"]))
        d = torch.full((ROW * 8,), 0x5a, dtype=torch.uint8, device="cuda")
        dp = torch.zeros((32 * 16,), dtype=torch.uint8, device="cuda")
        out = ctypes.create_string_buffer(b"\x5a" * 8 * ROW, 8 * ROW)
        hd = ctypes.c_void_p()
        c.submit_device(recs.data_ptr(), case["n"], bytes.fromhex(case["rnd"]))
        assert L.mi355_bls_fk20_open_cells_many_device(c._h, s._h, dp.data_ptr(), 1, 1, 0, d.data_ptr(), None, None) == -3
        assert L.mi355_bls_fk20_open_cells_many(c._h, s._h, bytes(16 * 32), 1, 1, 0, out, None) == -3
        assert b"not been waited for" in L.mi355_bls_last_error()
        assert L.mi355_bls_fk20_setup_create_cells(c._h, ctypes.byref(hd), srs, 16, 4) == -3 and not hd.value
        assert c.wait() is True
        assert host(d) == out.raw == b"\x5a" * 8 * ROW
        assert L.mi355_bls_fk20_open_cells_many(c._h, s._h, bytes(16 * 32), 1, 1, 0, out, None) == 0 and out.raw == bytes(8 * ROW)
    finally:
        c.close()


# ---- beyond the fixture: expected images from scalars
@pytest.fixture(scope="module")
def images(m, cache):
    """[a]G for a tuple of scalars, each tuple once"""
    @functools.lru_cache(maxsize=None)
    def get(scalars):
        return gi.multiples_of_g(m, cache, list(scalars))
    return get


@pytest.fixture(scope="module")
def srs_setups(m, cache, images):
    """a cells handle over [tau^i]G, the SRS made on the device and handed over there; released at the end"""
    made = {}

    def get(n, cell):
        if (n, cell) not in made:
            d_srs = dev(images(lc.srs_scalars(n)))
            made[n, cell] = m.fk20_setup_create_cells_device(cache, d_srs.data_ptr(), n, cell)
        return made[n, cell]
    yield get
    for s in made.values():
        m.fk20_setup_destroy(s)


def expect(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
        assert a == b, (what, i)


@pytest.mark.parametrize("n,cell,ext,k,flag_values", lc.SHAPES, ids=["n%d_l%d_x%d" % c[:3] for c in lc.SHAPES])
def test_sums_of_two_and_three_levels(m, cache, images, srs_setups, n, cell, ext, k, flag_values):
    """l >= 16: the levels at strides 8 and 64 store in place in the product array, the last one into the workspace"""
    rows, status = lc.polynomials(n, cell, ext, k)
    for flags in flag_values:
        rc, got, st = both_forms(m, cache, srs_setups(n, cell), lc.pack(rows), ext, flags)
        assert (rc, st) == (1, status), flags
        expect(got, images(lc.expected(n, cell, ext, k, flags)), (n, cell, ext, flags))


def test_forced_passes_and_a_forced_tile_behind_a_two_level_sum(m, cache, images, srs_setups):
    n, cell, ext, k = lc.FORCED
    rows, status = lc.polynomials(n, cell, ext, k)
    s = srs_setups(n, cell)
    for flags in lc.ALL:
        want = (1, images(lc.expected(n, cell, ext, k, flags)), status)
        for forced in (1, 2):
            try:
                m.debug_fk20_set_pass(cache, forced)
                assert both_forms(m, cache, s, lc.pack(rows), ext, flags) == want, (flags, forced)
            finally:
                m.debug_fk20_set_pass(cache, 0)
        try:
            m.debug_frntt_set_tile(cache, 2)                                  # 2q = 8 scalars in tiles of four: two passes
            assert both_forms(m, cache, s, lc.pack(rows), ext, flags) == want, flags
        finally:
            m.debug_frntt_set_tile(cache, 0)


def test_fr_transform_in_two_passes_gives_the_same_bytes(m, cache, setups):
    """a tile of four elements: the 2q = 8 or 16 scalars of a vector take two passes, in place in the scalar array"""
    seen = set()
    try:
        m.debug_frntt_set_tile(cache, 2)
        for name, n, k, cell, ext, flags, setup, polys, want, status in kc.cases():
            if name in ("n16_l4_x1", "wide_n16", "n64_l8_x1", "special_n16"):
                rc, got, st = both_forms(m, cache, setups(setup, cell), polys, ext, flags)
                assert st == status and rc == sum(1 for b in status if b), (name, flags)
                expect(got, want, (name, flags))
                seen.add((name, flags))
    finally:
        m.debug_frntt_set_tile(cache, 0)
    assert len(seen) == 3 + 2 + 2 + 2


def test_fr_transform_in_two_passes_at_the_default_tile(m, cache, images, srs_setups):
    """n = 2048 in cells of 2 points: 2q = 2048 scalars per vector, two vectors per polynomial"""
    n, cell, ext = 2048, 2, 0
    assert 2 * (n // cell) > lc.fr_tile()
    rows, status = lc.polynomials(n, cell, ext, 1)
    for flags in (kc.BITREV, kc.H):
        rc, got, st = both_forms(m, cache, srs_setups(n, cell), lc.pack(rows), ext, flags)
        assert (rc, st) == (1, status), flags
        expect(got, images(lc.expected(n, cell, ext, 1, flags)), flags)


@pytest.mark.parametrize("name", sorted(lc.sums_n64()))
def test_sums_n64(m, cache, images, name):
    """n = 64, l = 16, no SRS: the second level adds two equal results (a doubling), two opposite ones, a result and infinity, and two
    infinities - each in every slot (tests/fk20_levels_cases.py sums_n64)"""
    n, cell, ext = lc.SUMS
    s, polys, kinds = lc.sums_n64()[name]
    setup = m.fk20_setup_create_cells(cache, images(tuple(s)), cell)
    try:
        for flags in lc.ALL:
            want = images(lc.sums_expected(name, flags))
            rc, got, st = both_forms(m, cache, setup, lc.pack(polys), ext, flags)
            assert (rc, st) == (0, bytes(len(polys))), flags
            expect(got, want, (name, flags))
            per = len(want) // ROW // len(polys)
            for g, kind in enumerate(kinds):                                  # the structure, on the images that came out
                mine = kc.rows(got)[g * per:(g + 1) * per]
                assert (set(mine) == {kc.INF}) == (kind == "infinity"), (name, flags, g)
                if kind == "finite":
                    assert [i for i, r in enumerate(mine) if r == kc.INF] == ([per - 1] if flags & kc.H else []), (name, flags, g)
    finally:
        m.fk20_setup_destroy(setup)


def test_finish_with_a_shared_inversion(m, cache, setups):
    """k = 4097 polynomials of n64_l8_x1, its two cycled: 65 552 cells, more than TOAFF_DEVICE_LANES, so a lane of k_fk20c_finish inverts
    once for two neighbouring cells"""
    c = kc.case("n64_l8_x1")
    k, per = 4097, kc.per_poly(c, kc.BITREV)
    assert k * per > lc.toaff_device_lanes() and k * per <= 2 * lc.toaff_device_lanes()
    size = c["n"] * 32
    polys = [bytes.fromhex(c["polys"])[g * size:(g + 1) * size] for g in range(2)]
    out = [bytes.fromhex(c["out"]["2"])[g * per * ROW:(g + 1) * per * ROW] for g in range(2)]
    assert kc.INF not in kc.rows(out[0] + out[1]) and out[0] != out[1]
    rc, got, st = both_forms(m, cache, setups(bytes.fromhex(c["setup"]), 8), lc.cycled(polys, k), 1, kc.BITREV)
    assert (rc, st) == (0, bytes(k))
    want = lc.cycled(out, k)
    assert got == want, [i for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))) if a != b][:8]
