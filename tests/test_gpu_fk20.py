"""All openings of k polynomials on the device (mi355_bls_fk20_open_all_many, host and device form): every case of tests/golden/fk20.json
byte for byte with its status bytes and return count, forced passes, a setup made through one context and used through another, k = 0,
destroy of NULL, and the argument errors of the C entry points.  Beyond the fixture (expected images are [a]G of tests/fk20_scalars.py's
scalars through p1sLincombMany_device): the Fr transform in more than one pass - a forced tile of four, and the default tile at n = 1024 -
and a finish over more than TOAFF_DEVICE_LANES elements, where neighbours share an inversion.  The CPU half is tests/test_fk20_emu.py."""
import ctypes
import functools

import pytest

import fk20_cases as kc
import fk20_levels_cases as lc
import fk20_scalars as ks
import frntt_cases as fc
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
    """one handle per distinct setup of the fixture, made by the host form; released at the end"""
    made = {}

    @functools.lru_cache(maxsize=None)
    def get(images):
        made[images] = m.fk20_setup_create(cache, images)
        return made[images]
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


def both_forms(m, cache, setup, polys, flags=0):
    """the host form and the device form (a 0xaa guard band behind the output; the polynomials untouched) -> (count, images, status)"""
    import torch
    n = setup.n
    k = len(polys) // (32 * n)
    rc, out, st = m.fk20OpenAllMany(cache, setup, polys, flags)
    d_polys = dev(polys)
    d_out = torch.full((k * n * ROW + GUARD,), 0xaa, dtype=torch.uint8, device="cuda")
    rc_d, st_d = m.fk20OpenAllMany_device(cache, setup, d_polys.data_ptr(), k, d_out.data_ptr(), flags)
    ho = host(d_out)
    assert ho[k * n * ROW:] == b"\xaa" * GUARD and host(d_polys) == polys
    assert (rc_d, st_d, ho[:k * n * ROW]) == (rc, st, out)
    return rc, out, st


def test_every_case_of_the_fixture(m, cache, setups):
    for name, n, k, flags, setup, polys, want, status in kc.cases():
        rc, got, st = both_forms(m, cache, setups(setup), polys, flags)
        assert st == status and rc == sum(1 for b in status if b), (name, flags)
        for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
            assert a == b, (name, flags, i)


def test_setup_made_from_device_memory_gives_the_same_proofs(m, cache):
    c = kc.case("n16_k3")
    d_srs = dev(bytes.fromhex(c["setup"]))
    s = m.fk20_setup_create_device(cache, d_srs.data_ptr(), 16)
    try:
        assert host(d_srs) == bytes.fromhex(c["setup"])
        for f in ("0", "2", "4"):
            assert both_forms(m, cache, s, bytes.fromhex(c["polys"]), int(f))[1] == bytes.fromhex(c["out"][f])
    finally:
        m.fk20_setup_destroy(s)


def test_forced_passes_give_the_same_bytes(m, cache, setups):
    for name in ("n1_k3", "n8_k3"):
        c = kc.case(name)
        s, polys = setups(bytes.fromhex(c["setup"])), bytes.fromhex(c["polys"])
        for f in sorted(c["out"]):
            for forced in (1, 2):
                try:
                    m.debug_fk20_set_pass(cache, forced)
                    assert both_forms(m, cache, s, polys, int(f)) == (0, bytes.fromhex(c["out"][f]), bytes(3)), (name, f, forced)
                finally:
                    m.debug_fk20_set_pass(cache, 0)
    c = kc.case("special_n8")                                        # the status bytes of a later pass land at their polynomials
    try:
        m.debug_fk20_set_pass(cache, 3)
        assert both_forms(m, cache, setups(bytes.fromhex(c["setup"])), bytes.fromhex(c["polys"]), 0) == (2, bytes.fromhex(c["out"]["0"]), bytes(c["status"]))
    finally:
        m.debug_fk20_set_pass(cache, 0)


def test_a_setup_serves_another_context_of_its_device(m, cache, setups):
    c = kc.case("n8_k3")
    s = setups(bytes.fromhex(c["setup"]))
    other = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        assert both_forms(m, other, s, bytes.fromhex(c["polys"]), 0)[1] == bytes.fromhex(c["out"]["0"])
    finally:
        other.close()
    assert both_forms(m, cache, s, bytes.fromhex(c["polys"]), kc.H)[1] == bytes.fromhex(c["out"]["4"])      # and outlives it


def test_one_context_through_changing_lengths(m, cache, setups):
    for name in ("n16_k3", "n2_k3", "n16_k3", "n1_k3"):
        c = kc.case(name)
        assert both_forms(m, cache, setups(bytes.fromhex(c["setup"])), bytes.fromhex(c["polys"]), 0)[1] == bytes.fromhex(c["out"]["0"]), name


def test_k_zero_and_destroy_of_null(m, cache, setups):
    import torch
    s = setups(bytes.fromhex(kc.case("n4_k3")["setup"]))
    L, h = m.lib(), cache._h
    out = ctypes.create_string_buffer(b"\x5a" * ROW, ROW)
    assert L.mi355_bls_fk20_open_all_many(h, s._h, bytes(32), 0, 0, out, None) == 0 and out.raw == b"\x5a" * ROW
    assert L.mi355_bls_fk20_open_all_many(h, None, None, 0, 99, None, None) == 0                # k == 0 touches nothing, looks at nothing
    d = torch.full((4 * ROW,), 0x5a, dtype=torch.uint8, device="cuda")
    assert L.mi355_bls_fk20_open_all_many_device(h, s._h, d.data_ptr(), 0, 0, d.data_ptr(), None, None) == 0 and host(d) == b"\x5a" * 4 * ROW
    assert m.fk20OpenAllMany(cache, s, b"") == (0, b"", b"")
    L.mi355_bls_fk20_setup_destroy(None)
    m.fk20_setup_destroy(None)


def test_argument_errors_with_a_context(m, cache, setups):
    """MI355_BLS_ERR_ARG (-3) from the C entry points themselves; nothing is written and no handle is made"""
    import torch
    L, h = m.lib(), cache._h
    s = setups(bytes.fromhex(kc.case("n4_k3")["setup"]))
    polys = bytes(4 * 32)
    out = ctypes.create_string_buffer(b"\x5a" * 4 * ROW, 4 * ROW)
    for case in (dict(setup=None), dict(polys=None), dict(out=None), dict(flags=1), dict(flags=8), dict(flags=0x80000002)):
        a = dict(setup=s._h, polys=polys, flags=0, out=out)
        a.update(case)
        assert L.mi355_bls_fk20_open_all_many(h, a["setup"], a["polys"], 1, a["flags"], a["out"], None) == -3, case
    d = torch.full((ROW * 4 + 8,), 0x5a, dtype=torch.uint8, device="cuda")
    dp = torch.zeros((32 * 4 + 8,), dtype=torch.uint8, device="cuda")
    before = host(d)
    P, Q = dp.data_ptr(), d.data_ptr()
    call = lambda pi, po, setup=s._h, flags=0: L.mi355_bls_fk20_open_all_many_device(h, setup, pi, 1, flags, po, None, None)      # noqa: E731
    assert call(P + 1, Q) == -3 and call(P, Q + 2) == -3 and call(None, Q) == -3 and call(P, None) == -3 and call(P, Q, setup=None) == -3
    assert call(P, Q, flags=16) == -3
    hd = ctypes.c_void_p()
    for n in (0, 3, 6, (1 << 31) + 1, 1 << 32):
        assert L.mi355_bls_fk20_setup_create(h, ctypes.byref(hd), bytes(96 * 8), n) == -3 and not hd.value, n
        assert L.mi355_bls_fk20_setup_create_device(h, ctypes.byref(hd), Q, n, None) == -3 and not hd.value, n
    assert L.mi355_bls_fk20_setup_create(h, None, bytes(96), 1) == -3 and L.mi355_bls_fk20_setup_create(h, ctypes.byref(hd), None, 1) == -3
    assert L.mi355_bls_fk20_setup_create_device(h, ctypes.byref(hd), None, 1, None) == -3
    assert L.mi355_bls_fk20_setup_create_device(h, ctypes.byref(hd), Q + 1, 1, None) == -3 and not hd.value
    assert host(d) == before and out.raw == b"\x5a" * 4 * ROW
    assert call(P + 4, Q + 4) == 0 and host(d)[4:4 + 4 * ROW] == bytes(4 * ROW)                   # aligned to 4 bytes, not to 16; the zero polynomial


def test_a_busy_context_is_refused(m, setups):
    """a context with a submitted batch that has not been waited for: -3 before anything is launched, the output untouched"""
    import json
    import os
    import torch
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch.json")))
    case = [c for c in g["cases"] if c["name"] == "n3"][0]
    s = setups(bytes.fromhex(kc.case("n4_k3")["setup"]))
    c = m.BatchedBLSVerifierCache.init(max_sets=64, numThreads=4)
    try:
        L = m.lib()
        recs = dev(bytes.fromhex(case["sets"]))
        d = torch.full((ROW * 4,), 0x5a, dtype=torch.uint8, device="cuda")
        dp = torch.zeros((32 * 4,), dtype=torch.uint8, device="cuda")
        out = ctypes.create_string_buffer(b"\x5a" * 4 * ROW, 4 * ROW)
        hd = ctypes.c_void_p()
        c.submit_device(recs.data_ptr(), case["n"], bytes.fromhex(case["rnd"]))
        assert L.mi355_bls_fk20_open_all_many_device(c._h, s._h, dp.data_ptr(), 1, 0, d.data_ptr(), None, None) == -3
        assert L.mi355_bls_fk20_open_all_many(c._h, s._h, bytes(4 * 32), 1, 0, out, None) == -3
        assert b"not been waited for" in L.mi355_bls_last_error()
        assert L.mi355_bls_fk20_setup_create(c._h, ctypes.byref(hd), bytes(96), 1) == -3 and not hd.value
        assert c.wait() is True
        assert host(d) == out.raw == b"\x5a" * 4 * ROW
        assert L.mi355_bls_fk20_open_all_many(c._h, s._h, bytes(4 * 32), 1, 0, out, None) == 0 and out.raw == bytes(4 * ROW)
    finally:
        c.close()


# ---- beyond the fixture: expected images from scalars
def test_fr_transform_in_more_than_one_pass_gives_the_same_bytes(m, cache, setups):
    """a tile of four elements: the 2n scalars of a polynomial take two passes at n = 8 and three at n = 16, in place in the scalar array"""
    seen = set()
    try:
        m.debug_frntt_set_tile(cache, 2)
        for name, n, k, flags, setup, polys, want, status in kc.cases():
            if name in ("n8_k3", "n16_k3", "special_n8"):
                rc, got, st = both_forms(m, cache, setups(setup), polys, flags)
                assert st == status and rc == sum(1 for b in status if b), (name, flags)
                for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))):
                    assert a == b, (name, flags, i)
                seen.add((name, flags))
    finally:
        m.debug_frntt_set_tile(cache, 0)
    assert len(seen) == 3 + 3 + 2


@pytest.fixture(scope="module")
def srs_setup(m, cache):
    """-> (handle over [tau^i]G, i < n; the SRS made on the device and handed over there), one per n; released at the end"""
    made = {}

    def get(n):
        if n not in made:
            d_srs = gi.dev(gi.multiples_of_g(m, cache, list(lc.srs_scalars(n))))
            made[n] = m.fk20_setup_create_device(cache, d_srs.data_ptr(), n)
        return made[n]
    yield get
    for s in made.values():
        m.fk20_setup_destroy(s)


@pytest.mark.parametrize("flags", [0, kc.BITREV, kc.H])
def test_fr_transform_in_two_passes_at_the_default_tile(m, cache, srs_setup, flags):
    """n = 1024: 2048 scalars per polynomial, twice the default tile; k = 3 and its first polynomial alone"""
    n = 1024
    assert 2 * n > lc.fr_tile()
    rows = [list(v) for v in fc.random_vectors(1024, 3, n)]
    rows[1][n - 1] += kc.R                                                    # status byte 2 at polynomial 1; c_(n-1) is the one the circulant wraps
    want = gi.multiples_of_g(m, cache, [a for row in ks.expected_srs(kc.TAU, rows, 1, 0, flags) for a in row])
    assert want.count(0) < 3 * n * 8
    assert both_forms(m, cache, srs_setup(n), fc.pack(rows), flags) == (1, want, bytes([0, 2, 0]))
    assert both_forms(m, cache, srs_setup(n), fc.pack(rows[:1]), flags) == (0, want[:n * ROW], bytes(1))


def with_a_root_at(n, j, tau, seed):
    """(X - omega_n^j)(X - tau) d(X) + const, d random of degree n - 3: the quotient by X - omega_n^j has the root tau, pi_j is infinity"""
    d = list(fc.random_vectors(seed, 1, n - 1)[0])
    p, const = d[:n - 2], d[n - 2]
    for root in (pow(fc.omega(n), j, kc.R), tau):
        p = [((p[i - 1] if i else 0) - root * (p[i] if i < len(p) else 0)) % kc.R for i in range(len(p) + 1)]
    p[0] = (p[0] + const) % kc.R
    return p


@pytest.mark.parametrize("flags", [kc.H, 0])
def test_finish_with_a_shared_inversion(m, cache, srs_setup, flags):
    """k = 1025 polynomials of 64 coefficients, three distinct ones cycled: 65 600 outputs, more than TOAFF_DEVICE_LANES, so a lane of
    k_fk20_finish inverts once for two neighbours.  With H every vector ends in h_62 beside the infinity h_63; without, one polynomial
    in three has the infinity pi_6 beside pi_7, stored at their bit-reversed places"""
    n, k, j = 64, 1025, 6
    assert k * n > lc.toaff_device_lanes() and k * n <= 2 * lc.toaff_device_lanes()
    rows = [list(v) for v in fc.random_vectors(65, 2, n)] + [with_a_root_at(n, j, kc.TAU, 66)]
    scalars = ks.expected_srs(kc.TAU, rows, 1, 0, flags)
    if flags & kc.H:
        assert all(row[n - 1] == 0 and all(row[:n - 1]) for row in scalars)
    else:
        assert all(all(row) for row in scalars[:2]) and [i for i, a in enumerate(scalars[2]) if a == 0] == [j] and scalars[2][j + 1]
    want = kc.rows(gi.multiples_of_g(m, cache, [a for row in scalars for a in row]))
    want = lc.cycled([b"".join(want[g * n:(g + 1) * n]) for g in range(3)], k)
    rc, got, st = both_forms(m, cache, srs_setup(n), lc.cycled([fc.pack([row]) for row in rows], k), flags)
    assert (rc, st) == (0, bytes(k))
    assert got == want, [i for i, (a, b) in enumerate(zip(kc.rows(got), kc.rows(want))) if a != b][:8]
