"""Short linear combinations per group on the device (mi355_bls_p1s_lincomb_many / mi355_bls_p2s_lincomb_many).  Images and status bytes are
held bit-exact to tests/golden/lincomb.json on both curves, in both context modes, on both G2 routes, in the host and the device form,
contiguous and indexed, with good and bad indices; a call forced into chunks of 16 terms gives the unchunked call's bytes; the same inputs
through the many-MSM calls and to_affine give byte-equal images; the recovery fixture's groups, run with Lagrange coefficients computed in
Python, give the fixture's recovered signatures; and the device output feeds the pairing check of an opening unchanged.  The CPU half is
tests/test_lincomb_emu.py."""
import random

import pytest

import lincomb_cases as lc
import recover_cases as rc

pytestmark = pytest.mark.gpu

ROUTES = [("g1", 0), ("g2", 0), ("g2", 1)]


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
def fx():
    return lc.fixture()


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def dev_idx(idx):
    import torch
    return torch.tensor(idx, dtype=torch.int64).to(torch.int32).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def call(m, curve):
    return (m.p2sLincombMany, m.p2sLincombMany_device) if curve == "g2" else (m.p1sLincombMany, m.p1sLincombMany_device)


@pytest.mark.parametrize("curve,psi", ROUTES)
def test_fixture_bit_exact_in_both_modes_and_forms(m, cache, fx, curve, psi):
    import torch
    row = lc.ROW[curve]
    many, many_device = call(m, curve)
    tab = lc.table_of(fx, curve)
    seen = set()
    for coop in (True, False):
        cache.set_cooperative(coop)
        for nbits in lc.nbits_values(fx, curve):
            groups = lc.groups_of(fx, curve, nbits, psi)
            pts, sc, offsets, want, status = lc.contiguous_inputs(fx, curve, groups)
            lists = [b"".join(tab[t] for t, _ in g["terms"]) for g in groups]
            scl = [[bytes.fromhex(s) for _, s in g["terms"]] for g in groups]
            got = many(cache, lists, scl, nbits, psi)
            bad_groups = [g["kind"] for i, g in enumerate(groups) if got[1][row * i:row * i + row] != want[row * i:row * i + row] or got[2][i] != status[i]]
            assert bad_groups == [] and got[0] == (not any(status)), (coop, nbits)
            seen |= set(status)
            if nbits != 255:
                continue
            assert many(cache, (pts, None, offsets), sc, nbits, psi) == (False, want, status), coop
            k = len(groups)
            d_p, d_s = dev(pts), dev(sc)
            out = torch.full((row * k,), 0x5a, dtype=torch.uint8, device="cuda")
            assert many_device(cache, d_p.data_ptr(), len(pts) // row, None, offsets, d_s.data_ptr(), out.data_ptr(), nbits, psi) == (False, status)
            assert host(out) == want, coop
            for bad in (False, True):
                table, idx, isc, ioffs, iwant, ist = lc.indexed_inputs(fx, curve, groups, bad)
                assert many(cache, (table, idx, ioffs), isc, nbits, psi) == (False, iwant, ist), (coop, bad)
                assert (3 in ist) == bad
                d_t, d_i, d_is = dev(table), dev_idx(idx), dev(isc)
                out = torch.full((row * k,), 0x5a, dtype=torch.uint8, device="cuda")
                assert many_device(cache, d_t.data_ptr(), len(table) // row, d_i.data_ptr(), ioffs, d_is.data_ptr(), out.data_ptr(), nbits, psi) == (False, ist)
                assert host(out) == iwant, (coop, bad)
            good = [g for g in groups if g["status"] == 0]
            pts, sc, offsets, want, status = lc.contiguous_inputs(fx, curve, good)
            assert many(cache, (pts, None, offsets), sc, nbits, psi) == (True, want, bytes(len(good))), coop
    cache.set_cooperative(True)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("curve,psi", ROUTES)
def test_forced_chunks_give_the_unchunked_bytes(m, cache, fx, curve, psi):
    many, _ = call(m, curve)
    groups = lc.groups_of(fx, curve, 255, psi)
    table, idx, sc, offsets, want, status = lc.indexed_inputs(fx, curve, groups, True)
    whole = many(cache, (table, idx, offsets), sc, 255, psi)
    try:
        m.debug_lincomb_set_chunk(cache, 16)
        assert many(cache, (table, idx, offsets), sc, 255, psi) == whole == (False, want, status)
    finally:
        m.debug_lincomb_set_chunk(cache, 0)


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_equals_the_many_msm_call_and_to_affine(m, cache, fx, curve):
    many, _ = call(m, curve)
    msm, to_affine = (m.p2s_mult_pippenger_many, m.p2s_to_affine) if curve == "g2" else (m.p1s_mult_pippenger_many, m.p1s_to_affine)
    for nbits in (255, 64):
        groups = lc.groups_of(fx, curve, 255)                 # the 255-bit groups again under nbits = 64: nothing expected from the fixture
        pts, sc, offsets, want, status = lc.contiguous_inputs(fx, curve, groups)
        images = to_affine(cache, b"".join(msm(cache, pts, sc, offsets, nbits)))
        for flags in ((0, 1) if curve == "g2" else (0,)):
            ok, out, st = many(cache, (pts, None, offsets), sc, nbits, flags)
            assert out == images and (nbits != 255 or (out, st) == (want, status)), (nbits, flags)


def test_argument_errors_with_a_context(m, cache, fx):
    """MI355_BLS_ERR_ARG (-3) from the C entry points themselves (the Python mirror refuses most of these before the call); nothing is written"""
    import ctypes
    import torch
    L, h = m.lib(), cache._h
    SZ = ctypes.c_size_t
    for name, curve in (("mi355_bls_p1s_lincomb_many", "g1"), ("mi355_bls_p2s_lincomb_many", "g2")):
        row = lc.ROW[curve]
        pt, sc = lc.table_of(fx, curve)[1] * 2, bytes([1]) + bytes(31) + bytes([2]) + bytes(63)          # (a third scalar: the offsets[k] = 3 case stages it)
        out, st = ctypes.create_string_buffer(b"\x5a" * row, row), ctypes.create_string_buffer(b"\x5a", 1)
        host_fn, dev_fn = getattr(L, name), getattr(L, name + "_device")
        offs = (SZ * 2)(0, 2)
        subgroup = m.LINCOMB_SUBGROUP if curve == "g1" else 0
        bad = [dict(nbits=0), dict(nbits=257), dict(flags=2), dict(flags=0x80000000), dict(offs=(SZ * 2)(2, 0)), dict(offs=(SZ * 2)(0, 3)), dict(pt=None), dict(sc=None),
               dict(out=None), dict(st=None), dict(offs=None)] + ([dict(flags=subgroup)] if subgroup else [])
        for case in bad:
            a = dict(pt=pt, offs=offs, sc=sc, nbits=255, flags=0, out=out, st=st)
            a.update(case)
            assert host_fn(h, a["pt"], 2, None, a["offs"], 1, a["sc"], a["nbits"], a["flags"], a["out"], a["st"]) == -3, (name, case)
        assert out.raw == b"\x5a" * row and st.raw == b"\x5a"
        assert host_fn(h, pt, 2, None, offs, 0, sc, 255, 0, out, st) == 0 and out.raw == b"\x5a" * row                   # k == 0: nothing written
        d_p, d_s, d_o = dev(pt), dev(sc + bytes(4)), torch.zeros(row + 4, dtype=torch.uint8, device="cuda")
        ok = lambda p, s, o, nbits=255, flags=0: dev_fn(h, p, 2, None, offs, 1, s, nbits, flags, o, st, None)            # noqa: E731
        assert ok(d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr()) == 1
        assert ok(d_p.data_ptr(), d_s.data_ptr() + 1, d_o.data_ptr()) == -3 and ok(d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr() + 2) == -3      # alignment
        assert ok(d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), nbits=0) == -3 and ok(d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), flags=4) == -3
        assert ok(d_p.data_ptr(), d_s.data_ptr(), None) == -3
        if curve == "g2":
            assert ok(d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), flags=m.LINCOMB_SUBGROUP) == 1
        assert L.mi355_bls_debug_lincomb_set_chunk(h, 0) == 0


def test_recovery_fixture_with_python_coefficients(m, cache):
    fx = rc.fixture()
    tab = rc.table_of(fx)
    groups = [g for g in fx["groups"] if g["status"] == 0]
    assert len(groups) >= 20
    lists, scalars = [], []
    for g in groups:
        ids = [int.from_bytes(bytes.fromhex(x), "little") for x in g["ids"]]
        lists.append(b"".join(tab[i] for i in g["members"]))
        scalars.append([1 if len(ids) == 1 else rc.coefficient(ids, i) for i in range(len(ids))])
    want = b"".join(bytes.fromhex(g["out192"]) for g in groups)
    for flags in (0, m.LINCOMB_SUBGROUP):
        assert m.p2sLincombMany(cache, lists, scalars, 255, flags) == (True, want, bytes(len(groups))), flags


def test_device_output_feeds_the_pairing_check_of_an_opening(m, cache):
    """K openings e(C - [y]G1, G2) e(-pi, [tau - z]G2) == 1: both sides made by the new calls in device memory.  G2 side: a one-row table (the
    generator), idx all 0, group 2 g = [1]G2, group 2 g + 1 = [tau]G2 + [-z_g]G2.  G1 side: the table is the setup [tau^i]G1, group 2 g =
    C_g - [y_g]G1 (five terms), group 2 g + 1 = -pi_g (three)."""
    import torch
    import bls12381_py as o
    K = 4
    rng = random.Random(2027)
    le = lambda v: (v % o.R).to_bytes(32, "little")          # noqa: E731
    tau = rng.randrange(2, o.R)
    srs = [o.g1_mul(o.G1_GEN, pow(tau, i, o.R)) for i in range(4)]
    polys = [[rng.randrange(o.R) for _ in range(4)] for _ in range(K)]
    zs = [rng.randrange(o.R) for _ in range(K)]
    qs, ys = [], []
    for p, z in zip(polys, zs):                                # p(X) = q(X) (X - z) + p(z)
        q, carry = [0, 0, 0], 0
        for i in (3, 2, 1):
            carry = (p[i] + carry * z) % o.R
            q[i - 1] = carry
        qs.append(q)
        ys.append((p[0] + carry * z) % o.R)
    d_gen = dev(o.g2_to_blst_affine(o.G2_GEN))
    d_srs = dev(b"".join(o.g1_to_blst_affine(p) for p in srs))
    d_q = torch.full((2 * K * 192,), 0xaa, dtype=torch.uint8, device="cuda")
    d_p = torch.full((2 * K * 96,), 0xaa, dtype=torch.uint8, device="cuda")
    offs_q, offs_p = [0], [0]
    for _ in range(K):
        offs_q += [offs_q[-1] + 1, offs_q[-1] + 3]
        offs_p += [offs_p[-1] + 5, offs_p[-1] + 8]
    d_iq, d_ip = dev_idx([0] * (3 * K)), dev_idx([0, 1, 2, 3, 0, 0, 1, 2] * K)
    d_sq = dev(b"".join(le(1) + le(tau) + le(-z) for z in zs))
    want_q = b"".join(o.g2_to_blst_affine(o.G2_GEN) + o.g2_to_blst_affine(o.g2_mul(o.G2_GEN, (tau - z) % o.R)) for z in zs)
    pair_offs = list(range(0, 2 * K + 1, 2))

    def verdicts(claimed, flags):
        d_q.fill_(0xaa)
        assert m.p2sLincombMany_device(cache, d_gen.data_ptr(), 1, d_iq.data_ptr(), offs_q, d_sq.data_ptr(), d_q.data_ptr(), 255, flags) == (True, bytes(2 * K))
        assert host(d_q) == want_q
        d_sp = dev(b"".join(b"".join(le(c) for c in p) + le(-y) + b"".join(le(-c) for c in q) for p, q, y in zip(polys, qs, claimed)))
        assert m.p1sLincombMany_device(cache, d_srs.data_ptr(), 4, d_ip.data_ptr(), offs_p, d_sp.data_ptr(), d_p.data_ptr()) == (True, bytes(2 * K))
        each, status = m.pairingCheckEach_device(cache, d_p.data_ptr(), d_q.data_ptr(), pair_offs, flags=m.PAIR_VALIDATE)
        assert status == [0] * (2 * K)
        return each

    assert verdicts(ys, 0) == [True] * K
    wrong = list(ys)
    wrong[2] = (wrong[2] + 1) % o.R
    assert verdicts(wrong, m.LINCOMB_SUBGROUP) == [True, True, False, True]
