"""All openings end to end, device-resident, at n = 64 and k = 2.  The proofs of mi355_bls_fk20_open_all_many_device must
  1 equal, byte for byte, the existing n-fold route: frOpenMany_device over each polynomial replicated n times and the whole domain, the
    k n quotients through p1s_mult_pippenger_many_device over the SRS, p1s_to_affine_device;
  2 pass the pairing check e(C - [y_l]G, G2) e(-pi_l, [tau - omega^l]G2) == 1 for every polynomial and every l, with [tau - omega^l]G2 from
    p2sLincombMany_device and C - [y_l]G, -pi_l from p1sLincombMany_device;
  3 fail it for the polynomial that had one byte of one coefficient changed before the proofs were made, and for that one alone.
Only the k n values y_l come back to the host, to form -y_l."""
import pytest

import fk20_cases as kc
import frntt_cases as fc
import g2many_helpers as h
import p1ntt_cases as pc

pytestmark = pytest.mark.gpu
N, K = 64, 2
R = kc.R
TAU = kc.TAU


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def test_proofs_equal_the_n_fold_route_and_verify(m):
    import bls12381_py as o
    import torch
    assert TAU and pow(TAU, N, R) != 1                              # tau outside the domain
    coefs = fc.random_vectors(2064, K, N)
    dom = fc.domain(N)
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    setup = None
    try:
        empty = lambda size: torch.empty((size,), dtype=torch.uint8, device="cuda")      # noqa: E731
        # the SRS [tau^j]G, made on the device
        d_srs, d_g1 = empty(N * 96), dev(pc.G_IMAGE)
        d_zero, d_pow = torch.zeros(N, dtype=torch.int32, device="cuda"), dev(b"".join(fc.le(pow(TAU, j, R)) for j in range(N)))
        ok, st = m.p1sLincombMany_device(cache, d_g1.data_ptr(), 1, d_zero.data_ptr(), list(range(N + 1)), d_pow.data_ptr(), d_srs.data_ptr())
        assert ok and st == bytes(N)
        setup = m.fk20_setup_create_device(cache, d_srs.data_ptr(), N)
        d_polys, d_proofs = dev(fc.pack(coefs)), empty(K * N * 96)
        assert m.fk20OpenAllMany_device(cache, setup, d_polys.data_ptr(), K, d_proofs.data_ptr()) == (0, bytes(K))

        # 1: the existing route - every polynomial n times, opened at the whole domain
        d_rep = d_polys.view(K, 1, N * 32).expand(K, N, N * 32).contiguous()
        d_zs = dev(fc.pack([dom] * K))
        d_ys, d_quot = empty(K * N * 32), empty(K * N * N * 32)
        reduced, _ = m.frOpenMany_device(cache, d_rep.data_ptr(), N, d_zs.data_ptr(), K * N, 0, None, d_ys.data_ptr(), d_quot.data_ptr())
        assert reduced == 0
        d_jac, d_old = empty(K * N * 144), empty(K * N * 96)
        m.p1s_mult_pippenger_many_device(cache, d_srs.data_ptr(), N, d_quot.data_ptr(), None, K * N, 255, d_out=d_jac.data_ptr())
        m.p1s_to_affine_device(cache, d_jac.data_ptr(), K * N, d_old.data_ptr())
        proofs = host(d_proofs)
        assert proofs.count(0) < K * N * 8
        for i, (a, b) in enumerate(zip(kc.rows(proofs), kc.rows(host(d_old)))):
            assert a == b, i
        ys = fc.images(host(d_ys))
        assert ys == [sum(c * pow(x, j, R) for j, c in enumerate(p)) % R for p in coefs for x in dom]

        # the commitments C_g
        d_cj, d_c = empty(K * 144), empty(K * 96)
        m.p1s_mult_pippenger_many_device(cache, d_srs.data_ptr(), N, d_polys.data_ptr(), None, K, 255, d_out=d_cj.data_ptr())
        m.p1s_to_affine_device(cache, d_cj.data_ptr(), K, d_c.data_ptr())

        # 2: G2 side - member 2 l is [1]G2, member 2 l + 1 is [1][tau]G2 + [-omega^l]G2, the same for every polynomial
        d_g2tab = dev(o.g2_to_blst_affine(o.g2_mul(o.G2_GEN, TAU)) + o.g2_to_blst_affine(o.G2_GEN))
        d_idx_g2 = torch.tensor([i for _ in range(K * N) for i in (1, 0, 1)], dtype=torch.int32, device="cuda")
        d_sc_g2 = dev(b"".join(fc.le(1) + fc.le(1) + fc.le(-x % R) for _ in range(K) for x in dom))
        d_q = empty(2 * K * N * 192)
        ok, st = m.p2sLincombMany_device(cache, d_g2tab.data_ptr(), 2, d_idx_g2.data_ptr(), h.offsets_of([1, 2] * (K * N)), d_sc_g2.data_ptr(), d_q.data_ptr())
        assert ok and st == bytes(2 * K * N)

        def verdicts(d_pi):
            """the pairing check of every (polynomial, l) with the proofs at d_pi: member 2 e is C_g - [y_e]G, member 2 e + 1 is -pi_e"""
            d_tab = torch.cat([d_c, d_g1, d_pi])                   # rows 0 .. K-1: C_g | row K: G | rows K + 1 ..: the proofs
            d_idx = torch.tensor([i for e in range(K * N) for i in (e // N, K, K + 1 + e)], dtype=torch.int32, device="cuda")
            d_sc = dev(b"".join(fc.le(1) + fc.le(-y % R) + fc.le(R - 1) for y in ys))
            d_p = empty(2 * K * N * 96)
            ok, st = m.p1sLincombMany_device(cache, d_tab.data_ptr(), K + 1 + K * N, d_idx.data_ptr(), h.offsets_of([2, 1] * (K * N)), d_sc.data_ptr(), d_p.data_ptr())
            assert ok and st == bytes(2 * K * N)
            each, status = m.pairingCheckEach_device(cache, d_p.data_ptr(), d_q.data_ptr(), h.offsets_of([2] * (K * N)), flags=m.PAIR_VALIDATE)
            assert status == [0] * (2 * K * N)
            return each

        assert verdicts(d_proofs) == [True] * (K * N)

        # 3: one byte of coefficient 5 of polynomial 1 changed before the proofs are made
        d_bad_polys, d_bad = d_polys.clone(), empty(K * N * 96)
        d_bad_polys[(N + 5) * 32 + 7] ^= 0x10
        assert m.fk20OpenAllMany_device(cache, setup, d_bad_polys.data_ptr(), K, d_bad.data_ptr()) == (0, bytes(K))
        assert host(d_bad)[:N * 96] == proofs[:N * 96]
        assert verdicts(d_bad) == [True] * N + [False] * N
    finally:
        m.fk20_setup_destroy(setup)
        cache.close()
