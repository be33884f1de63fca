"""Cell proofs end to end, device-resident, at n = 64, cells of l = 8 points, ext_log2 = 1 (16 cells on the domain of 128) and k = 2.  The
cells are mi355_bls_fr_ntt_many's (BITREV) evaluation of the zero-extended coefficients: cell i is slots [8 i, 8 i + 8), the coset
x^8 = omega_16^rev4(i).  The proofs of mi355_bls_fk20_open_cells_many_device (BITREV, the same cell order) must
  1 equal, byte for byte, the definition route: the quotients p(X) div (X^8 - a_i) from Python integers, the k 16 of them through
    p1s_mult_pippenger_many_device over the shared SRS, p1s_to_affine_device;
  2 pass the pairing check e(C - [I_i(tau)]G, G2) e(-pi_i, [tau^8 - a_i]G2) == 1 for every polynomial and every cell, I_i the interpolant of
    the cell's eight values as the device transform gave them, with [tau^8 - a_i]G2 from p2sLincombMany_device and C - [I_i(tau)]G, -pi_i
    from p1sLincombMany_device;
  3 fail it for the polynomial that had one byte of one coefficient changed before the proofs were made, and for that one alone."""
import pytest

import fk20_cells_cases as kc
import frntt_cases as fc
import g2many_helpers as h
import p1ntt_cases as pc

pytestmark = pytest.mark.gpu
N, L, EXT, K = 64, 8, 1, 2
Q = N // L
CELLS = Q << EXT                                                   # 16
DOMAIN = N << EXT                                                  # 128
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


def divide(c, a):
    """p(X) = quo(X) (X^L - a) + rem(X) -> (quo: n coefficients, the top L of them 0; rem: L coefficients)"""
    rem, quo = list(c), [0] * len(c)
    for d in range(len(c) - 1, L - 1, -1):
        quo[d - L] = rem[d]
        rem[d - L] = (rem[d - L] + a * rem[d]) % R
        rem[d] = 0
    return quo, rem[:L]


def test_proofs_equal_the_definition_route_and_verify(m):
    import bls12381_py as o
    import torch
    assert TAU and pow(TAU, DOMAIN, R) != 1                        # tau outside the domain
    coefs = fc.random_vectors(2065, K, N)
    w = fc.omega(DOMAIN)
    mc, md = CELLS.bit_length() - 1, DOMAIN.bit_length() - 1
    a_of = [pow(fc.omega(CELLS), fc.rev(i, mc), R) for i in range(CELLS)]          # cell i: x^L = a_of[i]
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    setup = None
    try:
        empty = lambda size: torch.empty((size,), dtype=torch.uint8, device="cuda")      # noqa: E731
        # the SRS [tau^j]G, made on the device
        d_srs, d_g1 = empty(N * 96), dev(pc.G_IMAGE)
        d_zero, d_pow = torch.zeros(N, dtype=torch.int32, device="cuda"), dev(b"".join(fc.le(pow(TAU, j, R)) for j in range(N)))
        ok, st = m.p1sLincombMany_device(cache, d_g1.data_ptr(), 1, d_zero.data_ptr(), list(range(N + 1)), d_pow.data_ptr(), d_srs.data_ptr())
        assert ok and st == bytes(N)
        setup = m.fk20_setup_create_cells_device(cache, d_srs.data_ptr(), N, L)

        # the cells: the bit-reversed evaluation of the zero-extended coefficients
        d_polys = dev(fc.pack(coefs))
        d_cells = dev(fc.pack([list(p) + [0] * (DOMAIN - N) for p in coefs]))
        assert m.frNttMany_device(cache, d_cells.data_ptr(), DOMAIN, K, m.FR_NTT_BITREV) == (0, bytes(K))
        cells = fc.images(host(d_cells))
        xs = [pow(w, fc.rev(s, md), R) for s in range(DOMAIN)]                      # slot s of a vector is the value at xs[s]
        assert cells == [sum(c * pow(x, j, R) for j, c in enumerate(p)) % R for p in coefs for x in xs]
        assert all(pow(xs[L * i + t], L, R) == a_of[i] for i in range(CELLS) for t in range(L))

        # the proofs
        d_proofs = empty(K * CELLS * 96)
        assert m.fk20OpenCellsMany_device(cache, setup, d_polys.data_ptr(), K, d_proofs.data_ptr(), EXT, m.FK20_BITREV) == (0, bytes(K))
        proofs = host(d_proofs)
        assert proofs.count(0) < K * CELLS * 8

        # 1: the definition route - a quotient per (polynomial, cell), an MSM each over the shared SRS
        parts = [divide(p, a) for p in coefs for a in a_of]
        d_quot = dev(fc.pack([quo for quo, _ in parts]))
        d_jac, d_old = empty(K * CELLS * 144), empty(K * CELLS * 96)
        m.p1s_mult_pippenger_many_device(cache, d_srs.data_ptr(), N, d_quot.data_ptr(), None, K * CELLS, 255, d_out=d_jac.data_ptr())
        m.p1s_to_affine_device(cache, d_jac.data_ptr(), K * CELLS, d_old.data_ptr())
        for i, (x, y) in enumerate(zip(kc.rows(proofs), kc.rows(host(d_old)))):
            assert x == y, i

        # I_e(tau) from the cell's values: L_t(tau) = (tau^L - a) / (L x_t^(L-1) (tau - x_t)) over the coset x^L = a
        def interpolant_at_tau(g, i):
            a, total = a_of[i], 0
            for t in range(L):
                x = xs[L * i + t]
                total += cells[g * DOMAIN + L * i + t] * pow(L * pow(x, L - 1, R) * (TAU - x), -1, R)
            return total * (pow(TAU, L, R) - a) % R

        its = [interpolant_at_tau(g, i) for g in range(K) for i in range(CELLS)]
        assert its == [sum(b * pow(TAU, j, R) for j, b in enumerate(rem)) % R for _, rem in parts]      # the remainder of the division

        # the commitments C_g
        d_cj, d_c = empty(K * 144), empty(K * 96)
        m.p1s_mult_pippenger_many_device(cache, d_srs.data_ptr(), N, d_polys.data_ptr(), None, K, 255, d_out=d_cj.data_ptr())
        m.p1s_to_affine_device(cache, d_cj.data_ptr(), K, d_c.data_ptr())

        # 2: G2 side - member 2 e is [1]G2, member 2 e + 1 is [1][tau^L]G2 + [-a_i]G2, the same for every polynomial
        d_g2tab = dev(o.g2_to_blst_affine(o.g2_mul(o.G2_GEN, pow(TAU, L, R))) + o.g2_to_blst_affine(o.G2_GEN))
        d_idx_g2 = torch.tensor([i for _ in range(K * CELLS) for i in (1, 0, 1)], dtype=torch.int32, device="cuda")
        d_sc_g2 = dev(b"".join(fc.le(1) + fc.le(1) + fc.le(-a % R) for _ in range(K) for a in a_of))
        d_q = empty(2 * K * CELLS * 192)
        ok, st = m.p2sLincombMany_device(cache, d_g2tab.data_ptr(), 2, d_idx_g2.data_ptr(), h.offsets_of([1, 2] * (K * CELLS)), d_sc_g2.data_ptr(), d_q.data_ptr())
        assert ok and st == bytes(2 * K * CELLS)

        def verdicts(d_pi):
            """the pairing check of every (polynomial, cell) with the proofs at d_pi: member 2 e is C_g - [I_e(tau)]G, member 2 e + 1 is -pi_e"""
            d_tab = torch.cat([d_c, d_g1, d_pi])                   # rows 0 .. K-1: C_g | row K: G | rows K + 1 ..: the proofs
            d_idx = torch.tensor([i for e in range(K * CELLS) for i in (e // CELLS, K, K + 1 + e)], dtype=torch.int32, device="cuda")
            d_sc = dev(b"".join(fc.le(1) + fc.le(-y % R) + fc.le(R - 1) for y in its))
            d_p = empty(2 * K * CELLS * 96)
            ok, st = m.p1sLincombMany_device(cache, d_tab.data_ptr(), K + 1 + K * CELLS, d_idx.data_ptr(), h.offsets_of([2, 1] * (K * CELLS)), d_sc.data_ptr(),
                                             d_p.data_ptr())
            assert ok and st == bytes(2 * K * CELLS)
            each, status = m.pairingCheckEach_device(cache, d_p.data_ptr(), d_q.data_ptr(), h.offsets_of([2] * (K * CELLS)), flags=m.PAIR_VALIDATE)
            assert status == [0] * (2 * K * CELLS)
            return each

        assert verdicts(d_proofs) == [True] * (K * CELLS)

        # 3: one byte of coefficient 61 of polynomial 1 changed before the proofs are made (a coefficient below l enters no proof at all)
        d_bad_polys, d_bad = d_polys.clone(), empty(K * CELLS * 96)
        d_bad_polys[(N + 61) * 32 + 7] ^= 0x10
        assert m.fk20OpenCellsMany_device(cache, setup, d_bad_polys.data_ptr(), K, d_bad.data_ptr(), EXT, m.FK20_BITREV) == (0, bytes(K))
        assert host(d_bad)[:CELLS * 96] == proofs[:CELLS * 96]
        assert verdicts(d_bad) == [True] * CELLS + [False] * CELLS
    finally:
        m.fk20_setup_destroy(setup)
        cache.close()
