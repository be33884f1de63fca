"""End to end on the device with the quotients made there: the flow of tests/test_gpu_opening_check.py - K openings checked by
e(C - [y]G1, G2) e(-pi, [tau - z]G2) == 1 - where y_g and the quotient scalars come from mi355_bls_fr_open_many_device and go into the MSM
call as device pointers.  One variant opens coefficient-form polynomials over the setup [tau^i]G1 with the many-MSM call, the other
evaluation-form polynomials over a toy Lagrange table of 8 points, made with the oracle from a known tau, with the fixed-base table call.  Only
the K values y_g come back to the host (to form -y_g, and to tamper with one)."""
import random

import pytest

import bls12381_py as o
import fropen_cases as fc
import g2many_helpers as h

pytestmark = pytest.mark.gpu
K = 5


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def le(v):
    return (v % o.R).to_bytes(32, "little")


def openings_verify(m, lagrange):
    import torch
    assert o.R == fc.R
    rng = random.Random(2028 + lagrange)
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    tau = rng.randrange(2, o.R)
    tau_g2 = o.g2_mul(o.G2_GEN, tau)
    if lagrange:                                                    # the basis [l_i(tau)]G1 over the 8th roots of unity, bit-reversed
        n = 8
        xs = fc.domain(n, True)
        c = (pow(tau, n, o.R) - 1) * pow(n, -1, o.R) % o.R
        basis = [o.g1_mul(o.G1_GEN, c * x % o.R * pow(tau - x, -1, o.R) % o.R) for x in xs]
        zs = [rng.randrange(o.R), xs[3], rng.randrange(o.R), rng.randrange(o.R), xs[0]]      # two of them inside the domain
    else:
        n, xs = 4, None
        basis = [o.g1_mul(o.G1_GEN, pow(tau, i, o.R)) for i in range(n)]
        zs = [rng.randrange(o.R) for _ in range(K)]
    polys = [[rng.randrange(o.R) for _ in range(n)] for _ in range(K)]
    want_ys, want_quot, want_st, _ = fc.expected(polys, zs, xs)
    d_g1 = on_device(o.g1_to_blst_affine(o.G1_GEN))
    d_g2s = on_device(o.g2_to_blst_affine(tau_g2) + o.g2_to_blst_affine(o.G2_GEN))

    # y_g and q_g on the device; the quotient never leaves it
    d_polys, d_zs = on_device(fc.pack(polys)), on_device(fc.pack([zs]))
    d_dom = on_device(fc.pack([xs])) if lagrange else None
    d_ys = torch.empty((K, 32), dtype=torch.uint8, device="cuda")
    d_quot = torch.empty((K, n * 32), dtype=torch.uint8, device="cuda")
    reduced, st = m.frOpenMany_device(cache, d_polys.data_ptr(), n, d_zs.data_ptr(), K, m.FR_OPEN_EVAL if lagrange else 0,
                                      d_dom.data_ptr() if lagrange else None, d_ys.data_ptr(), d_quot.data_ptr())
    assert (reduced, st) == (0, want_st) and (sum(st) == 2) == bool(lagrange)
    torch.cuda.synchronize()
    ys = fc.images(bytes(d_ys.cpu().numpy()))                       # K scalars back: -y_g below is formed on the host
    assert ys == fc.images(want_ys)

    # C_g and pi_g: 2 K MSMs over the n shared points, member 2 g the polynomial, member 2 g + 1 its quotient as the call above left it
    d_sc1 = torch.cat([d_polys.view(K, 1, n * 32), d_quot.view(K, 1, n * 32)], dim=1).contiguous()
    d_jac1 = torch.empty((2 * K * 144,), dtype=torch.uint8, device="cuda")
    d_cpi = torch.empty((2 * K, 96), dtype=torch.uint8, device="cuda")
    points = b"".join(o.g1_to_blst_affine(p) for p in basis)
    table = None
    if lagrange:
        table = m.p1s_table_create(cache, points, 8, 255)
        m.p1s_mult_table_many_device(cache, table, d_sc1.data_ptr(), 2 * K, 255, d_out=d_jac1.data_ptr())
    else:
        d_srs = on_device(points)
        m.p1s_mult_pippenger_many_device(cache, d_srs.data_ptr(), n, d_sc1.data_ptr(), None, 2 * K, 255, d_out=d_jac1.data_ptr())
    m.p1s_to_affine_device(cache, d_jac1.data_ptr(), 2 * K, d_cpi.data_ptr())
    # [tau - z_g]G2 next to G2 itself, in the order the pairs take them: member 2 g is [1]G2, member 2 g + 1 is [1][tau]G2 + [-z_g]G2
    d_pts_g2 = torch.cat([d_g2s[192:], d_g2s]).repeat(K).contiguous()
    offs_g2 = h.offsets_of([1, 2] * K)
    d_jac_q = torch.empty((2 * K * 288,), dtype=torch.uint8, device="cuda")
    d_q = torch.full((2 * K * 192,), 0xaa, dtype=torch.uint8, device="cuda")
    d_sc_g2 = on_device(b"".join(le(1) + le(1) + le(-z) for z in zs))
    m.p2s_mult_pippenger_many_device(cache, d_pts_g2.data_ptr(), 3 * K, d_sc_g2.data_ptr(), offs_g2, 2 * K, 255, d_out=d_jac_q.data_ptr(), ret=False)
    m.p2s_to_affine_device(cache, d_jac_q.data_ptr(), 2 * K, d_q.data_ptr())

    # C_g - [y_g]G1 and -pi_g: member 2 g over (C_g, G1), member 2 g + 1 over (pi_g)
    d_pts_g1 = torch.cat([d_cpi[0::2], d_g1.view(1, 96).expand(K, 96), d_cpi[1::2]], dim=1).contiguous()      # K rows of C_g | G1 | pi_g
    offs_g1 = h.offsets_of([2, 1] * K)
    d_jac_p = torch.empty((2 * K * 144,), dtype=torch.uint8, device="cuda")
    d_p = torch.empty((2 * K * 96,), dtype=torch.uint8, device="cuda")

    def verdicts(claimed):
        d_sc = on_device(b"".join(le(1) + le(-y) + le(-1) for y in claimed))
        m.p1s_mult_pippenger_many_device(cache, d_pts_g1.data_ptr(), 3 * K, d_sc.data_ptr(), offs_g1, 2 * K, 255, d_out=d_jac_p.data_ptr())
        m.p1s_to_affine_device(cache, d_jac_p.data_ptr(), 2 * K, d_p.data_ptr())
        pair_offs = h.offsets_of([2] * K)
        each, status = m.pairingCheckEach_device(cache, d_p.data_ptr(), d_q.data_ptr(), pair_offs, flags=m.PAIR_VALIDATE)
        assert status == [0] * (2 * K)
        return each

    try:
        assert verdicts(ys) == [True] * K
        wrong = list(ys)
        wrong[2] = (wrong[2] + 1) % o.R
        assert verdicts(wrong) == [True, True, False, True, True]                      # a tampered y_g: that group alone
    finally:
        m.p1s_table_destroy(table)
        cache.close()


def test_coefficient_form_openings_over_the_setup(m):
    openings_verify(m, False)


def test_evaluation_form_openings_over_a_lagrange_table(m):
    openings_verify(m, True)
