"""End to end on the device: k polynomial openings checked by e(C - [y]G1, G2) e(-pi, [tau - z]G2) == 1 with every point produced, normalised and
paired in device memory - commitments and proofs by the G1 many-MSM call, C - [y]G1 and -pi by the same call (ragged), [tau]G2 - [z]G2 by the G2
many-MSM call, both normalised by the to_affine calls, the verdicts by pairing_check_each under MI355_BLS_PAIR_VALIDATE.  Only scalars, offsets
and verdicts cross to or from the host.  The setup is a toy the test makes with the oracle."""
import random

import pytest

import bls12381_py as o
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


def quotient(coeffs, z):
    """p(X) = q(X) (X - z) + p(z) for a cubic p: -> (the three coefficients of q, p(z)), mod r"""
    q = [0, 0, 0]
    carry = 0
    for i in (3, 2, 1):
        carry = (coeffs[i] + carry * z) % o.R
        q[i - 1] = carry
    return q, (coeffs[0] + carry * z) % o.R


def test_openings_verify_without_a_point_crossing_to_the_host(m):
    import torch
    rng = random.Random(2026)
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    tau = rng.randrange(2, o.R)
    srs = [o.g1_mul(o.G1_GEN, pow(tau, i, o.R)) for i in range(4)]
    tau_g2 = o.g2_mul(o.G2_GEN, tau)
    polys = [[rng.randrange(o.R) for _ in range(4)] for _ in range(K)]
    zs = [rng.randrange(o.R) for _ in range(K)]
    qs, ys = zip(*(quotient(p, z) for p, z in zip(polys, zs)))
    assert all(sum(c * pow(z, i, o.R) for i, c in enumerate(p)) % o.R == y for p, z, y in zip(polys, zs, ys))
    d_srs = on_device(b"".join(o.g1_to_blst_affine(p) for p in srs))
    d_g1 = on_device(o.g1_to_blst_affine(o.G1_GEN))
    d_g2s = on_device(o.g2_to_blst_affine(tau_g2) + o.g2_to_blst_affine(o.G2_GEN))

    # C_g and pi_g: 2 K MSMs over the four shared points, member 2 g the polynomial, member 2 g + 1 its quotient
    sc1 = b"".join(b"".join(le(c) for c in p) + b"".join(le(c) for c in q) + le(0) for p, q in zip(polys, qs))
    d_jac1 = torch.empty((2 * K * 144,), dtype=torch.uint8, device="cuda")
    d_cpi = torch.empty((2 * K, 96), dtype=torch.uint8, device="cuda")
    d_sc1 = on_device(sc1)
    m.p1s_mult_pippenger_many_device(cache, d_srs.data_ptr(), 4, d_sc1.data_ptr(), None, 2 * K, 255, d_out=d_jac1.data_ptr())
    m.p1s_to_affine_device(cache, d_jac1.data_ptr(), 2 * K, d_cpi.data_ptr())
    # [tau - z_g]G2 next to G2 itself, in the order the pairs take them: member 2 g is [1]G2, member 2 g + 1 is [1][tau]G2 + [-z_g]G2
    d_pts_g2 = torch.cat([d_g2s[192:], d_g2s]).repeat(K).contiguous()
    offs_g2 = h.offsets_of([1, 2] * K)
    d_jac_q = torch.empty((2 * K * 288,), dtype=torch.uint8, device="cuda")
    d_q = torch.full((2 * K * 192,), 0xaa, dtype=torch.uint8, device="cuda")
    d_sc_g2 = on_device(b"".join(le(1) + le(1) + le(-z) for z in zs))
    assert m.p2s_mult_pippenger_many_device(cache, d_pts_g2.data_ptr(), 3 * K, d_sc_g2.data_ptr(), offs_g2, 2 * K, 255, d_out=d_jac_q.data_ptr(),
                                            ret=False) is None
    m.p2s_to_affine_device(cache, d_jac_q.data_ptr(), 2 * K, d_q.data_ptr())
    want_q = b"".join(o.g2_to_blst_affine(o.G2_GEN) + o.g2_to_blst_affine(o.g2_add(tau_g2, o.g2_neg(o.g2_mul(o.G2_GEN, z)))) for z in zs)
    assert bytes(d_q.cpu().numpy()) == want_q                                          # (read back to check the new calls; the flow below does not need it)

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
        assert status == [0] * (2 * K)                                                # every operand on its curve and in its group
        return each, m.batchPairingCheck_device(cache, d_p.data_ptr(), d_q.data_ptr(), pair_offs, bytes(range(32)), flags=m.PAIR_VALIDATE)

    assert verdicts(ys) == ([True] * K, True)
    wrong = list(ys)
    wrong[2] = (wrong[2] + 1) % o.R
    assert verdicts(wrong) == ([True, True, False, True, True], False)                # a wrong y_g: that group alone
    cache.close()
