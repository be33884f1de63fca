"""The Lagrange table of an SRS, device-resident: the monomial table [tau^j]G comes from p1sLincombMany_device, its inverse transform
(mi355_bls_p1s_ntt_many_device) is the Lagrange table, the values of K polynomials come from frNttMany_device, and the commitments to the
values over the Lagrange table must equal, byte for byte, the commitments to the coefficients over the monomial table and the image of
[p(tau)]G with p(tau) computed in Python integers - in natural order and with BITREV on both transforms.
With BITREV the evaluation side of each transform is bit-reversed and the other side stays natural: the G1 inverse then READS the monomial
table at bit-reversed slots and still writes the natural Lagrange table, while the Fr forward WRITES the values at bit-reversed slots.  The
DFT matrix does not commute with the bit reversal, so the two only meet with the slots matched: the run hands the inverse the monomial
table gathered at rev(i) and pairs the values with the Lagrange table gathered at rev(i), both gathers device-side copies."""
import pytest

import frntt_cases as fc
import p1ntt_cases as pc

pytestmark = pytest.mark.gpu
N, K = 64, 2
R = pc.R
TAU = 0x5a17e9d3c4b2a1908f7e6d5c4b3a29181706f5e4d3c2b1a0998877665544332211 % R


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


def multiples_of_g(m, cache, scalars, d_out):
    """[a]G for each scalar into d_out, through p1sLincombMany_device over the one-row table of G"""
    import torch
    count = len(scalars)
    d_tab, d_idx = dev(pc.G_IMAGE), torch.zeros(count, dtype=torch.int32, device="cuda")
    d_sc = dev(b"".join(fc.le(a) for a in scalars))
    ok, st = m.p1sLincombMany_device(cache, d_tab.data_ptr(), 1, d_idx.data_ptr(), list(range(count + 1)), d_sc.data_ptr(), d_out.data_ptr())
    assert ok and st == bytes(count)


@pytest.mark.parametrize("bitrev", [False, True])
def test_commitments_over_the_lagrange_table_equal_those_over_the_monomial_table(m, bitrev):
    import torch
    order = m.P1S_NTT_BITREV if bitrev else 0
    assert m.P1S_NTT_BITREV == m.FR_NTT_BITREV and m.P1S_NTT_INVERSE == m.FR_NTT_INVERSE
    coefs = fc.random_vectors(6400 + bitrev, K, N)
    assert TAU and pow(TAU, N, R) != 1                              # tau outside the domain
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    try:
        empty = lambda size: torch.empty((size,), dtype=torch.uint8, device="cuda")      # noqa: E731
        rev = torch.tensor([fc.rev(i, N.bit_length() - 1) for i in range(N)], device="cuda")
        gather = lambda d: d.view(N, 96)[rev].contiguous().view(-1) if bitrev else d      # noqa: E731
        d_mono, d_lagr = empty(N * 96), empty(N * 96)
        multiples_of_g(m, cache, [pow(TAU, j, R) for j in range(N)], d_mono)
        d_mono_eval = gather(d_mono)                                # the monomial table as the inverse's evaluation side holds it
        m.p1sNttMany_device(cache, d_mono_eval.data_ptr(), N, 1, order | m.P1S_NTT_INVERSE, d_lagr.data_ptr())
        d_coefs, d_vals = dev(fc.pack(coefs)), empty(K * N * 32)
        assert m.frNttMany_device(cache, d_coefs.data_ptr(), N, K, order, None, d_vals.data_ptr()) == (0, bytes(K))
        d_jac, d_by_coefs, d_by_vals, d_direct = empty(K * 144), empty(K * 96), empty(K * 96), empty(K * 96)
        m.p1s_mult_pippenger_many_device(cache, d_mono.data_ptr(), N, d_coefs.data_ptr(), None, K, 255, d_jac.data_ptr())
        m.p1s_to_affine_device(cache, d_jac.data_ptr(), K, d_by_coefs.data_ptr())
        d_lagr_vals = gather(d_lagr)                                # entry i: the Lagrange point of the domain element value slot i is taken at
        m.p1s_mult_pippenger_many_device(cache, d_lagr_vals.data_ptr(), N, d_vals.data_ptr(), None, K, 255, d_jac.data_ptr())
        m.p1s_to_affine_device(cache, d_jac.data_ptr(), K, d_by_vals.data_ptr())
        multiples_of_g(m, cache, [sum(c * pow(TAU, j, R) for j, c in enumerate(p)) % R for p in coefs], d_direct)
        want = host(d_direct)
        assert want.count(0) < 16 and host(d_by_coefs) == want and host(d_by_vals) == want
        # the table itself, natural in both runs: L_i(tau) G, L_i the Lagrange polynomial of omega^i
        dom = fc.domain(N)
        ninv = pow(N, -1, R)
        lag = [(pow(TAU, N, R) - 1) * x % R * ninv % R * pow(TAU - x, -1, R) % R for x in dom]
        d_want = empty(N * 96)
        multiples_of_g(m, cache, lag, d_want)
        assert host(d_lagr) == host(d_want)
    finally:
        cache.close()
