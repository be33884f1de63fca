"""The link between fr_open_many's two forms, device-resident: random coefficients are transformed with mi355_bls_fr_ntt_many_device, the
domain comes from mi355_bls_fr_domain_device in the same order, and the evaluation-form opening over them must give, byte for byte, the
values of the coefficient-form opening and the forward transform of its quotient; the inverse transform returns the coefficients."""
import random

import pytest

import fropen_cases as fo
import frntt_cases as fc

pytestmark = pytest.mark.gpu
N, K = 256, 4


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


@pytest.mark.parametrize("bitrev", [False, True])
def test_evaluation_form_opening_of_transformed_coefficients(m, bitrev):
    import torch
    order = m.FR_NTT_BITREV if bitrev else 0
    rng = random.Random(2029 + bitrev)
    coefs = fc.random_vectors(2029, K, N)
    xs = set(fo.domain(N))
    zs = [rng.randrange(fc.R) for _ in range(K)]
    assert not xs & set(zs)                                         # every z outside the domain
    cache = m.BatchedBLSVerifierCache.init(max_sets=64)
    try:
        empty = lambda count: torch.empty((count * 32,), dtype=torch.uint8, device="cuda")      # noqa: E731
        d_coefs, d_zs = dev(fc.pack(coefs)), dev(fc.pack([zs]))
        d_vals, d_dom = empty(K * N), empty(N)
        assert m.frNttMany_device(cache, d_coefs.data_ptr(), N, K, order, None, d_vals.data_ptr()) == (0, bytes(K))
        m.frDomain_device(cache, N, d_dom.data_ptr(), order)
        d_y_c, d_q_c, d_y_e, d_q_e = empty(K), empty(K * N), empty(K), empty(K * N)
        assert m.frOpenMany_device(cache, d_coefs.data_ptr(), N, d_zs.data_ptr(), K, 0, None, d_y_c.data_ptr(), d_q_c.data_ptr()) == (0, bytes(K))
        assert m.frOpenMany_device(cache, d_vals.data_ptr(), N, d_zs.data_ptr(), K, m.FR_OPEN_EVAL, d_dom.data_ptr(), d_y_e.data_ptr(), d_q_e.data_ptr()) == (0, bytes(K))
        assert host(d_y_e) == host(d_y_c) == fo.pack([[fo.evaluate(c, z) for c, z in zip(coefs, zs)]])
        d_q_t = empty(K * N)                                        # the coefficient-form quotient, transformed: the evaluation-form slots
        assert m.frNttMany_device(cache, d_q_c.data_ptr(), N, K, order, None, d_q_t.data_ptr())[0] == 0
        assert host(d_q_e) == host(d_q_t)
        assert m.frNttMany_device(cache, d_vals.data_ptr(), N, K, order | m.FR_NTT_INVERSE)[0] == 0      # in place
        assert host(d_vals) == host(d_coefs) == fc.pack(coefs)
    finally:
        cache.close()
