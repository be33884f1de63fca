"""GPU parity of the Jacobian-to-affine calls (mi355_bls_p1s_to_affine / mi355_bls_p2s_to_affine and their _device forms) with the Python oracle,
byte for byte: both fields, sizes around a wave, the plan's own run length and the test hook's 8 points per lane, infinities at the places the
host emulation test uses, the d_out of the G1 many-MSM call as input, and the argument errors."""
import ctypes
import random

import pytest

import bls12381_py as o
import g2many_helpers as h

pytestmark = pytest.mark.gpu
SIZES = (1, 7, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    yield c
    m.debug_to_affine_set_run(c, 0)


@pytest.fixture(scope="module")
def cases():
    """(g2, n) -> [(Jacobian images, affine images expected)]: made once, shared by both run lengths"""
    out = {}
    for g2 in (False, True):
        for n in SIZES:
            places = h.infinity_placements(n, 8)
            if n == 1000:
                places = [(), tuple(range(496, 504)) + (0, 999, 777)]                 # a whole run of 8, the first and the last point, one alone
            out[(g2, n)] = [h.to_affine_case(g2, n, inf_at, seed=3, unit_z_at=(0, n - 1)) for inf_at in places]
    return out


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("force_run", [0, 8])
def test_both_fields_every_size(m, cache, cases, g2, force_run):
    import torch
    m.debug_to_affine_set_run(cache, force_run)
    host, dev, affb = (m.p2s_to_affine, m.p2s_to_affine_device, 192) if g2 else (m.p1s_to_affine, m.p1s_to_affine_device, 96)
    for n in SIZES:
        assert h.to_affine_plan(n, force_run)[0] == (min(8, force_run) if force_run else 1)      # what the library runs with: C = 1, and C = 8
        for images, want in cases[(g2, n)]:
            assert host(cache, images) == want, (g2, force_run, n)
            d_in = on_device(images)
            d_out = torch.full((n * affb,), 0xaa, dtype=torch.uint8, device="cuda")
            dev(cache, d_in.data_ptr(), n, d_out.data_ptr())
            assert bytes(d_out.cpu().numpy()) == want, (g2, force_run, n)
    m.debug_to_affine_set_run(cache, 0)


def test_the_many_msm_calls_device_output_is_its_input(m, cache):
    import c_oracle as co
    import torch
    rng = random.Random(5)
    lengths = [3, 0, 1, 20, 2]
    n, k = sum(lengths), len(lengths)
    pts = b"".join(co.sk_to_pk(rng.getrandbits(96) | 1) for _ in range(n))
    sc = bytearray(b"".join(rng.getrandbits(255).to_bytes(32, "little") for _ in range(n)))
    pts = pts[:96 * 24] + pts[96 * 24:96 * 25] * 2                                    # the last member: P and P ...
    neg = (o.R - int.from_bytes(sc[32 * 24:32 * 25], "little")) % o.R
    sc[32 * 25:32 * 26] = neg.to_bytes(32, "little")                                  # ... under s and -s: an infinite result among the k
    offs = h.offsets_of(lengths)
    want = [co.msm_g1(pts[96 * a:96 * b], bytes(sc[32 * a:32 * b]), 255) if b > a else bytes(96) for a, b in zip(offs, offs[1:])]
    want[4] = bytes(96)
    dp, ds = on_device(pts), on_device(bytes(sc))
    d_jac = torch.empty((k * 144,), dtype=torch.uint8, device="cuda")
    d_aff = torch.full((k * 96,), 0xaa, dtype=torch.uint8, device="cuda")
    m.p1s_mult_pippenger_many_device(cache, dp.data_ptr(), n, ds.data_ptr(), offs, k, 255, d_out=d_jac.data_ptr())
    m.p1s_to_affine_device(cache, d_jac.data_ptr(), k, d_aff.data_ptr())
    assert bytes(d_aff.cpu().numpy()) == b"".join(want)


def test_argument_errors(m, cache):
    import torch
    L = m.lib()
    buf = torch.zeros((1024,), dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for host, dev in ((L.mi355_bls_p1s_to_affine, L.mi355_bls_p1s_to_affine_device), (L.mi355_bls_p2s_to_affine, L.mi355_bls_p2s_to_affine_device)):
        out = ctypes.create_string_buffer(192)
        assert host(None, bytes(288), 1, out) == -3 and dev(None, p, 1, p + 512, None) == -3
        assert host(cache._h, None, 0, None) == 0 and dev(cache._h, None, 0, None, None) == 0
        assert host(cache._h, None, 1, out) == -3 and host(cache._h, bytes(288), 1, None) == -3
        assert dev(cache._h, None, 1, p + 512, None) == -3 and dev(cache._h, p, 1, None, None) == -3
        assert dev(cache._h, p + 2, 1, p + 512, None) == -3 and dev(cache._h, p, 1, p + 513, None) == -3
        assert dev(cache._h, p, 1, p + 512, None) == 0                                # (the all-zero image: infinity in, infinity out)
    assert bytes(buf.cpu().numpy()) == bytes(1024)
