"""[a]G as 96-byte affine images for lists of scalars, from code that shares nothing with the transforms and FK20 routes under test:
on the device through p1sLincombMany_device over the one-row table of G (golden tests of its own: tests/test_gpu_lincomb.py), on the CPU
through the project's C oracle.  a == 0 is the all-zero image on both."""
import functools

import frntt_cases as fc
import p1ntt_cases as pc

ROW = pc.ROW
INF = bytes(ROW)


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def multiples_of_g(m, cache, scalars):
    """[a]G for each scalar, as affine images, through p1sLincombMany_device over the one-row table of G (a == 0: the all-zero image)"""
    import torch
    count = len(scalars)
    d_tab, d_idx = dev(pc.G_IMAGE), torch.zeros(count, dtype=torch.int32, device="cuda")
    d_sc = dev(b"".join(fc.le(a) for a in scalars))
    d_out = torch.empty((count * ROW,), dtype=torch.uint8, device="cuda")
    _, st = m.p1sLincombMany_device(cache, d_tab.data_ptr(), 1, d_idx.data_ptr(), list(range(count + 1)), d_sc.data_ptr(), d_out.data_ptr())
    assert all(s == (2 if a == 0 else 0) for s, a in zip(st, scalars))
    return host(d_out)


@functools.lru_cache(maxsize=None)
def _oracle_image(a):
    import c_oracle
    return c_oracle.sk_to_pk(a)


@functools.lru_cache(maxsize=None)
def _oracle_format_is_the_fixtures():
    """the oracle's image of [tau]G is the one tests/golden/fk20_cells.json stores as setup entry 1 of n16_l1_x0"""
    import fk20_cells_cases as kc
    srs = kc.rows(bytes.fromhex(kc.case("n16_l1_x0")["setup"]))
    assert _oracle_image(1) == srs[0] == pc.G_IMAGE and _oracle_image(kc.TAU) == srs[1] and srs[1] != srs[0]
    return True


def multiples_of_g_cpu(scalars):
    """the same images from the C oracle's [a]G, its format pinned to a stored fixture image first"""
    assert _oracle_format_is_the_fixtures()
    assert all(0 <= a < fc.R for a in scalars)
    return b"".join(INF if a == 0 else _oracle_image(a) for a in scalars)
