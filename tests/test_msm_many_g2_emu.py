"""The Horner walk of the G2 per-MSM tail (csrc/msmmany.hpp many_tail_walk, what wave 0 of k_pip_tail_many_g2 runs) executed on the host with
the plain jac_dbl / jac_add formulas under the bounds tracker (tests/host_emu/msmmany_g2.cpp), over window sums made with the Python oracle
from the product's own digits: the result is the oracle's MSM; an empty top window and an MSM of empty windows cost no doubling; a walk that
meets 2^width acc == +-R_w ends where the oracle says."""
import ctypes
import random

import pytest

import bls12381_py as o
import g2many_helpers as h
from util import LAMBDAS_FP2, g2_jac_image, g2_jac_to_affine


def walk(sums, n_ref, nbits):
    """sums: affine points (None = infinity), window 0 first -> (affine result, doublings, additions)"""
    images = b"".join(g2_jac_image(p, LAMBDAS_FP2[(3 * i + 1) % len(LAMBDAS_FP2)]) for i, p in enumerate(sums))
    out, counts = ctypes.create_string_buffer(288), (ctypes.c_uint32 * 3)()
    h.tail_lib().emu_g2_tail_walk(images, n_ref, nbits, out, counts)
    got = g2_jac_to_affine(out.raw)
    if got is None:
        assert out.raw == bytes(288)                                                  # an infinite result is 288 zero bytes
    return got, counts[0], counts[1]


def window_sums(points, scalars, n_ref, nbits):
    nwin, _ = h.windows(n_ref, nbits)
    sums = [None] * nwin
    for p, k in zip(points, scalars):
        for w, d in enumerate(h.digits(k, n_ref, nbits)):
            if d and p is not None:
                sums[w] = o.g2_add(sums[w], o.g2_mul(p, d) if d > 0 else o.g2_neg(o.g2_mul(p, -d)))
    return sums


@pytest.fixture(scope="module")
def pts():
    rng = random.Random(77)
    return [o.g2_mul(o.G2_GEN, rng.randrange(1, o.R)) for _ in range(6)]


@pytest.mark.parametrize("nbits", [5, 64, 255, 256])
def test_the_walk_over_oracle_window_sums_is_the_msm(pts, nbits):
    rng = random.Random(nbits)
    for n_ref in (1, 4096):                                                           # 5-bit windows, and 9-bit ones
        scalars = [rng.getrandbits(256) for _ in pts]
        scalars[1] = (1 << 256) - 1
        nwin, offs = h.windows(n_ref, nbits)
        assert offs[0] == 0 and offs[nwin] == nbits + 1
        got, dbl, add = walk(window_sums(pts, scalars, n_ref, nbits), n_ref, nbits)
        assert got == h.msm_g2(pts, scalars, nbits), (nbits, n_ref)
        assert dbl <= nbits + 1 - (offs[nwin] - offs[nwin - 1]) and add <= nwin - 1    # at most one doubling per bit below the top window


def test_an_empty_top_window_costs_no_doubling(pts):
    n_ref, nbits = 1, 255
    nwin, offs = h.windows(n_ref, nbits)
    k = (1 << offs[nwin - 2]) * 5 + 3                                                 # nothing in the top window, and none of the others carries into it
    sums = window_sums(pts[:1], [k], n_ref, nbits)
    assert sums[nwin - 1] is None
    top = max(w for w in range(nwin) if sums[w] is not None)
    got, dbl, add = walk(sums, n_ref, nbits)
    assert got == o.g2_mul(pts[0], k) and dbl == offs[top] and add == top            # the walk starts at the first window that holds something


def test_an_msm_of_empty_windows(pts):
    for nbits in (5, 255):
        nwin, _ = h.windows(1, nbits)
        assert walk([None] * nwin, 1, nbits) == (None, 0, 0)
        assert walk(window_sums(pts[:2], [0, 1 << nbits], 1, nbits), 1, nbits) == (None, 0, 0)      # a zero scalar, and one with no bit below nbits


@pytest.mark.parametrize("n_ref", [1, 4096])
def test_the_walk_meets_equal_opposite_and_infinite_operands(pts, n_ref):
    nbits = 255
    nwin, offs = h.windows(n_ref, nbits)
    P = pts[0]
    for w in (nwin - 2, 1):
        width = offs[w + 1] - offs[w]
        Q = o.g2_mul(P, 1 << width)
        for low, name in ((Q, "equal"), (o.g2_neg(Q), "opposite"), (None, "infinite")):
            sums = [None] * nwin
            sums[w + 1], sums[w] = P, low                                             # 2^width acc == +-R_w at window w
            sums[0] = o.g2_add(sums[0], pts[1])                                       # ... and the walk goes on from what that left (w == 1: an addition to it)
            want = None
            for v in range(nwin):
                if sums[v] is not None:
                    want = o.g2_add(want, o.g2_mul(sums[v], 1 << offs[v]))
            got, _, _ = walk(sums, n_ref, nbits)
            assert got == want, (n_ref, w, name)
