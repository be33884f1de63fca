"""The counting sort of k MSMs in one pass (csrc/msmmany.hpp: owner, point, digit, bucket, list start) executed on the CPU through
tests/host_emu/msmmany.cpp: every pair is bucketed with the product's own index bodies, the buckets are summed here with the Python oracle,
each MSM's windows are walked, and the result is compared with the oracle's MSM of that member alone.  No pair may land in a virtual window of
another MSM."""
import ctypes
import os
import random
import subprocess

import pytest

import bls12381_py as o

HERE = os.path.dirname(os.path.abspath(__file__))
RAGGED = [0, 1, 2, 31, 32, 33, 0, 100, 1]
NBITS = (5, 64, 255, 256)
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_msmmany.sh"), "emu"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libmsmmany.so"))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L.emu_many_sort.argtypes = [ctypes.c_char_p, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t] + [u32p] * 5
        L.emu_many_sort.restype = ctypes.c_long
        _lib = L
    return _lib


@pytest.fixture(scope="module")
def points():
    """a few distinct points with cheap multiples, repeated (the oracle's additions are what this test spends its time on)"""
    rng = random.Random(4)
    base = [o.g1_mul(o.G1_GEN, rng.randrange(1, o.R)) for _ in range(7)]
    return [base[i % 7] if i % 11 != 10 else None for i in range(200)]          # every eleventh: the point at infinity


def win_off(W, w):
    nwin, wbase, wrem = W[0], W[1], W[2]
    return w * (wbase + 1) if w < wrem else wrem * (wbase + 1) + (w - wrem) * wbase


def sort_pass(scalars, lengths, shared_n, nbits):
    """-> W (14 words), hist, offs, sorted, gb, words; lengths: the ragged members, or None with shared_n points per MSM and k = pairs / n"""
    pairs = len(scalars)
    if lengths is None:
        k, offs, n = pairs // shared_n, None, shared_n
    else:
        k, n = len(lengths), 0
        acc = [0]
        for v in lengths:
            acc.append(acc[-1] + v)
        offs = (ctypes.c_uint32 * (k + 1))(*acc)
    raw = b"".join(s.to_bytes(32, "little") for s in scalars)
    W = (ctypes.c_uint32 * 14)()
    total_cap = k * 64 * 256                                                       # at most 64 windows; 2^cbk <= 256 buckets each at these sizes (asserted below)
    hist, offs_out = (ctypes.c_uint32 * total_cap)(), (ctypes.c_uint32 * total_cap)()
    srt, gb = (ctypes.c_uint32 * (pairs * 64))(), (ctypes.c_uint32 * (pairs * 64))()
    words = emu().emu_many_sort(raw, offs, pairs, k, n, nbits, W, hist, offs_out, srt, gb)
    assert words >= 0, "an index left its array"
    W = list(W)
    assert W[0] <= 64 and W[4] <= 8 and words == pairs * W[0]
    return W, hist, offs_out, srt, gb, k


def want_msm(P, ks, nbits):
    """o.msm_g1 of one MSM alone.  The points repeat, so the scalars (mod 2^nbits) of equal points are added first: the same sum with seven
    scalar multiplications of the pure-Python oracle instead of one per pair."""
    per = {}
    for q, s in zip(P, ks):
        if q is not None:
            per[q] = per.get(q, 0) + (s & ((1 << nbits) - 1))
    return o.msm_g1(list(per), list(per.values()), 272)


def check(points_of, scalars, lengths, shared_n, nbits):
    """points_of(j): the points of MSM j, in order; scalars: by pair"""
    W, hist, offs, srt, gb, k = sort_pass(scalars, lengths, shared_n, nbits)
    nwin, cbk = W[0], W[4]
    nb = 1 << cbk
    pair0 = 0
    for j in range(k):
        P = points_of(j)
        n_j = len(P)
        ks = scalars[pair0:pair0 + n_j]
        # every pair of MSM j met only virtual windows j nwin .. j nwin + nwin - 1, each window w at v = j nwin + w
        seen = set()
        for i in range(n_j):
            for w in range(nwin):
                g = gb[(pair0 + i) * nwin + w]
                if g != 0xffffffff:
                    assert g >> cbk == j * nwin + w, (j, i, w, g)
                    seen.add(g >> cbk)
        assert seen <= set(range(j * nwin, (j + 1) * nwin)), j
        # bucket sums from the sorted lists, window sums, the Horner walk from the top window down
        acc = None
        for w in reversed(range(nwin)):
            v = j * nwin + w
            if w + 1 < nwin:
                for _ in range(win_off(W, w + 1) - win_off(W, w)):
                    acc = o.g1_add(acc, acc)
            sums = {}
            for b in range(nb):
                g = (v << cbk) | b
                B = None
                for e in srt[offs[g]:offs[g] + hist[g]]:
                    # a point of this MSM: an index into the shared points, or (ragged) into the pass's concatenated points
                    idx = (e & 0x7fffffff) - (pair0 if lengths is not None else 0)
                    assert e != 0xffffffff and 0 <= idx < n_j, (j, w, b, e)
                    q = P[idx]
                    B = o.g1_add(B, o.g1_neg(q) if e >> 31 else q)
                if B is not None:
                    sums[b] = B
            # the window's value sum (b + 1) B_b: running sums from the top bucket down, or - few buckets in use - a multiple per bucket
            S = None
            if len(sums) > 4:
                run = None
                for b in reversed(range(max(sums) + 1)):
                    run = o.g1_add(run, sums.get(b))
                    S = o.g1_add(S, run)
            else:
                for b, B in sums.items():
                    S = o.g1_add(S, o.g1_mul(B, b + 1))
            acc = o.g1_add(acc, S)
        assert acc == want_msm(P, ks, nbits), (j, n_j, nbits)
        pair0 += n_j
    # the lists of the virtual windows tile `sorted` in order, without overlap
    end = 0
    for v in range(k * nwin):
        assert offs[v << cbk] >= end, v
        end = offs[(v << cbk) | (nb - 1)] + hist[(v << cbk) | (nb - 1)]


@pytest.mark.parametrize("nbits", NBITS)
def test_ragged_members_through_the_index_bodies(points, nbits):
    rng = random.Random(nbits)
    starts = [sum(RAGGED[:j]) for j in range(len(RAGGED))]
    scalars = [rng.getrandbits(256) for _ in range(sum(RAGGED))]
    scalars[3] = 0                                                                   # a zero scalar: no bucket in any window
    scalars[40] = (1 << 256) - 1
    check(lambda j: points[starts[j]:starts[j] + RAGGED[j]], scalars, RAGGED, 0, nbits)


@pytest.mark.parametrize("nbits", NBITS)
def test_shared_points_through_the_index_bodies(points, nbits):
    rng = random.Random(100 + nbits)
    k, n = 3, 5
    P = points[:n]
    scalars = [rng.getrandbits(256) for _ in range(k * n)]
    check(lambda j: P, scalars, None, n, nbits)


def test_a_set_built_from_the_products_indices_shows_a_leak():
    """the check above is not vacuous: with the offsets of OTHER lengths the same pairs land in other members' virtual windows"""
    rng = random.Random(9)
    scalars = [rng.getrandbits(255) | 1 for _ in range(6)]
    W, hist, offs, srt, gb, k = sort_pass(scalars, [3, 3], 0, 255)
    nwin, cbk = W[0], W[4]
    owners = {(p, (gb[p * nwin + w] >> cbk) // nwin) for p in range(6) for w in range(nwin) if gb[p * nwin + w] != 0xffffffff}
    assert owners == {(p, p // 3) for p in range(6)}                                 # [3, 3]: pairs 0..2 with MSM 0, 3..5 with MSM 1
    W2, _, _, _, gb2, _ = sort_pass(scalars, [2, 4], 0, 255)
    owners2 = {(p, (gb2[p * W2[0] + w] >> W2[4]) // W2[0]) for p in range(6) for w in range(W2[0]) if gb2[p * W2[0] + w] != 0xffffffff}
    assert owners2 == {(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1)} and owners2 != owners
