"""The counting sort of the fixed-base table MSM (csrc/msmtable.hpp: owner, point, digit, set, bucket, entry, list start) executed on the CPU
through tests/host_emu/msmtable.cpp: the signed digits of chosen scalars recombine to the scalar, every (pair, window) is bucketed with the
product's own index bodies into set j S + w mod S of its own MSM, the buckets are summed here with the Python oracle over oracle-made table rows
[2^(w wbits)] P_i, and the plain sum of an MSM's sets is compared with the oracle's MSM of that MSM alone."""
import ctypes
import os
import random
import subprocess

import pytest

import bls12381_py as o

HERE = os.path.dirname(os.path.abspath(__file__))
NBITS = (5, 64, 255, 256)
WBITS = (5, 8, 16)
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_msmtable.sh"), "emu"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libmsmtable.so"))
        u32p, sz, u32 = ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_uint32
        L.emu_fixed_digits.argtypes = [ctypes.c_char_p, sz, sz, ctypes.POINTER(ctypes.c_int32)]
        L.emu_fixed_digits.restype = u32
        L.emu_fixed_sort.argtypes = [ctypes.c_char_p, u32, u32, sz, sz, u32] + [u32p] * 5
        L.emu_fixed_sort.restype = ctypes.c_long
        _lib = L
    return _lib


def windows(wbits, nbits):
    return -(-(nbits + 1) // wbits)


def chosen_scalars(rng, wbits, nbits):
    """0, 1, 2^nbits - 1, r - 1, 0x...8000 patterns whose bias carries through every window, alternating digits of +-2^(wbits - 1), random ones"""
    W = windows(wbits, nbits)
    half = 1 << (wbits - 1)
    carry = sum(half << (w * wbits) for w in range(W))                                 # every window exactly at the half: the bias carries through all of them
    alt = sum((half if w % 2 == 0 else half - 1) << (w * wbits) for w in range(W))       # digits -2^(wbits-1) + 2^(wbits-1) ... after the bias: alternating extremes
    full = (1 << 256) - 1                                                              # (the patterns are cut to the 32-byte image)
    return [0, 1, (1 << nbits) - 1, o.R - 1, carry & full, (carry - 1) & full, (carry + 1) & full, alt & full, full ^ (alt & full), full] + [
        rng.getrandbits(256) for _ in range(6)]


@pytest.mark.parametrize("wbits", WBITS)
@pytest.mark.parametrize("nbits", NBITS)
def test_the_signed_digits_recombine_to_the_scalar(wbits, nbits):
    rng = random.Random(wbits * 1000 + nbits)
    W = windows(wbits, nbits)
    digits = (ctypes.c_int32 * 64)()
    for s in chosen_scalars(rng, wbits, nbits):
        assert emu().emu_fixed_digits(s.to_bytes(32, "little"), wbits, nbits, digits) == W
        d = list(digits[:W])
        assert sum(v << (w * wbits) for w, v in enumerate(d)) == s & ((1 << nbits) - 1), (hex(s), d)
        assert all(-(1 << (wbits - 1)) <= v < (1 << (wbits - 1)) for v in d[:-1]) and 0 <= d[-1] <= 1 << (wbits - 1), (hex(s), d)


@pytest.fixture(scope="module")
def points():
    """a few distinct points with cheap multiples, repeated (tests/test_msm_many_emu.py's fixture): 200 points, every eleventh at infinity"""
    rng = random.Random(4)
    base = [o.g1_mul(o.G1_GEN, rng.randrange(1, o.R)) for _ in range(7)]
    return base, [i % 7 if i % 11 != 10 else None for i in range(200)]


_rows = {}


def table_rows(base, wbits, W):
    """oracle-made rows of the seven base points: rows[w][b] = [2^(w wbits)] base[b]"""
    have = _rows.setdefault(wbits, [list(base)])
    while len(have) < W:
        row = []
        for q in have[-1]:
            for _ in range(wbits):
                q = o.g1_add(q, q)
            row.append(q)
        have.append(row)
    return have


def want_msm(base, which, ks, nbits):
    per = {}
    for b, s in zip(which, ks):
        if b is not None:
            per[b] = per.get(b, 0) + (s & ((1 << nbits) - 1))
    key = (nbits, tuple(sorted(per.items())))
    if key not in _wants:
        _wants[key] = o.msm_g1([base[b] for b in per], list(per.values()), 272)
    return _wants[key]


_sums, _wants = {}, {}


def row_sum(rows, wbits, coeff):
    """sum of coeff[w, b] x rows[w][b] with the oracle's additions: one double-and-add walk over all rows at once.  Remembered by its
    coefficients: the same pairs sorted under another S must name the same rows with the same coefficients, and then cost nothing again."""
    key = (wbits, tuple(sorted(coeff.items())))
    if key not in _sums:
        terms = [(o.g1_neg(rows[w][b]) if c < 0 else rows[w][b], abs(c)) for (w, b), c in coeff.items() if c]
        acc = None
        for bit in reversed(range(max([c.bit_length() for _, c in terms] + [0]))):
            acc = o.g1_add(acc, acc)
            for q, c in terms:
                if c >> bit & 1:
                    acc = o.g1_add(acc, q)
        _sums[key] = acc
    return _sums[key]


def check(points, scalars, k, n, wbits, nbits, S):
    base, which = points
    which = which[:n]
    W = windows(wbits, nbits)
    S = min(S, W)
    rows = table_rows(base, wbits, W)
    pairs = k * n
    raw = b"".join(s.to_bytes(32, "little") for s in scalars)
    win = (ctypes.c_uint32 * 14)()
    total = k * S << (wbits - 1)
    hist, offs = (ctypes.c_uint32 * total)(), (ctypes.c_uint32 * total)()
    srt, gb = (ctypes.c_uint32 * (pairs * W))(), (ctypes.c_uint32 * (pairs * W))()
    words = emu().emu_fixed_sort(raw, k, n, wbits, nbits, S, win, hist, offs, srt, gb)
    assert words == pairs * W, "an index left its array"
    assert win[0] == W and win[4] == wbits - 1
    cbk = wbits - 1
    hist, offs, srt, gb = list(hist), list(offs), list(srt), list(gb)
    for j in range(k):
        ks = scalars[j * n:(j + 1) * n]
        # every (pair, window) of MSM j landed in set j S + w mod S, in no other MSM's buckets
        for i in range(n):
            for w in range(W):
                g = gb[(j * n + i) * W + w]
                if g != 0xffffffff:
                    assert g >> cbk == j * S + w % S, (j, i, w, g)
        # The sets' bucket sums over the table rows the sorted words name: set s is worth sum_b (b + 1) B_b with B_b = the signed sum of the rows
        # bucket b lists, and the MSM the plain sum of its sets.  The points repeat, so that sum is taken row by row: every listed entry adds
        # +-(b + 1) to the coefficient of its oracle-made row, and the rows are then combined by the oracle (row_sum).
        coeff = {}
        used = 0
        for s in range(S):
            v = j * S + s
            for b in range(1 << cbk):
                g = (v << cbk) | b
                for e in srt[offs[g]:offs[g] + hist[g]]:
                    assert e != 0xffffffff
                    w, i = divmod(e & 0x7fffffff, n)
                    assert w < W and w % S == s, (j, s, b, e)
                    used += 1
                    if which[i] is not None:
                        coeff[w, which[i]] = coeff.get((w, which[i]), 0) + (-(b + 1) if e >> 31 else b + 1)
        assert row_sum(rows, wbits, coeff) == want_msm(base, which, ks, nbits), (j, wbits, nbits, S)
        assert used == sum(1 for i in range(n) for w in range(W) if gb[(j * n + i) * W + w] != 0xffffffff)
    # the lists of the sets tile `sorted` in order, without overlap
    end = 0
    nb = 1 << cbk
    for v in range(k * S):
        assert offs[v << cbk] >= end, v
        end = offs[(v << cbk) | (nb - 1)] + hist[(v << cbk) | (nb - 1)]
    assert end <= words


@pytest.mark.parametrize("wbits", WBITS)
@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("k", [1, 3])
def test_buckets_through_the_index_bodies(points, k, nbits, wbits):
    rng = random.Random(k * 100000 + nbits * 100 + wbits)
    n = 200 if k == 1 else 23
    W = windows(wbits, nbits)
    scalars = [rng.getrandbits(256) for _ in range(k * n)]
    chosen = chosen_scalars(rng, wbits, nbits)
    scalars[:len(chosen)] = chosen
    for S in sorted({1, min(2, W), W}):
        check(points, scalars, k, n, wbits, nbits, S)
