"""The cases beyond the fixtures that the FK20 tests share (tests/test_fk20_cells_emu.py on the CPU; tests/test_gpu_fk20_cells.py,
tests/test_gpu_fk20.py and tests/test_gpu_p1s_ntt.py on the device): cells of l >= 16 points, where k_fk20c_sum runs two and three levels,
as polynomials and EXPECTED SCALARS (tests/fk20_scalars.py) - the images are [a]G of those scalars, made by tests/g1_images.py on either
side - and the constants of csrc/plan.hpp at which the Fr transform takes a second pass and a finish shares an inversion.  Nothing here
comes from the code under test."""
import functools
import hashlib
import random

import fk20_cells_cases as kc
import fk20_scalars as ks
import frntt_cases as fc

R = ks.R
BITREV, H = ks.BITREV, ks.H
TAU = kc.TAU
ALL = (0, BITREV, H)
# (n, l, ext, k, flags): the smallest case of ...
SHAPES = (
    (64, 16, 0, 3, ALL),              # two levels (8, then 2), q = 4; N = q: a vector is 2q images wide (k_p1ntt_stage for the inverse)
    (64, 16, 1, 3, ALL),              # the same with N = 2q
    (64, 16, 2, 3, ALL),              # the same with N > 2q (k_fk20c_stage for the inverse)
    (128, 64, 1, 2, ALL),             # two full levels, PeerDAS' l and ext, q = 2
    (512, 64, 1, 2, (BITREV,)),       # the same at q = 8: an inverse with twiddles that are not 1 behind the two-level sum
    (256, 128, 0, 1, ALL),            # three levels (8, 8, 2)
    (1024, 512, 0, 1, (0,)),          # three full levels
)
FORCED = (64, 16, 1, 3)               # the shape the forced passes and the forced tile run


@functools.lru_cache(maxsize=None)
def polynomials(n, l, ext, k):
    """-> (k rows of coefficient IMAGES, the status bytes): random below r, one image of the LAST polynomial is c + r"""
    rng = random.Random("fk20 levels %d %d %d %d" % (n, l, ext, k))
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(k)]
    rows[k - 1][n - 3] += R
    assert rows[k - 1][n - 3] < 1 << 256
    return tuple(tuple(p) for p in rows), bytes([0] * (k - 1) + [kc.REDUCED])


@functools.lru_cache(maxsize=None)
def srs_scalars(n):
    return tuple(ks.srs(TAU, n))


@functools.lru_cache(maxsize=None)
def expected(n, l, ext, k, flags):
    """-> the flat tuple of the scalars of the k output rows; never all zero, and with H zero exactly at h_(q-1)"""
    rows = ks.expected_srs(TAU, polynomials(n, l, ext, k)[0], l, ext, flags)
    q = n // l
    per = q if flags & H else q << ext
    assert all(len(row) == per for row in rows)
    if flags & H:
        assert all(row[q - 1] == 0 and all(row[:q - 1]) for row in rows)
    else:
        assert all(all(row) for row in rows)
    return tuple(a for row in rows for a in row)


# ---- sums_n64: n = 64, l = 16, ext = 1, q = 4, no SRS.  A term of slot `slot` is bilinear in the sub-polynomial c^(v)_u = c_(16 u + v) and
# the sub-setup S^(v)_u = S_(16 u + v), so a relation between sub-sequences holds in every slot of the l-fold sum.  Level 0 adds v = 0 .. 7
# and v = 8 .. 15, level 1 the two results.
SUMS = (64, 16, 1)


def _h(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "little") % R


def _spread(sub):
    """the 16 sub-sequences of 4 entries -> the sequence of 64: entry 16 u + v = sub[v][u]"""
    return [sub[i % 16][i // 16] for i in range(64)]


@functools.lru_cache(maxsize=None)
def sums_n64():
    """-> {name: (setup scalars, rows of coefficients, per row: "finite" | "infinity")}
    equal_halves     S^(v+8) = S^(v).  0: c^(v+8) = c^(v), the two level-0 results are EQUAL and level 1 doubles | 1: c^(v+8) = -c^(v), they
                     are OPPOSITE, every slot and every output is infinity | 2: c^(v+8) = 0, the second result is infinity
    cancelling_pairs additionally S^(2w+1) = -S^(2w).  0: c^(2w+1) = c^(2w), both level-0 groups cancel inside the level and level 1 adds
                     infinity to infinity | 1: c^(2w+1) = 2 c^(2w), the same setup with results that are no infinity"""
    rnd = lambda tag, v: [_h(b"fk20 sums_n64 %s %d %d" % (tag, v, u)) for u in range(4)]      # noqa: E731
    neg = lambda seq: [-a % R for a in seq]                                                    # noqa: E731
    sa = [rnd(b"setup a", v % 8) for v in range(16)]
    c0 = [rnd(b"poly 0", v % 8) for v in range(16)]
    c1 = [rnd(b"poly 1", v) if v < 8 else neg(rnd(b"poly 1", v - 8)) for v in range(16)]
    c2 = [rnd(b"poly 2", v) if v < 8 else [0] * 4 for v in range(16)]
    sb = [rnd(b"setup b", (v % 8) // 2) if v % 2 == 0 else neg(rnd(b"setup b", (v % 8) // 2)) for v in range(16)]
    d0 = [rnd(b"poly b0", v // 2) for v in range(16)]
    d1 = [rnd(b"poly b1", v // 2) if v % 2 == 0 else [2 * a % R for a in rnd(b"poly b1", v // 2)] for v in range(16)]
    out = {"equal_halves": (_spread(sa), [_spread(c0), _spread(c1), _spread(c2)], ("finite", "infinity", "finite")),
           "cancelling_pairs": (_spread(sb), [_spread(d0), _spread(d1)], ("infinity", "finite"))}
    # the relations the names claim, on the sequences themselves
    s, (p0, p1, p2), _ = out["equal_halves"]
    assert all(s) and all(s[i + 8] == s[i] and p0[i + 8] == p0[i] and (p1[i + 8] + p1[i]) % R == 0 and p2[i + 8] == 0 and p0[i] and p1[i] and p2[i]
               for i in range(64) if i % 16 < 8)
    s, (q0, q1), _ = out["cancelling_pairs"]
    assert all(s) and all(s[i + 8] == s[i] for i in range(64) if i % 16 < 8)
    assert all((s[i + 1] + s[i]) % R == 0 and q0[i + 1] == q0[i] and q1[i + 1] == 2 * q1[i] % R and q0[i] and q1[i] for i in range(0, 64, 2))
    return out


@functools.lru_cache(maxsize=None)
def sums_expected(name, flags):
    """-> the flat tuple of expected scalars from the DEFINING sums, with the structure the case claims asserted on them"""
    n, l, ext = SUMS
    s, polys, kinds = sums_n64()[name]
    rows = ks.expected_any(s, polys, l, ext, flags)
    q = n // l
    for row, kind in zip(rows, kinds):
        if kind == "infinity":
            assert not any(row)
        elif flags & H:
            assert row[q - 1] == 0 and all(row[:q - 1])
        else:
            assert all(row)
    return tuple(a for row in rows for a in row)


def plan_constant(pattern):
    """the first group of `pattern` in csrc/plan.hpp, as text"""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nim-blscurve_amd", "csrc", "plan.hpp")) as f:
        return re.search(pattern, f.read()).groups()


def toaff_device_lanes():
    """TOAFF_DEVICE_LANES as csrc/plan.hpp has it: a finish over more elements than this shares an inversion between neighbours (run >= 2)"""
    a, b = plan_constant(r"TOAFF_DEVICE_LANES = (\d+) \* (\d+) \* WAVE;")
    return int(a) * int(b) * int(plan_constant(r"constexpr uint32_t WAVE = (\d+);")[0])


def fr_tile():
    """the default tile of the Fr transform, in elements"""
    return 1 << int(plan_constant(r"FRNTT_TILE_LOG2 = (\d+)")[0])


def cycled(rows, k):
    """k rows: the given ones over and over"""
    return b"".join(rows[g % len(rows)] for g in range(k))


def pack(polys):
    return fc.pack(polys)
