"""The launch plan of the key aggregation by participation bits (csrc/plan.hpp aggbits_measure / aggbits_fill), executed through
tests/host_emu/plan_aggbits.cpp: level 0 covers every committee position of every set exactly once in items of at most P positions, no item
spans two sets, the byte offsets tile the packed bit fields exactly, sets that share a committee get items of their own, the levels above
are the segmented sum of aggsets_fill, and the plan refuses decreasing offsets, a committee number that is not there and 2^32 items."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEVELS = 11
C2 = 2 * 64 + 3


def plan_aggbits_lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggbits.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_aggbits.so"))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    L.aggbits_plan_p.restype = L.aggbits_plan_c.restype = L.aggbits_plan_none.restype = u32
    L.aggbits_plan_measure.argtypes = [ctypes.POINTER(sz), sz, ctypes.POINTER(u32), sz, ctypes.POINTER(u32), ctypes.POINTER(sz), ctypes.POINTER(sz),
                                       ctypes.POINTER(sz)]
    L.aggbits_plan_fill.argtypes = [ctypes.POINTER(sz), sz, ctypes.POINTER(u32), sz, ctypes.c_void_p, ctypes.c_void_p]
    return L


def measure(L, c_offsets, which):
    """-> None (refused) | (levels, level_first, items, bits_bytes)"""
    m, k = len(c_offsets) - 1, len(which)
    levels, n_items, nbytes = ctypes.c_uint32(), ctypes.c_size_t(), ctypes.c_size_t()
    lf = (ctypes.c_size_t * (MAX_LEVELS + 1))()
    ok = L.aggbits_plan_measure((ctypes.c_size_t * (m + 1))(*c_offsets), m, (ctypes.c_uint32 * max(k, 1))(*which), k, ctypes.byref(levels), lf,
                                ctypes.byref(n_items), ctypes.byref(nbytes))
    return (levels.value, list(lf)[:levels.value + 1], n_items.value, nbytes.value) if ok else None


def aggbits_plan(L, lengths, which, first=0):
    """-> (levels, level_first, items (n, 4): src_first, count, dst | byte offset, set; sets (k, 4): bits_first, len, committee, final_of;
    bits_bytes) for committees of these lengths and sets naming them"""
    import numpy as np
    c_offsets = [first]
    for n in lengths:
        c_offsets.append(c_offsets[-1] + n)
    got = measure(L, c_offsets, which)
    assert got is not None
    levels, lf, n_items, nbytes = got
    m, k = len(lengths), len(which)
    items, sets = np.zeros((n_items, 4), dtype=np.uint32), np.zeros((k, 4), dtype=np.uint32)
    assert L.aggbits_plan_fill((ctypes.c_size_t * (m + 1))(*c_offsets), m, (ctypes.c_uint32 * max(k, 1))(*which), k, items.ctypes.data, sets.ctypes.data) == 1
    return levels, lf, items, sets, nbytes, c_offsets


@pytest.fixture(scope="module")
def pl():
    return plan_aggbits_lib()


def levels_of(L, P, C):
    """item counts per level of one set whose committee has L positions"""
    out, n = [], -(-L // P)
    while n > 0:
        out.append(n)
        if n == 1:
            break
        n = -(-n // C)
    return out


def check(L, lengths, which, first=0):
    import numpy as np
    P, C, NONE = L.aggbits_plan_p(), L.aggbits_plan_c(), L.aggbits_plan_none()
    levels, lf, items, sets, nbytes, c_offsets = aggbits_plan(L, lengths, which, first)
    k = len(which)
    want = [levels_of(lengths[c], P, C) for c in which]
    assert levels == max([len(w) for w in want] + [0])
    assert [b - a for a, b in zip(lf, lf[1:])] == [sum(w[l] for w in want if len(w) > l) for l in range(levels)]
    assert lf[0] == 0 and lf[-1] == len(items)
    src, cnt, dst, seg = (items[:, j].astype(np.int64) for j in range(4))
    assert (seg < k).all()
    # the set table: fields packed end to end in set order, ceil(L / 8) bytes each
    at = 0
    for s, c in enumerate(which):
        assert tuple(sets[s][:3]) == (at, lengths[c], c), s
        at += (lengths[c] + 7) // 8
    assert nbytes == at
    # level 0: per set, its committee's positions in order, P at a time; the byte offsets tile the set's field
    a, b = lf[0], lf[1] if levels else 0
    tiles = np.zeros(nbytes + 1, dtype=np.int64)
    seen = {}
    for i in range(a, b):
        s = int(seg[i])
        c = which[s]
        j = seen.get(s, 0)                                       # the set's j-th item
        seen[s] = j + 1
        assert src[i] == c_offsets[c] + j * P and cnt[i] == min(P, lengths[c] - j * P) and cnt[i] >= 1, i       # inside its own committee: no item spans two sets
        assert dst[i] == sets[s][0] + j * (P // 8), i
        tiles[dst[i]] += 1
        tiles[dst[i] + (cnt[i] + 7) // 8] -= 1
    assert (np.cumsum(tiles)[:nbytes] == 1).all() and tiles.sum() == 0
    assert all(seen.get(s, 0) == -(-lengths[c] // P) for s, c in enumerate(which))      # sets that share a committee: items of their own
    # above: aggsets_fill's levels over the partials (partial i is written by item i)
    assert (dst[b:] == np.arange(b, len(items))).all()
    reads = np.zeros(len(items) + 1, dtype=np.int64)
    for l in range(1, levels):
        a, b = lf[l], lf[l + 1]
        assert ((cnt[a:b] >= 1) & (cnt[a:b] <= C)).all()
        assert (src[a:b] >= lf[l - 1]).all() and (src[a:b] + cnt[a:b] <= lf[l]).all()
        np.add.at(reads, src[a:b], 1)
        np.add.at(reads, src[a:b] + cnt[a:b], -1)
        for e in (0, -1):
            op = src[a:b] + (cnt[a:b] - 1 if e else 0)
            assert (seg[op] == seg[a:b]).all()
    final = sets[:, 3].astype(np.int64)
    has = final != NONE
    assert (has == np.array([lengths[c] > 0 for c in which], dtype=bool)).all()         # AGG_NONE only for a committee of length 0
    live = np.zeros(len(items), dtype=bool)
    live[final[has]] = True
    assert (seg[final[has]] == np.nonzero(has)[0]).all()
    assert (np.cumsum(reads)[:len(items)] + live == 1).all()
    return levels, lf, items, sets


def test_first_choice_of_p(pl):
    assert pl.aggbits_plan_p() == 8 and pl.aggbits_plan_c() == 8


def test_item_counts_and_levels(pl):
    P, C = pl.aggbits_plan_p(), pl.aggbits_plan_c()
    lengths = [0, 1, 7, 8, 9, 63, 64, 65, C2]
    for c, n in enumerate(lengths):
        levels, lf, items, sets = check(pl, lengths, [c])
        assert [b - a for a, b in zip(lf, lf[1:])] == levels_of(n, P, C)
    want = {0: [], 1: [1], 7: [1], 8: [1], 9: [2, 1], 63: [8, 1], 64: [8, 1], 65: [9, 2, 1], C2: [17, 3, 1]}
    if (P, C) == (8, 8):
        assert {n: levels_of(n, P, C) for n in lengths} == want
    check(pl, lengths, list(range(len(lengths))))
    check(pl, lengths, [8, 0, 3, 3, 7, 1, 0, 8, 2, 6, 5, 4, 4], first=11)      # any order, repeats, offsets need not start at 0


def test_sets_that_share_a_committee_get_distinct_items(pl):
    import numpy as np
    levels, lf, items, sets = check(pl, [65, 9], [0] * 16 + [1, 0])
    l0 = items[:lf[1]]
    assert len(l0) == 17 * 9 + 2
    assert len({(int(r[0]), int(r[3])) for r in l0}) == len(l0)
    assert len(np.unique(l0[:, 2])) == len(l0)                                   # every item its own byte of the fields
    assert len(np.unique(sets[:, 3])) == 18


def test_no_sets_and_empty_committees(pl):
    assert measure(pl, [0, 5], []) == (0, [0], 0, 0)
    assert measure(pl, [0, 0, 0], [0, 1, 1]) == (0, [0], 0, 0)
    check(pl, [0, 0], [0, 1, 1])


def test_refusals(pl):
    assert measure(pl, [0, 5, 4], [0]) is None                                   # decreasing offsets
    assert measure(pl, [0, 5, 4], []) is None
    assert measure(pl, [0, 5], [1]) is None                                      # which >= m
    assert measure(pl, [0, 5], [0, 0, 7]) is None
    assert measure(pl, [0], [0]) is None                                         # no committee at all
    assert measure(pl, [0, 1 << 32], [0]) is None                                # positions are 32-bit
    big = 1 << 31
    per_set = sum(levels_of(big, pl.aggbits_plan_p(), pl.aggbits_plan_c()))
    assert 13 * per_set < (1 << 32) - 1 <= 14 * per_set and 14 * (big // 8) < 1 << 32
    assert measure(pl, [0, big], [0] * 13)[2] == 13 * per_set                    # fits
    assert measure(pl, [0, big], [0] * 14) is None                               # level 0 fits, all levels together do not
    assert measure(pl, [0, big], [0] * 16) is None                               # 2^32 level-0 items
