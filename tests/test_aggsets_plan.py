"""The launch plan of the per-set key aggregation (csrc/plan.hpp aggsets_measure / aggsets_fill), executed through
tests/host_emu/plan_aggsets.cpp: level 0 covers every key of every segment exactly once, no item crosses a segment, every item has 1 .. C
operands, every non-empty segment ends with exactly one partial, the levels number ceil(log_C(longest segment)) and the stated buffer size
holds every partial.  Plus the export check of the new C ABI."""
import ctypes
import os
import random
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEVELS = 11


def plan_aggsets_lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggsets.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_aggsets.so"))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    L.aggsets_plan_c.restype = L.aggsets_plan_none.restype = u32
    L.aggsets_plan_measure.argtypes = [ctypes.POINTER(sz), sz, ctypes.POINTER(u32), ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.aggsets_plan_fill.argtypes = [ctypes.POINTER(sz), sz, ctypes.c_void_p, ctypes.c_void_p]
    return L


def aggsets_plan(L, lengths, first=0):
    """-> (levels, level_first, items as a (n, 4) array of src_first, count, dst, seg, final_of) for segments of these lengths"""
    import numpy as np
    offs = np.concatenate(([first], first + np.cumsum(np.asarray(lengths, dtype=np.uint64)))).astype(np.uint64)
    k = len(lengths)
    po = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
    levels, n_items = ctypes.c_uint32(), ctypes.c_size_t()
    lf = (ctypes.c_size_t * (MAX_LEVELS + 1))()
    assert L.aggsets_plan_measure(po, k, ctypes.byref(levels), lf, ctypes.byref(n_items)) == 1
    items = np.zeros((n_items.value, 4), dtype=np.uint32)
    final_of = np.zeros(k, dtype=np.uint32)
    assert L.aggsets_plan_fill(po, k, items.ctypes.data, final_of.ctypes.data) == 1
    return levels.value, list(lf)[:levels.value + 1], items, final_of


@pytest.fixture(scope="module")
def pl():
    return plan_aggsets_lib()


def ceil_log(C, n):
    lv, reach = 0, 1
    while reach < n:
        reach *= C
        lv += 1
    return lv


def cases(C):
    rng = random.Random(20261017)
    return [[1], [0], [0, 1, 0], [C - 1, C, C + 1], [C * C, C * C + 1], [64 * C + 1], [1] * 65536, [1 << 20], [rng.randint(0, 2100) for _ in range(700)]]


def check(L, lengths, first=0):
    import numpy as np
    C, NONE = L.aggsets_plan_c(), L.aggsets_plan_none()
    levels, lf, items, final_of = aggsets_plan(L, lengths, first)
    lengths = np.asarray(lengths, dtype=np.int64)
    k, n_keys = len(lengths), int(lengths.sum())
    offs = first + np.concatenate(([0], np.cumsum(lengths)))
    src, cnt, dst, seg = (items[:, j].astype(np.int64) for j in range(4))
    # the levels and the buffer
    longest = int(lengths.max()) if k else 0
    assert levels == (max(1, ceil_log(C, longest)) if longest else 0)
    assert lf[0] == 0 and lf[-1] == len(items) and all(a <= b for a, b in zip(lf, lf[1:]))
    # proportional to the keys plus k: a segment of n keys has at most n / C + n / C^2 + ... < n / (C - 1) items plus one rounding per level,
    # and at most 2 + n / C levels
    assert len(items) <= n_keys / (C - 1) + n_keys / C + 2 * k
    assert ((cnt >= 1) & (cnt <= C)).all()
    assert (dst == np.arange(len(items))).all() and (dst < lf[-1]).all()                  # every partial has a slot of its own inside the stated size
    assert (seg < k).all()
    # level 0: every key exactly once, inside its own segment
    a, b = lf[0], lf[1] if levels else 0
    cover = np.zeros(n_keys + 1, dtype=np.int64)
    np.add.at(cover, src[a:b] - first, 1)
    np.add.at(cover, src[a:b] + cnt[a:b] - first, -1)
    assert (np.cumsum(cover)[:n_keys] == 1).all() and cover.sum() == 0
    assert (src[a:b] >= offs[seg[a:b]]).all() and (src[a:b] + cnt[a:b] <= offs[seg[a:b] + 1]).all()
    # higher levels: every partial of the level below that is not its segment's last one is read exactly once, by an item of its own segment
    live = np.zeros(len(items), dtype=bool)                     # partials that are some segment's result
    has = final_of != NONE
    assert (has == (lengths > 0)).all()
    live[final_of[has]] = True
    assert (seg[final_of[has]] == np.nonzero(has)[0]).all()
    reads = np.zeros(len(items) + 1, dtype=np.int64)
    for l in range(1, levels):
        a, b = lf[l], lf[l + 1]
        assert (src[a:b] >= lf[l - 1]).all() and (src[a:b] + cnt[a:b] <= lf[l]).all()     # operands: partials of the level below
        np.add.at(reads, src[a:b], 1)
        np.add.at(reads, src[a:b] + cnt[a:b], -1)
        for j in (0, -1):                                       # first and last operand belong to the item's segment (operands are consecutive,
            at = src[a:b] + (cnt[a:b] - 1 if j else 0)          # and a segment's partials of one level are consecutive)
            assert (seg[at] == seg[a:b]).all()
    nreads = np.cumsum(reads)[:len(items)]
    assert (nreads + live == 1).all()                           # read once, or the end of its segment: never both, never neither
    return levels, lf, items, final_of


def test_plan_properties(pl):
    C = pl.aggsets_plan_c()
    assert C == 8
    for lengths in cases(C):
        check(pl, lengths)
    check(pl, [3, 0, C + 2, 1], first=5)                         # offsets need not start at 0


def test_shapes_without_a_degenerate_launch(pl):
    C = pl.aggsets_plan_c()
    levels, lf, items, _ = aggsets_plan(pl, [1] * 65536)
    assert (levels, lf) == (1, [0, 65536])
    levels, lf, items, final_of = aggsets_plan(pl, [1 << 20])
    assert levels == 7 and [b - a for a, b in zip(lf, lf[1:])] == [(1 << 20) // C ** (l + 1) or 1 for l in range(7)]
    assert final_of[0] == len(items) - 1
    assert aggsets_plan(pl, [0, 0])[0] == 0 and len(aggsets_plan(pl, [0, 0])[2]) == 0
    for j in range(1, 5):
        for d, want in ((-1, j), (0, j), (1, j + 1)):
            assert aggsets_plan(pl, [C ** j + d])[0] == want, (j, d)                  # C^j - 1 and C^j keys: j levels; one more key: one more level


def test_plan_refuses_decreasing_offsets(pl):
    offs = (ctypes.c_size_t * 3)(0, 5, 4)
    levels, items = ctypes.c_uint32(), ctypes.c_size_t()
    lf = (ctypes.c_size_t * (MAX_LEVELS + 1))()
    assert pl.aggsets_plan_measure(offs, 2, ctypes.byref(levels), lf, ctypes.byref(items)) == 0
    offs = (ctypes.c_size_t * 2)(0, 1 << 32)
    assert pl.aggsets_plan_measure(offs, 1, ctypes.byref(levels), lf, ctypes.byref(items)) == 0


def test_new_entry_points_are_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    m = ge.load_package()
    hdr = open(m.HEADER_PATH).read()
    names = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in ("mi355_bls_aggregate_sets", "mi355_bls_aggregate_sets_device", "mi355_bls_fast_aggregate_verify_each",
              "mi355_bls_fast_aggregate_verify_each_device", "mi355_bls_batch_fast_aggregate_verify", "mi355_bls_batch_fast_aggregate_verify_device"):
        assert n in names, n
        assert hasattr(L, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    assert exported == names, (sorted(exported - names), sorted(names - exported))
    for f in ("aggregateSets", "aggregateSets_device", "fastAggregateVerifyEach", "fastAggregateVerifyEach_device", "batchFastAggregateVerify",
              "batchFastAggregateVerify_device"):
        assert callable(getattr(m, f))
    with pytest.raises(ValueError):
        m.aggregateSets(None, [bytes(95)], bytes(32), bytes(192))          # refused before the cache is touched
    with pytest.raises(ValueError):
        m.fastAggregateVerifyEach(None, [bytes(96)], bytes(64), bytes(192))
    with pytest.raises(ValueError):
        m.batchFastAggregateVerify(None, [bytes(96)], bytes(32), bytes(192), bytes(31))
    assert m.fastAggregateVerifyEach(None, [], b"", b"") == []
