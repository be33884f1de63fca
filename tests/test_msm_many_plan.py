"""The launch plan of k MSMs in one pass (csrc/plan.hpp msm_many_for / msm_many_next / msm_many_extents / msm_many_sizes_for, asked through
tests/host_emu/plan_msmmany.cpp): for every call of a sweep, every extent fits the workspace the call grows, the grids cover the pairs, buckets
and segments, the virtual windows of a pass respect the grid limit, an MSM has at most 64 windows, the passes cover all MSMs once and in order,
and a member over the per-pass bound is routed to the single path."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CONSTANTS = ("VWIN_MAX", "BUCKETS_MAX", "PAIRS_MAX", "MSM_WINDOWS_MAX", "MSM_TEAM_LANES_MAX", "MSM_SEG", "MSM_ORD_PER", "WAVE", "HEAD", "ROW")
WIN = ("nwin", "wbase", "wrem", "nbits", "cbk") + tuple("H%d" % j for j in range(9))
BUFFERS = ("pts_int", "offs_dev", "hist", "chist", "sorted", "buckets", "segout", "part")
HEAD = WIN + ("shared", "n_ref", "buckets_per_msm", "segs_per_win", "nsplit", "tail_waves", "tail_lanes", "msms_max") + tuple("size_" + b for b in BUFFERS)
ROW = ("single", "j0", "j1", "pair0", "pairs", "points", "nv", "total", "nseg", "pair_grid", "order_grid", "bucket_grid", "team", "segred_grid") + BUFFERS
_lib = None


def plan_lib():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_msmmany.sh"), "plan"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_msmmany.so"))
        u64p, szp = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)
        L.plan_manymsm_constants.argtypes = [u64p]
        L.plan_manymsm_call.argtypes = [szp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, u64p, u64p, ctypes.c_size_t]
        L.plan_manymsm_call.restype = ctypes.c_size_t
        _lib = L
    return _lib


def constants():
    c = (ctypes.c_uint64 * 10)()
    plan_lib().plan_manymsm_constants(c)
    C = dict(zip(CONSTANTS, c))
    assert C["HEAD"] == len(HEAD) and C["ROW"] == len(ROW)
    return C


def call_plan(k, nbits, n=None, lengths=None):
    """-> (head, passes) of a shared call (n points, k MSMs) or a ragged one (lengths)"""
    if lengths is None:
        offs, npoints = None, n
    else:
        acc = [0]
        for v in lengths:
            acc.append(acc[-1] + v)
        offs, npoints, k = (ctypes.c_size_t * len(acc))(*acc), acc[-1], len(lengths)
    head = (ctypes.c_uint64 * len(HEAD))()
    cap = k + 1
    rows = (ctypes.c_uint64 * (cap * len(ROW)))()
    count = plan_lib().plan_manymsm_call(offs, npoints, k, nbits, head, rows, cap)
    assert count <= cap
    return dict(zip(HEAD, head)), [dict(zip(ROW, rows[i * len(ROW):(i + 1) * len(ROW)])) for i in range(count)]


def check_call(k, nbits, n=None, lengths=None):
    C = constants()
    head, passes = call_plan(k, nbits, n, lengths)
    lens = lengths if lengths is not None else [n] * k
    starts = [sum(lens[:j]) for j in range(len(lens))] if lengths is not None and len(lens) < 2000 else None
    nwin, cbk = head["nwin"], head["cbk"]
    assert 1 <= nwin <= 64 == C["MSM_WINDOWS_MAX"] and head["nbits"] == nbits
    assert head["buckets_per_msm"] == nwin << cbk and head["segs_per_win"] * C["MSM_SEG"] == 1 << cbk and head["segs_per_win"] >= 1
    assert head["nsplit"] in (1, 4, 16)
    assert head["tail_lanes"] == head["tail_waves"] * C["WAVE"] <= 1024 and 1 <= head["tail_waves"] <= nwin
    assert head["msms_max"] >= 1
    assert head["shared"] == (lengths is None)
    # the window width comes from the shared n or from the mean member length
    mean = n if lengths is None else max(1, -(-sum(lens) // len(lens)))
    assert head["n_ref"] == max(1, min(mean, C["PAIRS_MAX"]))
    # the passes cover all MSMs once and in order
    at = 0
    for p in passes:
        assert p["j0"] == at and p["j1"] > p["j0"]
        at = p["j1"]
        kp = p["j1"] - p["j0"]
        if starts is not None:
            assert p["pair0"] == starts[p["j0"]]
        elif lengths is None:
            assert p["pair0"] == p["j0"] * n
        if p["single"]:
            assert kp == 1 and (len(lens) == 1 or lens[p["j0"]] > C["PAIRS_MAX"])
            assert all(p[b] == 0 for b in BUFFERS)
            continue
        assert len(lens) > 1 and all(lens[j] <= C["PAIRS_MAX"] for j in range(p["j0"], p["j1"]))
        pairs = sum(lens[p["j0"]:p["j1"]])
        assert p["pairs"] == pairs <= C["PAIRS_MAX"]
        assert kp <= head["msms_max"]
        assert p["nv"] == kp * nwin <= C["VWIN_MAX"] <= 65535                          # no grid axis beyond gridDim.y's limit
        assert p["total"] == p["nv"] << cbk <= C["BUCKETS_MAX"]
        assert p["nseg"] * C["MSM_SEG"] == p["total"]
        assert p["points"] == (n if lengths is None else pairs)
        # a pass is never cut short: the next member would not have fitted
        if p["j1"] < len(lens) and lens[p["j1"]] <= C["PAIRS_MAX"]:
            assert kp == head["msms_max"] or pairs + lens[p["j1"]] > C["PAIRS_MAX"]
        if pairs == 0:
            assert all(p[b] == 0 for b in BUFFERS)
            continue
        # the grids cover the pairs, the buckets and the segments
        assert p["pair_grid"] * C["WAVE"] >= pairs > (p["pair_grid"] - 1) * C["WAVE"]
        assert p["bucket_grid"] * C["WAVE"] >= p["total"]
        assert p["order_grid"] * C["WAVE"] * C["MSM_ORD_PER"] >= p["total"]
        assert p["team"] in (1, 2, 4) and p["segred_grid"] * C["WAVE"] >= p["nseg"] * p["team"]
        assert p["team"] == 1 or p["nseg"] * p["team"] <= C["MSM_TEAM_LANES_MAX"]
        # what the kernels touch, restated from their indexing, and all of it inside what the call grows the workspace to
        assert p["pts_int"] == p["points"] * 128 and p["hist"] == p["total"] * 4 and p["chist"] == 1024
        assert p["offs_dev"] == (0 if lengths is None else (kp + 1) * 4)
        assert p["sorted"] == pairs * nwin * 4 < 1 << 33
        assert p["buckets"] == p["total"] * 192 and p["segout"] == p["nseg"] * 192 and p["part"] == p["nv"] * head["nsplit"] * 192
        for b in BUFFERS:
            assert p[b] <= head["size_" + b], b
    assert at == len(lens)
    for b in BUFFERS:
        assert head["size_" + b] == max([p[b] for p in passes] + [0]), b
    return head, passes


@pytest.mark.parametrize("nbits", [1, 64, 255, 256])
@pytest.mark.parametrize("k", [1, 2, 3, 64, 65, 1000, 70000])
def test_shared_calls(k, nbits):
    for n in (1, 31, 32, 33, 4096, 1 << 16):
        head, passes = check_call(k, nbits, n=n)
        if k == 1:
            assert [p["single"] for p in passes] == [1]
        else:
            assert not any(p["single"] for p in passes)


@pytest.mark.parametrize("nbits", [1, 64, 255, 256])
def test_ragged_calls_with_empties_and_one_long_member(nbits):
    C = constants()
    big = C["PAIRS_MAX"]
    for lengths in ([0, 1, 2, 31, 32, 33, 0, 1000, 1], [0, 0, 0], [5], [0], [7] * 65, [3, 0] * 500, [1] * 70000, [4096] * 64 + [100000],
                    [100, big + 1, 100, 0], [big + 1, big + 1], [big, 1, big], [10, big, 10]):
        head, passes = check_call(len(lengths), nbits, lengths=lengths)
        singles = [p["j0"] for p in passes if p["single"]]
        over = [j for j, v in enumerate(lengths) if v > big] if len(lengths) > 1 else [0]
        assert singles == over, lengths[:8]                                           # exactly the members over the bound take the single path


def test_the_bounds_cut_the_workload_shapes_as_documented():
    """k = 64 x 4 096 is one pass; k = 512 x 4 096 is cut by the pair bound; n = 8 per MSM is cut by the virtual windows"""
    C = constants()
    head, passes = check_call(64, 255, n=4096)
    assert len(passes) == 1 and passes[0]["team"] == 2
    head, passes = check_call(512, 255, n=4096)
    assert [p["j1"] - p["j0"] for p in passes] == [256, 256]
    head8, _ = call_plan(2, 255, n=8)
    head, passes = check_call(head8["msms_max"] + 1, 255, n=8)
    per = C["VWIN_MAX"] // head["nwin"]
    assert head["msms_max"] == per and [p["j1"] - p["j0"] for p in passes] == [per, 1]
