"""The launch plan of the fixed-base table MSM (csrc/plan.hpp fixed_win / fixed_wbits_for / fixed_for / fixed_next / fixed_extents /
fixed_sizes_for, asked through tests/host_emu/plan_msmtable.cpp): over a sweep of table shapes and calls, W = ceil((nbits + 1) / wbits),
1 <= S <= W, every extent fits the workspace the call grows, the grids cover the pairs, buckets and segments, the passes tile the k MSMs without
gap or overlap, table_sizeof is W x npoints x entry bytes, and a table one point beyond the index bound is refused.  The same sweep runs a
second time inside the plan program built stand-alone with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CONSTANTS = ("ENTRIES_MAX", "ENTRY_BYTES", "PAIRS_MAX", "VWIN_MAX", "BUCKETS_MAX", "MSM_TEAM_LANES_MAX", "MSM_SEG", "MSM_ORD_PER", "WAVE", "HEAD", "ROW",
             "SCRATCH_BYTES")
WIN = ("nwin", "wbase", "wrem", "nbits", "cbk") + tuple("H%d" % j for j in range(9))
BUFFERS = ("hist", "chist", "sorted", "buckets", "segout", "part", "out")
HEAD = WIN + ("n", "S", "buckets_per_msm", "segs_per_set", "nsplit", "tail_waves", "tail_lanes", "pairs_max", "msms_max") + tuple("size_" + b for b in BUFFERS)
ROW = ("j0", "j1", "pair0", "pairs", "nv", "total", "nseg", "pair_grid", "order_grid", "bucket_grid", "team", "segred_grid") + BUFFERS
NPOINTS = (1, 2, 63, 64, 65, 4096, 1 << 16, 1 << 20)
NBITS = (1, 5, 64, 255, 256)
KS = (1, 2, 9, 64, 512)
SLOTS = 1024                                                                          # 4 x 256 CUs
_lib = None


def plan_lib():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_msmtable.sh"), "plan"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_msmtable.so"))
        u64p, sz, u32 = ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_uint32
        L.plan_fixed_constants.argtypes = [u64p]
        for name in ("plan_fixed_args_ok", "plan_fixed_table_bytes"):
            getattr(L, name).argtypes = [sz, sz, sz]
            getattr(L, name).restype = ctypes.c_uint64
        L.plan_fixed_wbits_for.argtypes = [sz]
        L.plan_fixed_wbits_for.restype = ctypes.c_uint64
        L.plan_fixed_rows_chunk.argtypes = [sz, u32]
        L.plan_fixed_rows_chunk.restype = ctypes.c_uint64
        L.plan_fixed_call.argtypes = [sz, sz, sz, sz, u32, u32, u32, u64p, u64p, sz]
        L.plan_fixed_call.restype = sz
        _lib = L
    return _lib


def constants():
    c = (ctypes.c_uint64 * 12)()
    plan_lib().plan_fixed_constants(c)
    C = dict(zip(CONSTANTS, c))
    assert C["HEAD"] == len(HEAD) and C["ROW"] == len(ROW)
    return C


def call_plan(npoints, wbits, nbits, k, slots=SLOTS, pairs_max=0, force_S=0):
    """-> (head, passes) of k MSMs over a table of npoints points"""
    head = (ctypes.c_uint64 * len(HEAD))()
    cap = k + 1
    rows = (ctypes.c_uint64 * (cap * len(ROW)))()
    count = plan_lib().plan_fixed_call(npoints, wbits, nbits, k, slots, pairs_max, force_S, head, rows, cap)
    assert count <= cap
    return dict(zip(HEAD, head)), [dict(zip(ROW, rows[i * len(ROW):(i + 1) * len(ROW)])) for i in range(count)]


def windows(wbits, nbits):
    return -(-(nbits + 1) // wbits)


def check_call(npoints, wbits, nbits, k, **kw):
    C = constants()
    head, passes = call_plan(npoints, wbits, nbits, k, **kw)
    W, cbk, S = head["nwin"], head["cbk"], head["S"]
    # uniform windows over nbits + 1 bits, the bias at the top bit of every window but the last
    assert W == windows(wbits, nbits) <= 52 and head["wbase"] == wbits and head["wrem"] == 0 and cbk == wbits - 1 and head["nbits"] == nbits
    bias = sum(head["H%d" % j] << (32 * j) for j in range(9))
    assert bias == sum(1 << (w * wbits + wbits - 1) for w in range(W - 1))
    assert 1 <= S <= W
    if kw.get("force_S"):
        assert S == min(kw["force_S"], W)
    assert head["n"] == npoints and head["buckets_per_msm"] == S << cbk and head["segs_per_set"] * C["MSM_SEG"] == 1 << cbk and head["segs_per_set"] >= 1
    assert head["nsplit"] in (1, 4, 16)
    assert head["tail_lanes"] == head["tail_waves"] * C["WAVE"] <= 1024 and 1 <= head["tail_waves"] <= S
    assert head["msms_max"] >= 1
    pairs_max = kw.get("pairs_max") or C["PAIRS_MAX"]
    assert head["pairs_max"] == pairs_max
    # the passes tile the k MSMs without gap or overlap
    at = 0
    for p in passes:
        assert p["j0"] == at and p["j1"] > p["j0"]
        at = p["j1"]
        kp = p["j1"] - p["j0"]
        assert p["pair0"] == p["j0"] * npoints and p["pairs"] == kp * npoints
        assert kp == 1 or p["pairs"] <= pairs_max
        assert p["pairs"] * W <= C["ENTRIES_MAX"]                                      # list positions and grid sizes stay 32-bit words
        assert kp <= head["msms_max"]
        assert p["nv"] == kp * S <= C["VWIN_MAX"] <= 65535
        assert p["total"] == p["nv"] << cbk <= C["BUCKETS_MAX"]
        assert p["nseg"] * C["MSM_SEG"] == p["total"]
        # a pass is never cut short: the next MSM would not have fitted
        if p["j1"] < k:
            assert kp == head["msms_max"] or p["pairs"] + npoints > pairs_max
        assert p["pair_grid"] * C["WAVE"] >= p["pairs"] > (p["pair_grid"] - 1) * C["WAVE"]
        assert p["bucket_grid"] * C["WAVE"] >= p["total"]
        assert p["order_grid"] * C["WAVE"] * C["MSM_ORD_PER"] >= p["total"]
        assert p["team"] in (1, 2, 4) and p["segred_grid"] * C["WAVE"] >= p["nseg"] * p["team"]
        assert p["team"] == 1 or p["nseg"] * p["team"] <= C["MSM_TEAM_LANES_MAX"]
        # what the kernels touch, restated from their indexing (msm_many's sizes per bucket, segment and part), inside what the call grows
        assert p["hist"] == p["total"] * 4 and p["chist"] == 1024 and p["sorted"] == p["pairs"] * W * 4
        assert p["buckets"] == p["total"] * 192 and p["segout"] == p["nseg"] * 192 and p["part"] == p["nv"] * head["nsplit"] * 192 and p["out"] == kp * 144
        for b in BUFFERS:
            assert p[b] <= head["size_" + b], b
    assert at == k
    for b in BUFFERS:
        assert head["size_" + b] == max(p[b] for p in passes), b
    return head, passes


def index_bound(wbits, nbits):
    return constants()["ENTRIES_MAX"] // windows(wbits, nbits)


@pytest.mark.parametrize("wbits", range(5, 17))
def test_the_sweep(wbits):
    L, C = plan_lib(), constants()
    assert C["ENTRY_BYTES"] == 128 and C["ENTRIES_MAX"] == 1 << 31
    for nbits in NBITS:
        bound = index_bound(wbits, nbits)
        for n in NPOINTS + (bound, bound + 1):
            ok = L.plan_fixed_args_ok(n, wbits, nbits)
            assert ok == (n <= bound), (n, nbits)                                      # refused at the bound + 1, not before
            assert L.plan_fixed_table_bytes(n, wbits, nbits) == (windows(wbits, nbits) * n * C["ENTRY_BYTES"] if ok else 0)
            if not ok:
                continue
            for k in KS:
                check_call(n, wbits, nbits, k)


def test_arguments_create_refuses():
    L = plan_lib()
    for n, wbits, nbits in ((0, 8, 255), (5, 4, 255), (5, 17, 255), (5, 1, 255), (5, 8, 0), (5, 8, 257), (5, 0, 0), ((1 << 31) + 1, 16, 1)):
        assert not L.plan_fixed_args_ok(n, wbits, nbits) and L.plan_fixed_table_bytes(n, wbits, nbits) == 0, (n, wbits, nbits)
    for n in (1, 31, 32, 4096, (1 << 14) - 1, 1 << 14, 1 << 20, 1 << 27):
        c = L.plan_fixed_wbits_for(n)
        assert c == (8 if n < 1 << 14 else 16)                                         # the rule for wbits == 0
        assert L.plan_fixed_args_ok(n, 0, 255)
        assert L.plan_fixed_table_bytes(n, 0, 255) == L.plan_fixed_table_bytes(n, c, 255)


def test_forced_sets_and_a_lowered_pass_bound():
    for wbits, nbits in ((5, 255), (8, 64), (16, 256)):
        W = windows(wbits, nbits)
        for S in (1, 2, W, W + 5):
            head, _ = check_call(65, wbits, nbits, 9, force_S=S)
            assert head["S"] == min(S, W)
    # 9 MSMs of 65 points under a bound of 130 pairs: two MSMs per pass, the last pass one
    _, passes = check_call(65, 8, 255, 9, pairs_max=130)
    assert [p["j1"] - p["j0"] for p in passes] == [2, 2, 2, 2, 1]
    # a bound below one MSM still gives every MSM a pass
    _, passes = check_call(65, 8, 255, 3, pairs_max=10)
    assert [p["j1"] - p["j0"] for p in passes] == [1, 1, 1]


def test_the_rule_for_sets_fills_the_bucket_kernel():
    """S: the fewest sets with which the first pass holds 2 x slots x 64 buckets, within 1 .. W"""
    C = constants()
    for wbits in range(5, 17):
        for n, k in ((4096, 1), (4096, 8), (4096, 64), (4096, 512), (1 << 20, 1), (65, 3)):
            head, passes = call_plan(n, wbits, 255, k)
            fit = max(1, min(k, C["PAIRS_MAX"] // n))
            want = -(-2 * SLOTS * C["WAVE"] // (fit << (wbits - 1)))
            assert head["S"] == max(1, min(want, head["nwin"])), (wbits, n, k)


def test_the_rows_kernel_chunks_stay_inside_the_scratch():
    L, C = plan_lib(), constants()
    for n in (1, 64, 65, 4096, 1 << 20, 1 << 25):
        for W in (1, 16, 22, 52):
            c = L.plan_fixed_rows_chunk(n, W)
            assert 1 <= c <= n and (c == n or c % C["WAVE"] == 0)
            assert c * W * C["ENTRY_BYTES"] <= max(C["SCRATCH_BYTES"], C["WAVE"] * W * C["ENTRY_BYTES"])


def test_the_sanitized_plan_program_runs_the_sweep_clean():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_msmtable.sh"), "san"])
    r = subprocess.run([os.path.join(HERE, "host_emu", "_build", "plan_msmtable_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_msmtable: %d cases" % (12 * len(NBITS) * (len(NPOINTS) + 1) * len(KS)) in r.stdout
