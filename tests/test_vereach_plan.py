"""The launch plan of per-set verification (csrc/plan.hpp each_for, each_slice_max and the slice schedule), executed through
tests/host_emu/plan_each.cpp: slices cover the input exactly once, the plan is monotone in n, and the executors change exactly at the
committed hand-over sizes.  Plus the export check of the new C ABI."""
import ctypes
import os
import re
import subprocess

import pytest

import util

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("setup_grid", "lines_team", "lines_form", "lines_grid", "lines_pairs", "extra_pairs", "tail_engine", "tail_grid")
SIZES = (1, 2, 63, 64, 65, 4096, 65536, 1 << 20)


def plan_each_lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_vereach.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_each.so"))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    for name, res, args in (("each_plan_slice_max", sz, (sz,)), ("each_plan_stride", sz, (sz,)), ("each_plan_nslices", sz, (sz, sz)),
                            ("each_plan_slice_count", sz, (sz, sz, sz, u32)), ("each_plan_team_clear_max", u32, (u32,)),
                            ("each_plan_team_lines_max", u32, (u32,)), ("each_plan_engine_max", u32, (u32,)), ("each_plan_engine_grid_max", u32, (u32,)),
                            ("each_plan_for", None, (u32, ctypes.c_int, u32, ctypes.POINTER(u32)))):
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


@pytest.fixture(scope="module")
def pl():
    return plan_each_lib()


def each_for(pl, S, coop, m):
    out = (ctypes.c_uint32 * len(FIELDS))()
    pl.each_plan_for(S, int(coop), m, out)
    return dict(zip(FIELDS, out))


def slices(pl, n, cap):
    """[(first, count)] of a call of n sets on a context of `cap`"""
    smax = pl.each_plan_slice_max(cap)
    ns = pl.each_plan_nslices(n, smax)
    out, done = [], 0
    for s in range(ns):
        m = pl.each_plan_slice_count(n, done, ns, s)
        out.append((done, m))
        done += m
    return smax, out


def test_slices_cover_once(pl):
    for cap in (16, 64, 8192, 65536):
        for n in SIZES:
            smax, sl = slices(pl, n, cap)
            assert smax == cap and 2 * smax <= pl.each_plan_stride(cap)               # a call of max_sets sets is one slice; both pairs of every set fit
            at = 0
            for first, m in sl:
                assert first == at and 1 <= m <= smax
                at += m
            assert at == n
            assert len(sl) == -(-n // smax)                                           # no more slices than needed
            assert max(m for _, m in sl) - min(m for _, m in sl) <= 1                 # balanced: never a sliver at the end


def test_monotone_in_n(pl):
    S = 1024
    for coop in (True, False):
        last = None
        for m in sorted(set(SIZES) | set(range(1, 600)) | {4095, 4097, 9216, 9217, 11264, 11265, 33000}):
            if m > 65536:
                continue
            p = each_for(pl, S, coop, m)
            assert p["setup_grid"] == -(-m // 64) and p["lines_pairs"] == 2 * m and p["extra_pairs"] == 0
            if p["tail_engine"]:
                assert coop and p["tail_grid"] == min(m, pl.each_plan_engine_grid_max(S))
            else:
                assert p["tail_grid"] == -(-m // 64)
            key = (0 if p["tail_engine"] else 1, 0 if p["lines_team"] else 1)         # an engine form is never taken back up as n grows
            if last is not None:
                assert all(a <= b for a, b in zip(last[0], key)), (m, last, key)
                if last[0] == key:
                    assert last[1] <= p["tail_grid"], m                               # within a form the grid grows
            last = (key, p["tail_grid"])
    for cap in (64, 8192):
        counts = [len(slices(pl, n, cap)[1]) for n in SIZES]
        assert counts == sorted(counts)


def test_executors_switch_exactly_at_the_hand_overs(pl):
    """profiles/verify_each_sweep.txt: in latency mode the tail on the Fp12 engine up to 7 sets per wave slot, the Miller lines on the
    lane-team engine up to 9 sets (18 pairs) per slot, the cofactor clearing up to 11 messages per slot"""
    for S, engine_max, lines_max, clear_max in ((1024, 7168, 9216, 11264), (1216, 8512, 10944, 13376), (64, 448, 576, 704)):
        assert (pl.each_plan_engine_max(S), pl.each_plan_team_lines_max(S), pl.each_plan_team_clear_max(S)) == (engine_max, lines_max, clear_max)
        assert [each_for(pl, S, True, m)["tail_engine"] for m in (engine_max - 1, engine_max, engine_max + 1)] == [1, 1, 0]
        assert [each_for(pl, S, True, m)["lines_team"] for m in (lines_max - 1, lines_max, lines_max + 1)] == [1, 1, 0]
        assert [util.slice_plan(m, S)["clear_team"] for m in (clear_max - 1, clear_max, clear_max + 1)] == [1, 1, 0]      # the hashing is the batch path's
        for m in (1, 64, engine_max, lines_max, 65536):                              # throughput mode: one lane per item at every size
            p = each_for(pl, S, False, m)
            assert (p["tail_engine"], p["lines_team"]) == (0, 0)
        for m in (1, 200, 448, 449, 4096, 4097):                                     # below the hand-over: the batch path's form for 2 m pairs
            assert util.TEAM_FORMS[each_for(pl, S, True, m)["lines_form"]] == util.team_form(2 * m, S)


def test_new_entry_points_are_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    m = ge.load_package()
    hdr = open(m.HEADER_PATH).read()
    names = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in ("mi355_bls_verify_each", "mi355_bls_verify_each_device", "mi355_bls_batch_verify_locate", "mi355_bls_batch_verify_locate_device",
              "mi355_bls_debug_verify_each_gt", "mi355_bls_debug_verify_each_passes"):
        assert n in names, n
        assert hasattr(L, n), n
    # prototypes and exports stay in one-to-one correspondence
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    assert exported == names, (sorted(exported - names), sorted(names - exported))
    for f in ("verifyEach", "verifyEach_device", "batchVerifyLocate"):
        assert callable(getattr(m, f))
    with pytest.raises(ValueError):
        m.verifyEach(None, bytes(321))                       # refused before the cache is touched
    with pytest.raises(ValueError):
        m.batchVerifyLocate(None, bytes(639), bytes(32))
