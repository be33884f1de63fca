"""The launch plan of the same-message pre-aggregation (csrc/plan.hpp combsets_measure, combsets_chain_on_host), called from the product's
header through tests/host_emu/plan_combsets.cpp: the member range, the chunks of the per-member multiplications, which chains the host
walks, and what the plan refuses."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def plan_combsets_lib():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_combsets.sh"), "plan"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_combsets.so"))
        sz = ctypes.c_size_t
        L.plan_comb_mul_chunk.restype = sz
        L.plan_comb_members_max.restype = sz
        L.plan_combsets_chain_on_host.argtypes = [sz]
        L.plan_combsets_measure.argtypes = [ctypes.POINTER(sz), sz, ctypes.POINTER(sz)]
        _lib = L
    return _lib


def measure(offsets):
    L = plan_combsets_lib()
    sz = ctypes.c_size_t
    out = (sz * 5)()
    ok = L.plan_combsets_measure((sz * len(offsets))(*offsets), len(offsets) - 1, out)
    return bool(ok), dict(zip(("lo", "members", "chunks", "chunk_cap", "host_chains"), out))


def test_constants_match_the_fixture_and_the_kernels():
    from util import golden
    L = plan_combsets_lib()
    assert L.plan_comb_agg_c() == golden("combine_sets")["C"] == 8
    assert L.plan_comb_mul_chunk() % 64 == 0                         # a chunk is whole waves
    assert (L.plan_comb_members_max() + 64) * 16 * 5 // 4 < 1 << 32   # k_pkmul: the byte stride of a row of its SoA output is a 32-bit value (buffer: a quarter of slack)


def test_chain_threshold():
    L = plan_combsets_lib()
    lane_max = L.plan_comb_chain_lane_max()
    assert lane_max >= 512                                           # the bench's largest groups stay on the device
    assert [L.plan_combsets_chain_on_host(n) for n in (0, 1, 2, lane_max, lane_max + 1, 1 << 20)] == [0, 0, 0, 0, 1, 1]


def test_member_range_and_chunks():
    L = plan_combsets_lib()
    chunk, lane_max = L.plan_comb_mul_chunk(), L.plan_comb_chain_lane_max()
    assert measure([0]) == (True, {"lo": 0, "members": 0, "chunks": 0, "chunk_cap": 0, "host_chains": 0})
    assert measure([5, 5, 5]) == (True, {"lo": 5, "members": 0, "chunks": 0, "chunk_cap": 0, "host_chains": 0})
    ok, p = measure([7, 8, 8, 77])
    assert ok and (p["lo"], p["members"], p["chunks"], p["chunk_cap"], p["host_chains"]) == (7, 70, 1, 128, 0)
    for n in (1, 63, 64, 65, chunk - 1, chunk):
        ok, p = measure([0, n])
        assert ok and p["chunks"] == 1 and n <= p["chunk_cap"] <= chunk and p["chunk_cap"] % 64 == 0 and p["chunk_cap"] - n < 64, n
    for n in (chunk + 1, 3 * chunk, 3 * chunk + 1):
        ok, p = measure([0, 3, n])
        assert ok and p["chunks"] == -(-n // chunk) and p["chunk_cap"] == chunk, n
    ok, p = measure([0, lane_max, 2 * lane_max + 1, 2 * lane_max + 3, 4 * lane_max + 5])
    assert ok and p["host_chains"] == 2


def test_refusals():
    L = plan_combsets_lib()
    top = L.plan_comb_members_max()
    assert measure([0, 2, 1])[0] is False
    assert measure([0, top])[0] is True and measure([0, top + 1])[0] is False
    assert measure([10, top + 10])[0] is True                        # the range counts, not the position
