"""The workspace sizes of the per-group signature aggregation (csrc/plan.hpp aggsigs_sizes_for, through tests/host_emu/aggsigs.cpp) held against
aggsets_measure's own numbers (tests/test_aggsets_plan.py's binding): every partial the item table names has a G2 slot, the table and
final_of fit, a flag word and a status byte per group, the two output arrays of the host form - for the fixture's group lengths, for the
plan test's cases and for k = 0."""
import ctypes
import os
import subprocess

import pytest

import aggsigs_cases as ac
from test_aggsets_plan import aggsets_plan, cases, plan_aggsets_lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def libs():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggsigs.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libaggsigs.so"))
    sz = ctypes.c_size_t
    L.aggsigs_plan_sizes.argtypes = [ctypes.POINTER(sz), sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.aggsigs_plan_g2_words.restype = ctypes.c_uint32
    return L, plan_aggsets_lib()


def sizes(L, lengths, first=0):
    offs = [first]
    for n in lengths:
        offs.append(offs[-1] + n)
    out, items = (ctypes.c_size_t * 6)(), ctypes.c_size_t()
    assert L.aggsigs_plan_sizes((ctypes.c_size_t * len(offs))(*offs), len(lengths), out, ctypes.byref(items)) == 1
    return dict(zip(("part", "tab", "bad", "status", "out192", "out96"), out)), items.value


def test_sizes_hold_the_plan(libs):
    L, P = libs
    assert L.aggsigs_plan_g2_words() == 96                      # six Fp elements of 16 words: an internal G2 Jacobian image
    C = P.aggsets_plan_c()
    fx_lengths = [len(g["members"]) for g in ac.fixture()["groups"]]
    assert {1, 2, C - 1, C, C + 1, C * C + 1, 64, 65, 0} <= set(fx_lengths)
    for lengths in [fx_lengths] + [c for c in cases(C) if len(c) < 1000 or sum(c) < 100000] + [[0, 0]]:
        s, items = sizes(L, lengths)
        _, lf, tab, final_of = aggsets_plan(P, lengths)
        k = len(lengths)
        assert items == len(tab) == lf[-1]
        assert s["part"] == max(items, 1) * 96 * 4
        if items:
            assert (int(tab[:, 2].max()) + 1) * 96 * 4 <= s["part"]                       # every dst, and so every src of a higher level, has a slot
        assert s["tab"] == (items * 4 + k) * 4 and s["bad"] == 4 * k and s["status"] == k
        assert s["out192"] == 192 * k and s["out96"] == 96 * k
    assert sizes(L, [3, 0, C + 2, 1], first=5)[0] == sizes(L, [3, 0, C + 2, 1])[0]       # offsets need not start at 0


def test_no_groups(libs):
    L, _ = libs
    s, items = sizes(L, [])
    assert items == 0 and s == {"part": 96 * 4, "tab": 0, "bad": 0, "status": 0, "out192": 0, "out96": 0}


def test_refused_offsets(libs):
    L, _ = libs
    out, items = (ctypes.c_size_t * 6)(), ctypes.c_size_t()
    assert L.aggsigs_plan_sizes((ctypes.c_size_t * 3)(0, 5, 4), 2, out, ctypes.byref(items)) == 0
