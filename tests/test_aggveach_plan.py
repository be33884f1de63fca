"""The plan of the per-group aggregateVerify (csrc/plan.hpp aggveach_cut, aggveach_groups, aggveach_measure, aggveach_fill, aggveach_for),
executed through tests/host_emu/plan_aggveach.cpp for group-length lists drawn from {0, 1, 2, C-1, C, C+1, C^2+1, cap-1, cap, cap+1, 3 cap+5} in
seeded orders, for cap 64 and 4096: the slices cover the positions exactly once and hold at most cap pairs, at most one group is open at a
boundary, empty groups occupy nothing, every position is in exactly one level-0 item, every partial is written once and consumed once, and
every group with pairs in a slice has exactly one final item there.  Plus the tail hand-over and the export check of the new C ABI."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pl():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggveach.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_aggveach.so"))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    psz, pu32 = ctypes.POINTER(sz), ctypes.POINTER(u32)
    L.aggveach_plan_c.restype = u32
    L.aggveach_plan_max_levels.restype = u32
    L.aggveach_plan_flags.argtypes = [pu32]
    L.aggveach_plan_walk.argtypes = [psz, sz, sz, u32, psz, pu32, pu32, psz]
    L.aggveach_plan_for.argtypes = [u32, ctypes.c_int, u32, u32, u32, pu32]
    L.aggveach_plan_engine_max.restype, L.aggveach_plan_engine_max.argtypes = u32, [u32]
    L.aggveach_plan_part_words.restype, L.aggveach_plan_part_words.argtypes = sz, [sz]
    L.aggveach_plan_step_words.restype, L.aggveach_plan_step_words.argtypes = sz, [sz]
    return L


def flags(pl):
    out = (ctypes.c_uint32 * 5)()
    pl.aggveach_plan_flags(out)
    return dict(zip(("FINAL", "SIG", "COUNT", "OPEN_IN", "OPEN_OUT"), out))


def walk(pl, lengths, cap, C, first=0):
    """-> [slice dict with its groups and items as integer arrays]"""
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    offs = [first]
    for n in lengths:
        offs.append(offs[-1] + n)
    oa, k = (sz * len(offs))(*offs), len(lengths)
    counts = (sz * 3)()
    pl.aggveach_plan_walk(oa, k, cap, C, None, None, None, counts)
    ns, ngr, nit = counts
    W = 10 + pl.aggveach_plan_max_levels() + 1
    sl, gr, it = (sz * max(ns * W, 1))(), (u32 * max(ngr * 4, 1))(), (u32 * max(nit * 4, 1))()
    pl.aggveach_plan_walk(oa, k, cap, C, sl, gr, it, counts)
    assert tuple(counts) == (ns, ngr, nit)
    sl = np.array(sl[:ns * W], dtype=np.int64).reshape(ns, W)
    gr = np.array(gr[:ngr * 4], dtype=np.int64).reshape(ngr, 4)
    it = np.array(it[:nit * 4], dtype=np.int64).reshape(nit, 4)
    out, ga, ia = [], 0, 0
    for r in sl:
        d = dict(zip(("g0", "g1", "pos0", "pos1", "ng", "open_in", "open_out", "levels", "items", "partials"), (int(x) for x in r[:10])))
        d["level_first"] = [int(x) for x in r[10:10 + d["levels"] + 1]]
        d["groups"], d["tab"] = gr[ga:ga + d["ng"]], it[ia:ia + d["items"]]
        ga, ia = ga + d["ng"], ia + d["items"]
        out.append(d)
    return offs, out


def check(pl, lengths, cap, C, first=0):
    F = flags(pl)
    offs, slices = walk(pl, lengths, cap, C, first)
    k = len(lengths)
    pos = offs[0]
    parts_of = [0] * k                                      # parts a group was walked in
    finals_of = [0] * k
    open_group = None
    for s in slices:
        P = s["pos1"] - s["pos0"]
        assert s["pos0"] == pos and 0 < P <= cap                                        # the slices follow each other and respect the store
        pos = s["pos1"]
        g = s["groups"]
        assert len(g) == s["ng"] >= 1
        # the groups tile the slice's pairs in order, none is empty, and they are the call's groups cut at the slice's ends
        assert g[0, 1] == 0 and (g[1:, 1] == g[:-1, 1] + g[:-1, 2]).all() and g[-1, 1] + g[-1, 2] == P and (g[:, 2] > 0).all()
        assert (np.diff(g[:, 0]) > 0).all()
        for i, (gg, gfirst, cnt, fl) in enumerate(g.tolist()):
            a, b = s["pos0"] + gfirst, s["pos0"] + gfirst + cnt
            assert offs[gg] <= a and b <= offs[gg + 1]
            assert bool(fl & F["OPEN_IN"]) == (a > offs[gg]) and bool(fl & F["OPEN_OUT"]) == (b < offs[gg + 1])
            assert not (fl & F["OPEN_IN"]) or i == 0                                    # only the first group can come from the slice before,
            assert not (fl & F["OPEN_OUT"]) or i == s["ng"] - 1                         # only the last can go on
            parts_of[gg] += 1
        assert bool(g[0, 3] & F["OPEN_IN"]) == bool(s["open_in"]) and bool(g[-1, 3] & F["OPEN_OUT"]) == bool(s["open_out"])
        assert bool(s["open_in"]) == (open_group is not None) and (open_group is None or open_group == g[0, 0])
        open_group = int(g[-1, 0]) if s["open_out"] else None
        if s["open_out"]:
            assert s["ng"] == 1 and P == cap                                            # a part of a long group is a slice of its own
        # the item table
        tab, lf = s["tab"], s["level_first"]
        assert lf[0] == 0 and lf[-1] == s["items"] == len(tab)
        cnt, final, sig = tab[:, 1] & F["COUNT"], (tab[:, 1] & F["FINAL"]) != 0, (tab[:, 1] & F["SIG"]) != 0
        assert (cnt >= 1).all() and (cnt <= C).all()
        l0 = slice(lf[0], lf[1])
        covered = np.zeros(P, dtype=np.int64)
        for f0, c0, seg in zip(tab[l0, 0], cnt[l0], tab[l0, 3]):
            covered[f0:f0 + c0] += 1
            assert g[seg, 1] <= f0 and f0 + c0 <= g[seg, 1] + g[seg, 2]                 # no item across two groups
        assert (covered == 1).all()                                                     # every position in exactly one level-0 item
        written, read = np.zeros(max(s["partials"], 1), dtype=np.int64), np.zeros(max(s["partials"], 1), dtype=np.int64)
        for l in range(s["levels"]):
            for f0, c0, dst, seg, fin in zip(tab[lf[l]:lf[l + 1], 0], cnt[lf[l]:lf[l + 1]], tab[lf[l]:lf[l + 1], 2], tab[lf[l]:lf[l + 1], 3], final[lf[l]:lf[l + 1]]):
                if l > 0:
                    assert (written[f0:f0 + c0] == 1).all()                             # written by a level below
                    read[f0:f0 + c0] += 1
                if fin:
                    assert dst == seg
                    finals_of[g[seg, 0]] += 1
                else:
                    assert dst < s["partials"]
                    written[dst] += 1
        if s["partials"]:
            assert (written == 1).all() and (read == 1).all()                           # every partial written once, consumed once
        assert (np.bincount(tab[final, 3], minlength=s["ng"]) == 1).all()               # one final per group of the slice
        # the signature line: at level 0, once, for every group that ends here
        assert not sig[lf[1]:].any()
        want_sig = (g[:, 3] & F["OPEN_OUT"]) == 0
        assert (np.bincount(tab[l0, 3][sig[l0]], minlength=s["ng"]) == want_sig.astype(np.int64)).all()
        assert pl.aggveach_plan_part_words(s["partials"]) == max(s["partials"], 1) * 68 * 192
        assert pl.aggveach_plan_step_words(s["ng"]) == s["ng"] * 68 * 192
    assert pos == offs[-1] and open_group is None
    for gg, n in enumerate(lengths):
        want = 0 if n == 0 else (1 if n <= cap else (n + cap - 1) // cap)
        assert parts_of[gg] == finals_of[gg] == want, (gg, n)                           # empty groups occupy nothing; one final per part
    return slices


@pytest.mark.parametrize("cap", [64, 4096])
def test_seeded_length_lists(pl, cap):
    C = pl.aggveach_plan_c()
    pool = [0, 1, 2, C - 1, C, C + 1, C * C + 1, cap - 1, cap, cap + 1, 3 * cap + 5]
    rng = random.Random(20260 + cap)
    for trial in range(12):
        lengths = pool[:] if trial == 0 else [rng.choice(pool) for _ in range(rng.randrange(1, 24))]
        rng.shuffle(lengths)
        check(pl, lengths, cap, C)
        check(pl, lengths, cap, 2, first=5 if trial % 2 else 0)                         # offsets need not start at 0; the width the CPU bodies are forced to
    check(pl, [0, 0, 0], cap, C)
    check(pl, [], cap, C)
    assert walk(pl, [0, 0], cap, C)[1] == []


def test_group_of_one_still_takes_its_signature_line(pl):
    F = flags(pl)
    (s,) = check(pl, [1], 64, pl.aggveach_plan_c())
    assert s["tab"].tolist() == [[0, 1 | F["FINAL"] | F["SIG"], 0, 0]] and s["partials"] == 0


def test_levels_of_a_long_group(pl):
    C = pl.aggveach_plan_c()
    (s,) = check(pl, [C * C + 1], 4096, C)
    assert s["levels"] == 3 and s["level_first"] == [0, C + 1, C + 3, C + 4] and s["partials"] == C + 3
    (s,) = check(pl, [9], 64, 2)
    assert s["levels"] == 4


def test_tail_hand_over(pl):
    out = (ctypes.c_uint32 * 5)()
    for S in (1024, 256):
        m = pl.aggveach_plan_engine_max(S)
        for ng, coop, engine in ((1, 1, 1), (m, 1, 1), (m + 1, 1, 0), (1, 0, 0), (m, 0, 0)):
            pl.aggveach_plan_for(S, coop, 4 * ng, ng, ng, out)
            assert out[3] == engine, (S, ng, coop)
            assert out[0] == (5 * ng + 63) // 64 and out[1] == 5 * ng
            assert out[4] == (min(ng, max(S // 2, 1)) if engine else (ng + 63) // 64)


def test_abi_is_declared():
    h = open(os.path.join(HERE, "..", "include", "blscurve_mi355x.h")).read()
    for name in ("mi355_bls_aggregate_verify_each", "mi355_bls_aggregate_verify_each_device", "mi355_bls_debug_aggregate_verify_each_gt"):
        assert re.search(r"\bint %s\(" % name, h), name
