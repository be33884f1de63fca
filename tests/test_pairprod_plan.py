"""The plan of the pairing-product calls (csrc/plan.hpp: the sig-less aggveach_fill, pairprod_for, pairprod_blind_cut, pairprod_real_groups,
pairprod_sizes_for) through tests/host_emu/plan_pairprod.cpp: group lengths 1, 2, 7, 8, 9, 63, 64, 65, 513 under slice caps that cut the
longest into one, two, three and nine parts.  Every pair is in exactly one level-0 item, no item has AGGV_SIG, the FINAL items equal the groups
(one per part), the partial counts equal aggveach_measure's, and the defaulted form of aggveach_fill reproduces today's tables bit for bit.
The same sweep runs a second time inside the plan program built stand-alone with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [1, 2, 7, 8, 9, 63, 64, 65, 513]
CAPS = [64, 171, 257, 513, 4096]                     # 513 pairs in nine, three, two parts and one


@pytest.fixture(scope="module")
def pl():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_pairprod.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_pairprod.so"))
    u32, sz, i32 = ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int
    psz, pu32 = ctypes.POINTER(sz), ctypes.POINTER(u32)
    L.pairprod_plan_c.restype = u32
    L.pairprod_plan_flags.argtypes = [pu32]
    L.pairprod_plan_walk.argtypes = [psz, sz, sz, i32, psz, pu32, pu32, psz]
    L.pairprod_plan_blind.argtypes = [psz, sz, sz, psz, pu32, psz]
    L.pairprod_plan_for.argtypes = [u32, i32, u32, u32, i32, pu32]
    L.pairprod_plan_sizes.argtypes = [sz, sz, i32, psz]
    L.pairprod_plan_validate_bit.restype = u32
    return L


@pytest.fixture(scope="module")
def old():
    """the per-group aggregateVerify plan's own library: today's tables"""
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggveach.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_aggveach.so"))
    u32, sz = ctypes.c_uint32, ctypes.c_size_t
    L.aggveach_plan_walk.argtypes = [ctypes.POINTER(sz), sz, sz, u32, ctypes.POINTER(sz), ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(sz)]
    L.aggveach_plan_max_levels.restype = u32
    return L


def flags(pl):
    out = (ctypes.c_uint32 * 5)()
    pl.pairprod_plan_flags(out)
    return dict(zip(("FINAL", "SIG", "COUNT", "OPEN_IN", "OPEN_OUT"), out))


def offsets_of(lengths):
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + n)
    return offs


def walk(pl, lengths, cap, form):
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    offs = offsets_of(lengths)
    oa, k = (sz * len(offs))(*offs), len(lengths)
    counts = (sz * 3)()
    pl.pairprod_plan_walk(oa, k, cap, form, None, None, None, counts)
    ns, ngr, nit = counts
    sl, gr, it = (sz * max(ns * 10, 1))(), (u32 * max(ngr * 4, 1))(), (u32 * max(nit * 4, 1))()
    pl.pairprod_plan_walk(oa, k, cap, form, sl, gr, it, counts)
    return (np.array(sl[:ns * 10], dtype=np.int64).reshape(ns, 10), np.array(gr[:ngr * 4], dtype=np.int64).reshape(ngr, 4),
            np.array(it[:nit * 4], dtype=np.int64).reshape(nit, 4))


def measure(counts, C):
    """aggveach_measure restated: (items, partials) of groups with these pair counts"""
    items = partials = 0
    for n in counts:
        while True:
            n = (n + C - 1) // C
            items += n
            if n == 1:
                break
            partials += n
    return items, partials


def check(pl, lengths, cap):
    F, C = flags(pl), pl.pairprod_plan_c()
    offs = offsets_of(lengths)
    sl, gr, it = walk(pl, lengths, cap, 0)
    finals, parts = [0] * len(lengths), [0] * len(lengths)
    ga = ia = 0
    pos = 0
    for s in sl:
        g0, g1, pos0, pos1, ng, open_in, open_out, levels, items, partials = (int(x) for x in s)
        P = pos1 - pos0
        assert pos0 == pos and 0 < P <= cap
        pos = pos1
        g, tab = gr[ga:ga + ng], it[ia:ia + items]
        assert (items, partials) == measure(g[:, 2].tolist(), C)                      # the partial counts are aggveach_measure's
        assert not (tab[:, 1] & F["SIG"]).any()                                       # no item has a signature line
        cnt, final = tab[:, 1] & F["COUNT"], (tab[:, 1] & F["FINAL"]) != 0
        n0 = sum((int(c) + C - 1) // C for c in g[:, 2])                              # level 0: ceil(count / C) items per group
        covered = np.zeros(P, dtype=np.int64)
        for f0, c0, seg in zip(tab[:n0, 0], cnt[:n0], tab[:n0, 3]):
            covered[f0:f0 + c0] += 1
            assert g[seg, 1] <= f0 and f0 + c0 <= g[seg, 1] + g[seg, 2]               # no item across two groups
        assert (covered == 1).all()                                                   # every pair in exactly one level-0 item
        assert (np.bincount(tab[final, 3], minlength=ng) == 1).all() and (tab[final, 2] == tab[final, 3]).all()
        for gg in g[:, 0]:
            parts[gg] += 1
        for seg in tab[final, 3]:
            finals[g[seg, 0]] += 1
        ga, ia = ga + ng, ia + items
    assert pos == offs[-1]
    for gg, n in enumerate(lengths):
        assert finals[gg] == parts[gg] == (0 if n == 0 else (n + cap - 1) // cap), (gg, n)      # the FINAL items equal the groups' parts
    return sl, gr, it


@pytest.mark.parametrize("cap", CAPS)
def test_sigless_plan_sweep(pl, cap):
    for a in LENGTHS:
        check(pl, [a], cap)
        for b in LENGTHS:
            check(pl, [0, a, 0, b, 0], cap)
            check(pl, [b, a, a], cap)
    check(pl, [], cap)
    check(pl, [0, 0], cap)
    assert len(check(pl, [513], cap)[0]) == (513 + cap - 1) // cap


@pytest.mark.parametrize("cap", [64, 257, 4096])
def test_defaulted_form_reproduces_todays_tables(pl, old, cap):
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    F, C = flags(pl), pl.pairprod_plan_c()
    for lengths in ([1], [513], [0, 9, 0, 65, 0], [64, 63, 513, 8, 7, 2, 1], LENGTHS):
        _, gr1, it1 = walk(pl, lengths, cap, 1)                                       # aggveach_fill(t, gr, ng, items)
        _, gr2, it2 = walk(pl, lengths, cap, 2)
        _, _, it0 = walk(pl, lengths, cap, 0)
        offs = offsets_of(lengths)
        oa, counts = (sz * len(offs))(*offs), (sz * 3)()
        old.aggveach_plan_walk(oa, len(lengths), cap, C, None, None, None, counts)
        W = 10 + old.aggveach_plan_max_levels() + 1
        sl, gr, it = (sz * max(counts[0] * W, 1))(), (u32 * max(counts[1] * 4, 1))(), (u32 * max(counts[2] * 4, 1))()
        old.aggveach_plan_walk(oa, len(lengths), cap, C, sl, gr, it, counts)
        assert it1.flatten().tolist() == it2.flatten().tolist() == list(it[:counts[2] * 4])      # bit for bit
        assert gr1.flatten().tolist() == list(gr[:counts[1] * 4])
        assert (it1[:, 1] & F["SIG"]).any()
        assert (it0[:, [0, 2, 3]] == it1[:, [0, 2, 3]]).all() and (it0[:, 1] == (it1[:, 1] & ~F["SIG"])).all()


def test_blinded_parts_and_their_real_groups(pl):
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    for cap in CAPS:
        for lengths in ([513], [0, 9, 0, 65, 0], [64, 63, 513, 8, 7, 2, 1], [0, 0], [1] * 130):
            offs = offsets_of(lengths)
            oa, counts = (sz * len(offs))(*offs), (sz * 2)()
            pl.pairprod_plan_blind(oa, len(lengths), cap, None, None, counts)
            parts, groups = (sz * max(counts[0] * 6, 1))(), (u32 * max(counts[1] * 4, 1))()
            pl.pairprod_plan_blind(oa, len(lengths), cap, parts, groups, counts)
            assert counts[0] == (offs[-1] + cap - 1) // cap
            owner = [g for g, n in enumerate(lengths) for _ in range(n)]              # the group of every position
            pos = 0
            for p in range(counts[0]):
                pos0, pos1, open_in, open_out, ng, at = parts[6 * p:6 * p + 6]
                assert pos0 == pos and (pos1 - pos0 == cap or pos1 == offs[-1]) and bool(open_in) == (p > 0) and bool(open_out) == (p + 1 < counts[0])
                got = []
                for i in range(ng):
                    g, first, cnt, _ = groups[4 * (at + i):4 * (at + i) + 4]
                    assert first == len(got) and cnt > 0
                    got += [g] * cnt
                assert got == owner[pos0:pos1]                                        # the real groups tile the part
                pos = pos1
            assert pos == offs[-1]


def test_launch_shapes_and_sizes(pl):
    out, s = (ctypes.c_uint32 * 5)(), (ctypes.c_size_t * 3)()
    for slots in (1024, 256):
        for coop in (0, 1):
            pl.pairprod_plan_for(slots, coop, 4096, 1, 1, out)
            assert list(out)[0:2] == [64, 4096] and list(out)[3:] == [1, 1]           # the blinded form: a lane per pair slot, always the engine tail
            pl.pairprod_plan_for(slots, coop, 130, 70, 0, out)
            assert out[0] == 3 and out[1] == 130 and (out[3], out[4]) == ((1, min(70, slots // 2)) if coop else (0, 2))
    pl.pairprod_plan_sizes(1000, 40, 0, s)
    assert list(s) == [1000, 160, 0]
    pl.pairprod_plan_sizes(1000, 40, 1, s)
    assert list(s) == [1000, 4, 320]
    pl.pairprod_plan_sizes(0, 3, 0, s)
    assert list(s) == [1, 12, 0]
    assert pl.pairprod_plan_validate_bit() == 1


def test_the_sanitized_plan_program_runs_the_sweep_clean():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_pairprod.sh"), "san"])
    r = subprocess.run([os.path.join(HERE, "host_emu", "_build", "plan_pairprod_san")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases clean" in r.stdout
