"""The per-batch plan of csrc/plan.hpp (manyeach_cut and the group / item tables built for its slices) through tests/host_emu/plan_manyeach.cpp:
count lists with zeros, ones, a batch equal to the capacity, one over it and slices that sets plus signature slots fill exactly, over several
capacities.  The slices cover every batch once and in order, none exceeds the set workspace or the pair store, a batch that fits no slice is
routed to the single-batch path alone, and the tables of a slice address exactly its sets and its own signature slots."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
C = 8                                     # plan.hpp AGGV_C and AGG_C
FINAL, SIG, COUNT = 0x80000000, 0x40000000, 0x3fffffff
NONE = 0xffffffff


@pytest.fixture(scope="module")
def P():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_manyeach.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_manyeach.so"))
    sz, pu = ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)
    L.manyeach_plan_walk.argtypes = [ctypes.POINTER(sz), sz, sz, sz, ctypes.POINTER(sz), pu, pu, pu, pu, ctypes.POINTER(sz)]
    L.manyeach_plan_walk.restype = None
    L.manyeach_plan_fits_alone.argtypes = [sz, sz, sz]
    L.manyeach_plan_pkmul_spread.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
    return L


def walk(P, counts, cap_sets, cap_pairs):
    """-> [slice dict with its groups, items, sum items and final_of]"""
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    k = len(counts)
    carr = (sz * max(k, 1))(*counts)
    out = (sz * 4)()
    P.manyeach_plan_walk(carr, k, cap_sets, cap_pairs, None, None, None, None, None, out)
    ns, ngr, nit, nsum = list(out)
    sl, gr, it = (sz * (9 * max(ns, 1)))(), (u32 * (4 * max(ngr, 1)))(), (u32 * (4 * max(nit, 1)))()
    su, fo = (u32 * (4 * max(nsum, 1)))(), (u32 * max(ngr, 1))()
    P.manyeach_plan_walk(carr, k, cap_sets, cap_pairs, sl, gr, it, su, fo, out)
    assert list(out) == [ns, ngr, nit, nsum]
    res, g_at, i_at, s_at = [], 0, 0, 0
    for s in range(ns):
        b0, b1, set0, sets, nb, single, n_items, n_sum, levels = sl[9 * s:9 * s + 9]
        d = dict(b0=b0, b1=b1, set0=set0, sets=sets, nb=nb, single=bool(single), groups=[], items=[], sums=[], final_of=[], sum_levels=levels)
        if nb and not single:
            d["groups"] = [tuple(gr[4 * (g_at + i):4 * (g_at + i) + 4]) for i in range(nb)]
            d["final_of"] = list(fo[g_at:g_at + nb])
            d["items"] = [tuple(it[4 * (i_at + i):4 * (i_at + i) + 4]) for i in range(n_items)]
            d["sums"] = [tuple(su[4 * (s_at + i):4 * (s_at + i) + 4]) for i in range(n_sum)]
            g_at, i_at, s_at = g_at + nb, i_at + n_items, s_at + n_sum
        res.append(d)
    return res


def check(P, counts, cap_sets, cap_pairs):
    slices = walk(P, counts, cap_sets, cap_pairs)
    offs = [0]
    for n in counts:
        offs.append(offs[-1] + n)
    at = 0
    for s in slices:
        # every batch once and in order, the sets with them
        assert s["b0"] == at and s["b1"] > at and s["set0"] == offs[at]
        at = s["b1"]
        mine = [b for b in range(s["b0"], s["b1"]) if counts[b]]
        assert s["sets"] == sum(counts[b] for b in mine) and s["nb"] == len(mine)
        if s["single"]:
            # routed to the single-batch path: one batch, alone, and one that indeed fits no slice
            assert len(mine) == 1 and not P.manyeach_plan_fits_alone(counts[mine[0]], cap_sets, cap_pairs)
            continue
        assert s["sets"] <= cap_sets and s["sets"] + s["nb"] <= cap_pairs
        assert all(P.manyeach_plan_fits_alone(counts[b], cap_sets, cap_pairs) for b in mine)
        # greedy: the next non-empty batch did not fit (or is one for the single path)
        nxt = next((b for b in range(s["b1"], len(counts)) if counts[b]), None)
        if nxt is not None and P.manyeach_plan_fits_alone(counts[nxt], cap_sets, cap_pairs):
            assert s["sets"] + counts[nxt] > cap_sets or s["sets"] + counts[nxt] + s["nb"] + 1 > cap_pairs
        if not mine:
            continue
        # the groups: the slice's non-empty batches, their sets end to end, none open
        first = 0
        for (g, f, c, fl), b in zip(s["groups"], mine):
            assert (g, f, c, fl) == (b, first, counts[b], 0)
            first += c
        # the line-product items: level 0 covers every pair of the slice once, within its group; each group's signature slot once, its own
        n, seen, sig_of, finals = s["sets"], [0] * s["sets"], {}, {}
        level0 = sum(-(-c // C) for _, _, c, _ in s["groups"])
        for idx, (src, cw, dst, seg) in enumerate(s["items"]):
            cnt = cw & COUNT
            assert 1 <= cnt <= C and seg < s["nb"]
            if idx < level0:
                _, f, c, _ = s["groups"][seg]
                assert f <= src and src + cnt <= f + c
                for j in range(src, src + cnt):
                    seen[j] += 1
                if cw & SIG:
                    assert seg not in sig_of
                    sig_of[seg] = n + seg                      # where k_aggveach_l0 looks: P + seg
            else:
                assert not cw & SIG
            if cw & FINAL:
                assert seg not in finals and dst == seg
                finals[seg] = idx
        assert seen == [1] * n
        assert sorted(sig_of) == list(range(s["nb"])) == sorted(finals)
        assert all(n <= slot < n + s["nb"] <= cap_pairs for slot in sig_of.values())
        # the G2 sum items: level 0 covers every product once within its batch, and final_of names the item that ends a batch
        seen = [0] * n
        level0 = sum(-(-c // C) for _, _, c, _ in s["groups"])
        for idx, (src, cnt, dst, seg) in enumerate(s["sums"]):
            assert dst == idx and 1 <= cnt <= C
            if idx < level0:
                _, f, c, _ = s["groups"][seg]
                assert f <= src and src + cnt <= f + c
                for j in range(src, src + cnt):
                    seen[j] += 1
        assert seen == [1] * n
        for l, fo in enumerate(s["final_of"]):
            assert fo != NONE and s["sums"][fo][3] == l
            # no later item reads a final partial
            assert all(not (i >= level0 and it[0] <= fo < it[0] + it[1]) for i, it in enumerate(s["sums"]) if i > fo)
    assert at == len(counts)
    return slices


CASES = [
    ([0, 0, 0], 8, 16),
    ([1], 1, 2),
    ([1, 1, 1, 1, 1], 2, 4),
    ([8], 8, 16),                                        # a batch equal to the capacity
    ([9], 8, 16),                                        # one over it: the single path
    ([3, 9, 0, 2, 8, 1], 8, 16),
    ([5, 4, 1], 16, 12),                                 # the pair store binds: 9 sets + 2 slots fit, the batch of one would make 13
    ([4, 4, 2], 16, 13),                                 # 10 sets + 3 slots = 13: filled exactly
    ([4, 4, 2, 1], 16, 13),
    ([7], 8, 7),                                         # fits the sets but not sets + 1: single
    ([100, 1, 2, 3, 0, 7, 8, 9, 64, 65, 257, 513], 2048, 4096),
    ([100, 1, 2, 3, 0, 7, 8, 9, 64, 65, 257, 513], 300, 640),
    ([0, 513, 0, 0, 1], 300, 640),
]


@pytest.mark.parametrize("counts,cap_sets,cap_pairs", CASES)
def test_chosen_lists(P, counts, cap_sets, cap_pairs):
    check(P, counts, cap_sets, cap_pairs)


def test_named_shapes(P):
    s = check(P, [8], 8, 16)
    assert len(s) == 1 and not s[0]["single"] and s[0]["sets"] == 8
    s = check(P, [9], 8, 16)
    assert len(s) == 1 and s[0]["single"]
    s = check(P, [4, 4, 2, 1], 16, 13)
    assert [(x["sets"], x["nb"]) for x in s] == [(10, 3), (1, 1)]                  # 10 + 3 == 13: exactly full, the batch of one starts the next
    s = check(P, [100, 1, 2, 3, 0, 7, 8, 9, 64, 65, 257, 513], 300, 640)
    assert [x["single"] for x in s].count(True) == 1 and next(x for x in s if x["single"])["sets"] == 513
    s = check(P, [100, 1, 2, 3, 0, 7, 8, 9, 64, 65, 257, 513], 2048, 4096)
    assert len(s) == 1 and s[0]["nb"] == 11 and s[0]["sets"] == 1029
    s = check(P, [3, 0, 0], 8, 16)
    assert len(s) == 1 and (s[0]["b0"], s[0]["b1"]) == (0, 3)                       # trailing empty batches ride along


def test_random_lists(P):
    rng = random.Random(20260)
    for _ in range(300):
        cap_sets = rng.choice([1, 2, 3, 8, 9, 64, 65, 100])
        cap_pairs = rng.choice([cap_sets, cap_sets + 1, cap_sets + 3, 2 * cap_sets, 2 * cap_sets + 62])
        pick = [0, 0, 1, 1, 2, 3, 7, 8, 9, cap_sets - 1, cap_sets, cap_sets + 1, 2 * cap_sets + 1, rng.randrange(1, 130)]
        counts = [max(0, rng.choice(pick)) for _ in range(rng.randrange(0, 40))]
        check(P, counts, cap_sets, cap_pairs)


def test_pkmul_form_is_the_batch_paths_rule(P):
    for slots in (4, 1024):
        for n in (1, 64, 65, 64 * slots, 64 * slots + 1):
            assert bool(P.manyeach_plan_pkmul_spread(slots, 1, n)) == (-(-n // 64) <= slots)
            assert not P.manyeach_plan_pkmul_spread(slots, 0, n)
