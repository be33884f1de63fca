"""The host layer's launch plans (csrc/plan.hpp), executed: tests/util.py asks the compiled header (tests/host_emu/plan.cpp), and the literal
tables below pin what it answers - a threshold moved in the product fails here (and against the sizes of tests/golden/latency_handover.json),
instead of leaving tests/test_gpu_latency_handover.py to pass away from the boundaries it is meant to sit on.  The parts of the plan no table
covers (the lines split, the line products' geometry, the slice schedule of a shard) are held to their invariants over exhaustive ranges."""
import bls12381_py as o
import util
from util import golden, latency_hand_overs, latency_plan, lineprod_plan, lines_plan, plan_lib, slice_plan, team_form


def test_mirror_at_s1024():
    """The MI355X plan (256 CUs): the hand-overs of the issue's table, and the plan the fixture's generator recorded."""
    S = 1024
    assert latency_hand_overs(S) == [("clear", 4096), ("clear", 11264), ("side", 16384), ("lines", 4096), ("lines", 18432), ("hash_map", 32768)]
    assert latency_plan(4096, S)["clear"] == "team_spread" and latency_plan(4097, S)["clear"] == "team_wide"
    assert latency_plan(11264, S)["clear"] == "team_wide" and latency_plan(11265, S)["clear"] == "one_lane"
    assert latency_plan(16384, S)["side"] == "fork" and latency_plan(16385, S)["side"] == "fork_sig"
    assert latency_plan(18432, S)["lines"] == "team_wide" and latency_plan(18433, S)["lines"] == "one_lane"
    assert latency_plan(32768, S)["hash_map"] == "spread" and latency_plan(32769, S)["hash_map"] == "plain"
    fx = golden("latency_handover")
    assert fx["slots"] == S
    sizes = [c["n"] for c in fx["cases"]]
    for stage, t in latency_hand_overs(S):
        assert t in sizes and t + 1 in sizes, (stage, t)
        assert latency_plan(t, S)[stage] != latency_plan(t + 1, S)[stage], (stage, t)
    for c in fx["cases"]:
        assert latency_plan(c["n"], S) == c["plan_s1024"], c["n"]


def test_constants():
    assert (util.TEAM_CLEAR_ITEMS_PER_SLOT, util.TEAM_LINES_ITEMS_PER_SLOT, util.SIG_WIDE_MIN, util.FORK_ITEMS_PER_SLOT) == (11, 18, 40000, 16)
    assert (util.WAVE, util.N_LINES, util.SIG_SLOTS_MAX) == (64, 68, 2048)


def test_hand_overs_at_other_device_shapes():
    """304 CUs (S = 1216) and 16 CUs (S = 64): the tables the Python rules gave before the plan was compiled from the product."""
    tables = {1216: [("clear", 4864, "team_spread", "team_wide"), ("clear", 13376, "team_wide", "one_lane"), ("side", 19456, "fork", "fork_sig"),
                     ("lines", 4864, "team_spread", "team_wide"), ("lines", 21888, "team_wide", "one_lane"), ("hash_map", 38912, "spread", "plain")],
              64: [("clear", 256, "team_spread", "team_wide"), ("clear", 704, "team_wide", "one_lane"), ("side", 1024, "fork", "fork_sig"),
                   ("lines", 256, "team_spread", "team_wide"), ("lines", 1152, "team_wide", "one_lane"), ("hash_map", 2048, "spread", "plain")]}
    for S, table in tables.items():
        assert latency_hand_overs(S) == [(stage, t) for stage, t, _, _ in table]
        for stage, t, below, above in table:
            assert (latency_plan(t, S)[stage], latency_plan(t + 1, S)[stage]) == (below, above), (S, stage, t)
        assert latency_plan(39999, S)["extra_pairs"] == 256 and latency_plan(40000, S)["extra_pairs"] == 2048
    # the rows / rows2 steps and the row form of the SSWU map, below 4 S
    assert util.rows_max(1216) == 266 and [team_form(n, 1216) for n in (266, 267, 532, 533)] == ["rows", "rows2", "rows2", "spread"]
    assert util.rows_max(64) == 14 and [team_form(n, 64) for n in (14, 15, 28, 29)] == ["rows", "rows2", "rows2", "spread"]
    assert [latency_plan(n, 1216)["hash_map"] for n in (2128, 2129)] == ["rows", "spread"]
    assert [latency_plan(n, 64)["hash_map"] for n in (112, 113)] == ["rows", "spread"]


def _covers(p, stage, count, S):
    """a stage's grid is the smallest that covers `count` items; an engine form only within its bound"""
    per = 64 if not p[stage + "_team"] else 1 if p[stage + "_form"] < 2 else 4      # items per workgroup: one-lane waves, rows, engine waves
    assert p[stage + "_grid"] >= 1 and (p[stage + "_grid"] - 1) * per < count <= p[stage + "_grid"] * per, (stage, count, p)
    if p[stage + "_team"]:
        assert count <= plan_lib().plan_team_lines_max(S) and util.TEAM_FORMS[p[stage + "_form"]] == team_form(count, S)


def test_lines_plan_properties():
    for S in (64, 1024):
        for coop in (True, False):
            for extra in (0, 256, 2048):
                for npairs in range(max(extra, 1), 20 * S + 2200):
                    p = lines_plan(npairs, extra, S, coop)
                    assert p["main_pairs"] + p["extra_pairs"] == npairs and p["main_pairs"] >= 1 and p["extra_pairs"] in (0, extra)
                    _covers(p, "main", p["main_pairs"], S)
                    if p["extra_pairs"]:
                        assert p["extra_team"] and not p["main_team"]
                        _covers(p, "extra", p["extra_pairs"], S)
                    assert coop or not p["main_team"] and not p["extra_pairs"]       # throughput mode: one lane per pair
    # the split itself, S = 1024: 65 536 tuple pairs are exactly one round of one-lane waves, the 2048 extra pairs would start a second
    assert lines_plan(65536 + 2048, 2048, 1024) == dict(main_pairs=65536, main_team=0, main_form=3, main_grid=1024,
                                                        extra_pairs=2048, extra_team=1, extra_form=2, extra_grid=512)
    assert lines_plan(65536 - 2048 + 2048, 2048, 1024)["extra_pairs"] == 0          # all pairs within that one round


def test_slice_plan_properties():
    for S in (64, 1024):
        for coop, have_side in ((True, True), (True, False), (False, False)):
            for n in list(range(1, 40 * S + 2)) + [65536, 131072, 1 << 20]:
                p = slice_plan(n, S, coop, have_side)
                assert (p["nb"] - 1) * 64 < n <= p["nb"] * 64
                assert (p["cw"], p["nwin"], p["total"]) == ((8, 8, 2048) if n >= 40000 else (4, 16, 256))
                assert p["lshift"] <= 6 and p["bucket_grid"] * 64 >= p["total"] << p["lshift"] > (p["bucket_grid"] - 1) * 64
                assert p["side"] == (0 if not have_side else 1 if n <= 16 * S else 2)
                assert (p["pk_stream"], p["sig_stream"]) == ((0, 0), (2, 1), (0, 1))[p["side"]]
                assert p["pkmul_spread"] == (coop and p["nb"] <= S)
                assert not p["extra_apart"] or p["side"]
                assert p["lines_main_pairs"] + p["lines_extra_pairs"] == (n if p["extra_apart"] else n + p["total"])
                if p["extra_apart"]:
                    _covers(p, "extra_lines", p["total"], S)


def test_line_products_properties():
    for S in (64, 1024, 1216):
        for nblk_cap in (1, 3, 15, 17, 64):
            for npairs in range(1, 9000):
                p = lineprod_plan(S, nblk_cap, 4096, npairs, True)
                assert 1 <= p["nblk"] <= min(nblk_cap, max(S // 68, 1)) and p["m"] >= 1
                assert (p["nblk"] - 1) * 64 * p["m"] < npairs <= p["nblk"] * 64 * p["m"]
                assert p["per"] >= 1 and (p["nb1"] - 1) * p["per"] < p["live"] <= p["nb1"] * p["per"] and p["nb1"] <= p["per"]
                assert 1 <= p["live"] <= min(npairs, p["nblk"] * 64) and p["per_lane"] == 1
                q = lineprod_plan(S, nblk_cap, 4096, npairs, False)
                assert (q["nblk"], q["m"], q["per_lane"], q["live"], q["per"], q["nb1"]) == (p["nblk"], p["m"], 1, 0, 0, 0)
    # the assembly loop's 32-bit byte offsets: stride * 16 * 24 + npairs * 16 < 2^32, the compiled loop from there
    for stride in (11184768, 11184832, 11180032):
        for npairs in range(max(1, (2**32 - stride * 384) // 16 - 70), (2**32 - stride * 384) // 16 + 70):
            assert lineprod_plan(1024, 15, stride, npairs, True)["per_lane"] == (1 if stride * 384 + npairs * 16 < 2**32 else 2), (stride, npairs)


def test_shard_slice_schedule():
    L = plan_lib()
    for cap in range(1, 41):
        for n in range(1, 6 * cap + 2):
            nslices = L.plan_shard_nslices(n, cap)
            assert (nslices - 1) * cap < n <= nslices * cap and L.plan_shard_workspaces(nslices) == min(max(nslices, 2), 3)
            for nl in (1, 2, 3):
                done, counts, where = 0, [], []
                for i in range(nslices):
                    counts.append(L.plan_shard_slice_count(n, done, nslices, i))
                    where.append(L.plan_shard_workspace_of(nslices, i, nl))
                    done += counts[-1]
                assert done == n and max(counts) <= cap and min(counts) >= 1 and max(counts) - min(counts) <= 1, (n, cap, counts)
                assert where[-1] == 0 and all(0 <= w < nl for w in where)
                assert all(where[i] != where[i + 1] for i in range(nslices - 1)) or nl == 1       # neighbouring slices overlap: different workspaces


def test_chunk_of_tuple_is_the_parallel_chunks_partition():
    L = plan_lib()
    pairs = [(n, B) for n in range(1, 41) for B in range(1, n + 1) if B <= 12] + [(1000, 7), (4097, 64), (65536, 48), (12345, 255)]
    assert len(pairs) >= 300
    for n_total, B in pairs:
        for c, (off, cnt) in enumerate(o.parallel_chunks(B, n_total)):
            ts = range(off, off + cnt) if n_total <= 1000 else (off, off + cnt // 2, off + cnt - 1)
            assert all(L.plan_chunk_of_tuple(n_total, B, t) == c for t in ts), (n_total, B, c)
