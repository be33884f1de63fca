"""The plans the older half of the host layer follows (csrc/plan.hpp pip_for, msm_for, msm_sizes_for / msm_extents, g1_sum_for / g2_sum_for,
ctx_for), called from the product's header through tests/host_emu/plan.cpp: the window plan of the Pippenger MSM, that every plan fits the
workspace msm_reserve allocates for it and the limits the kernels are written for, that the point sums' partials fit the export area, and that
the context's line-product buffer holds what the line products hand over.  No GPU: the rules are plain integer functions."""
import itertools

import numpy as np
import pytest

import util

NPOINTS = list(range(1, 4097)) + [(1 << j) + d for j in range(13, 29) for d in (-1, 0, 1)]
NBITS = (1, 5, 8, 64, 128, 254, 255, 256)
SLOTS = (4, 64, 416, 1024, 1216, 2048)
MAX_SETS = (1, 64, 65536)


@pytest.fixture(scope="module")
def sweep():
    """{(nbits, g2, allow_split, have_side): plans of NPOINTS}, computed once and left unchanged"""
    return {k: util.msm_plans(NPOINTS, *k) for k in itertools.product(NBITS, (False, True), (False, True), (False, True))}


def test_window_plan(sweep):
    """widths that sum to nbits + 1 and differ by at most a bit, cbk, and the bias H against its definition"""
    for (nbits, *_), p in sweep.items():
        nwin, wbase, wrem, cbk = p["nwin"], p["wbase"], p["wrem"], p["cbk"]
        assert np.all(p["nbits"] == nbits) and np.all(nwin >= 1) and np.all(wrem < nwin)
        assert np.all(wrem * (wbase + 1) + (nwin - wrem) * wbase == nbits + 1)       # wrem windows of wbase + 1 bits, the others of wbase
        widest = wbase + (wrem > 0)
        assert np.all(cbk == np.maximum(widest - 1, 4))
        W = np.stack([nwin, wbase, wrem] + [p["H%d" % j] for j in range(9)], axis=1)
        for row in np.unique(W, axis=0):                                             # every distinct plan of the sweep
            nw, wb, wr = (int(x) for x in row[:3])
            want, off = 0, 0
            for w in range(nw):
                length = wb + 1 if w < wr else wb
                if w + 1 < nw:
                    want += 1 << (off + length - 1)
                off += length
            assert off == nbits + 1
            assert sum(int(h) << (32 * j) for j, h in enumerate(row[3:])) == want, (nbits, nw, wb, wr)
            assert want < 1 << 288 and all(int(h) < 1 << 32 for h in row[3:])


def test_every_plan_fits_its_workspace_and_the_kernels_limits(sweep):
    assert (util.MSM_WINDOWS_MAX, util.MSM_NSPLIT_MAX, util.MSM_GROUPS_MAX, util.MSM_TEAM_LANES_MAX) == (64, 16, 2, 61440)
    for (nbits, g2, allow_split, have_side), p in sweep.items():
        key = (nbits, g2, allow_split, have_side)
        for b in util.MSM_BUFFERS:
            assert np.all(p["touch_" + b] <= p["size_" + b]), (key, b)
        assert np.all(p["nwin"] <= util.MSM_WINDOWS_MAX) and np.all(p["nsplit"] <= util.MSM_NSPLIT_MAX), key
        assert np.all(p["ngroups"] >= 1) and np.all(p["ngroups"] <= util.MSM_GROUPS_MAX), key
        if not (allow_split and have_side):
            assert np.all(p["ngroups"] == 1), key
        lds = p["lds_sort"] == 1
        assert np.all(p["cbk"][lds] <= util.PIP_SORT_MAX_CBK) and np.all((1 << p["cbk"][lds]) % util.PIP_SORT_THREADS == 0), key
        assert np.all(p["per"] * util.PIP_SLICES >= p["n"]) and np.all(p["point_grid"] * util.WAVE >= p["n"]), key
        assert np.all(p["slice_scan_grid"] * util.WAVE >= p["total"]) and np.all(p["total"] == p["nwin"] << p["cbk"]), key
        assert np.all(p["segs_per_win"] * util.MSM_SEG == 1 << p["cbk"]) and np.all(p["nseg"] == p["nwin"] * p["segs_per_win"]), key
        # the cuts fall strictly from nwin to 0, and the groups are the windows between them
        cut = [p["cut0"], p["cut1"], p["cut2"]]
        assert np.all(cut[0] == p["nwin"]) and np.all(cut[1] < cut[0]) and np.all(cut[2] == 0), key
        two = p["ngroups"] == 2
        assert np.all(cut[1][two] > 0) and np.all(cut[1][~two] == 0), key
        for g in range(2):
            live = p["ngroups"] > g
            G = {f: p["g%d_%s" % (g, f)][live] for f in ("w0", "w1", "g0", "gc", "t0", "tc", "order_grid", "bucket_grid", "team", "segred_grid", "tail_waves", "tail_lanes")}
            cbk, spw = p["cbk"][live], p["segs_per_win"][live]
            assert np.all(G["w0"] == cut[g + 1][live]) and np.all(G["w1"] == cut[g][live]), key
            assert np.all(G["g0"] == G["w0"] << cbk) and np.all(G["gc"] == (G["w1"] - G["w0"]) << cbk), key
            assert np.all(G["t0"] == G["w0"] * spw) and np.all(G["tc"] == (G["w1"] - G["w0"]) * spw), key
            assert np.all(G["bucket_grid"] * util.WAVE >= G["gc"]) and np.all(G["order_grid"] * util.WAVE * util.MSM_ORD_PER >= G["gc"]), key
            assert np.all(np.isin(G["team"], (1, 2, 4))) and np.all(G["segred_grid"] * util.WAVE >= G["tc"] * G["team"]), key
            wide = G["team"] > 1
            assert np.all((G["tc"] * G["team"])[wide] <= util.MSM_TEAM_LANES_MAX) and (not g2 or not wide.any()), key
            assert np.all(G["tail_waves"] >= 1) and np.all(G["tail_waves"] * util.WAVE <= 1024) and np.all(G["tail_lanes"] == G["tail_waves"] * util.WAVE), key


def test_point_sums_cover_the_points_and_fit_the_export_area():
    for S in SLOTS:
        n = np.array(list(range(1, 40 * S + 2)) + [1 << 20, 1 << 30], dtype=np.uint64)
        for g2, words in ((False, util.G1_WORDS), (True, util.G2_WORDS)):
            nblk, m = util.sum_plans(g2, S, n)
            assert np.all(nblk >= 1) and np.all(nblk * util.WAVE * m >= n), (S, g2)
            assert np.all(nblk * words * 4 <= util.SUM_PARTS_BYTES), (S, g2)
            for max_sets in MAX_SETS:
                c = util.ctx_sizes(S, max_sets)
                assert c["export_bytes"] == c["stride"] * 288 + util.SUM_PARTS_BYTES, (S, max_sets)


def test_context_sizes_hold_the_line_products():
    for S, max_sets in itertools.product(SLOTS, MAX_SETS):
        c = util.ctx_sizes(S, max_sets)
        stride, cap = c["stride"], c["nblk_cap"]
        assert stride % util.WAVE == 0 and stride >= max_sets + 1 + util.SIG_SLOTS_MAX and c["mstride"] % util.WAVE == 0 and c["mstride"] >= 2 * max_sets
        assert 1 <= cap <= stride // util.WAVE
        for fold in (False, True):
            p = util.lineprod_plans(S, cap, stride, 1, stride, fold)
            assert np.all(p["nblk"] >= 1) and np.all(p["nblk"] <= cap), (S, max_sets, fold)
            assert np.all(p["nblk"] * util.WAVE * p["m"] >= np.arange(1, stride + 1, dtype=np.uint64)), (S, max_sets, fold)
            # k_lineprod: N_LINES x nblk x 64 values from the start; k_fold's first level: N_LINES x nb1 values from lpart_mid_words on
            assert np.all(util.N_LINES * p["nblk"] * util.WAVE * util.F12_WORDS <= c["lpart_mid_words"]), (S, max_sets, fold)
            assert np.all(c["lpart_mid_words"] + util.N_LINES * p["nb1"] * util.F12_WORDS <= c["lpart_words"]), (S, max_sets, fold)
