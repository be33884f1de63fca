"""The Python mirror of the latency-mode plan (tests/util.py latency_plan) against the constants and bounds of csrc/host_api.inc it restates:
a threshold moved in the product without the mirror (and the sizes of tests/golden/latency_handover.json) fails here, instead of leaving
tests/test_gpu_latency_handover.py to pass away from the boundaries it is meant to sit on."""
import os
import re

import util
from util import golden, latency_hand_overs, latency_plan

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nim-blscurve_amd", "csrc", "host_api.inc")


def _src():
    with open(SRC) as f:
        return f.read()


def _function(src, head):
    """the body of the static function whose signature starts with `head`, up to its closing brace at column 0"""
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


def _norm(s):
    return re.sub(r"\s+", " ", s)


def test_constants_match_the_product():
    src = _src()
    m = re.search(r"constexpr uint32_t TEAM_CLEAR_ITEMS_PER_SLOT = (\d+), TEAM_LINES_ITEMS_PER_SLOT = (\d+);", src)
    assert m, "TEAM_*_ITEMS_PER_SLOT not found in host_api.inc"
    assert int(m.group(1)) == util.TEAM_CLEAR_ITEMS_PER_SLOT
    assert int(m.group(2)) == util.TEAM_LINES_ITEMS_PER_SLOT
    m = re.search(r"constexpr size_t SIG_WIDE_MIN = (\d+);", src)
    assert m and int(m.group(1)) == util.SIG_WIDE_MIN
    assert "return c->slots * TEAM_CLEAR_ITEMS_PER_SLOT;" in src and "return c->slots * TEAM_LINES_ITEMS_PER_SLOT;" in src


def test_bounds_match_the_product():
    src = _src()
    # run_pairs: the two fork streams up to 16 S sets, the signature side's stream alone beyond
    m = re.search(r"const bool fork = have_side && n32 <= (\d+) \* c->slots;", src)
    assert m and int(m.group(1)) == util.FORK_ITEMS_PER_SLOT
    assert "const bool fork_sig = !fork && have_side;" in src
    assert "uint32_t cw = n >= SIG_WIDE_MIN ? 8 : 4, nwin = 64 / cw, total = nwin << cw;" in src
    # team_form_for: rows, rows2, spread, wide
    tf = _norm(_function(src, "static team_form team_form_for("))
    assert "const uint32_t rows_max = (c->slots - c->slots / 8) / 4;" in tf
    assert "if (count <= rows_max) return TEAM_ROWS;" in tf
    assert "if (count <= 2 * rows_max) return TEAM_ROWS2;" in tf
    assert "return (count + 3) / 4 <= c->slots ? TEAM_SPREAD : TEAM_WIDE;" in tf
    # launch_hash_map: a pair per row, one wave per SIMD, the plain grid
    hm = _norm(_function(src, "static void launch_hash_map("))
    assert "const uint32_t waves = (2 * n32 + WAVE - 1) / WAVE;" in hm
    assert "if (c->coop && (2 * n32 + 3) / 4 <= c->slots - c->slots / 8) k_hash_map_rows<<<" in hm
    assert "else if (c->coop && waves <= c->slots) k_hash_map_spread<<<" in hm
    assert "else k_hash_map<<<" in hm
    # launch_hash_clear / launch_lines: the engine up to 11 S messages / 18 S pairs
    assert "if (c->coop && n32 <= team_clear_max(c)) launch_team_clear(c, n32, st);" in _norm(_function(src, "static void launch_hash_clear("))
    assert "if (c->coop && npairs <= team_lines_max(c)) {" in _norm(_function(src, "static void launch_lines("))


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
