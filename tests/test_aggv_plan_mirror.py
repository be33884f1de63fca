"""aggregateVerify's slicing as the product's own code decides it (csrc/plan.hpp aggv_cut / aggv_all32, through tests/util.py aggv_slice_plan), pinned
by literal plans, and the plans tests/test_gpu_aggv_varlen.py relies on: a bound moved in the product fails here, instead of leaving the GPU test to
pass without the byte-budget cut or without slices on both hashing paths.  Also the rule of tests/util.py varlen_case and its fixture."""
import hashlib
import os
import re

from util import (VARLEN_CASES, VARLEN_LONG, VARLEN_PAD_EDGES, VARLEN_PREFIXES, VARLEN_REQUIRED, VARLEN_RUN32, aggv_one_slice_cap, aggv_slice_plan,
                  golden, varlen_case, varlen_defect, varlen_lengths)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_message_limit():
    """what the header promises is what the compiled cut does: a lone message of cap * 320 - 104 bytes fits, one byte more is refused"""
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "blscurve_mi355x.h")).read().replace("\n * ", " "))
    assert "A single message must fit the context's staging buffer (max_sets * 320 - 104 bytes), else MI355_BLS_ERR_CAPACITY." in hdr
    for cap in (1, 2, 64, 1000, 65536):
        limit = cap * 320 - 104
        assert aggv_slice_plan([limit], cap) == [(0, 1, "end", False)] and aggv_slice_plan([limit + 1], cap) is None
        assert aggv_slice_plan([0, limit, 0], cap) == [(0, 1, "bytes" if cap > 1 else "pairs", False), (1, 2, "bytes" if cap > 1 else "pairs", False), (2, 3, "end", False)]
        assert aggv_one_slice_cap([limit]) == cap and aggv_one_slice_cap([limit + 1]) == cap + 1


def test_restated_cut():
    # pair cap alone; the byte budget alone; the exact edge of the budget (the product breaks on bytes + add > budget, not >=)
    assert aggv_slice_plan([32] * 130, 64) == [(0, 64, "pairs", True), (64, 128, "pairs", True), (128, 130, "end", True)]
    assert aggv_slice_plan([64 * 320 - 104], 64) == [(0, 1, "end", False)]
    assert aggv_slice_plan([64 * 320 - 103], 64) is None
    assert aggv_slice_plan([5, 64 * 320 - 103, 5], 64) is None
    # two pairs filling the budget to the byte, and one byte more
    assert aggv_slice_plan([538, 538], 4) == [(0, 2, "end", False)]          # 4 + 638 + 638 = 1 280 = budget
    assert aggv_slice_plan([538, 539], 4) == [(0, 1, "bytes", False), (1, 2, "end", False)]
    assert aggv_one_slice_cap([538, 538]) == 4 and aggv_one_slice_cap([538, 539]) == 5
    assert aggv_one_slice_cap([0] * 10) == 10


def test_lengths_rule():
    for name in VARLEN_CASES:
        L = varlen_lengths(name)                                 # asserts residues, required lengths and the lane layout itself
        assert len(L) == max(VARLEN_PREFIXES[name])
        if len(L) >= 74:                                         # room for every required length beside every residue
            assert set(VARLEN_REQUIRED) <= set(L) and {x % 64 for x in L} == set(range(64))
    assert varlen_lengths("one") == [17]
    W = varlen_lengths("wave")
    assert sorted(x % 64 for x in W[:64]) == list(range(64)) and W[64] == 4096 and W[63] > 0
    assert {8, 9, 16, 17, 0, 1, 31, 32, 33, 1000, 4095} <= set(W[:64])
    assert sorted(VARLEN_PAD_EDGES) == [8, 9, 16, 17, 72, 73, 80, 81, 136, 137, 144, 145]
    # the padding edges under the 43-byte DST: the first hash of expand_message_xmd absorbs len + 111 bytes.  Residue 8: 0x80 and the bit count
    # end block 2 exactly; 9: the bit count no longer fits, a third block; 16: 0x80 is the last byte of block 2; 17: 0x80 opens block 3
    for r, blocks in ((8, 2), (9, 3), (16, 3), (17, 3)):
        assert (r + 111 + 1 + 8 + 63) // 64 == blocks
    assert (8 + 111 + 1 + 8) % 64 == 0 and (16 + 111 + 1) % 64 == 0 and (17 + 111) % 64 == 0
    M = varlen_lengths("mixed")
    a, b = VARLEN_RUN32
    assert b - a >= 256 and set(M[a:b]) == {32} and M[a - 1] != 32 and M[b] != 32 and M.count(32) > b - a
    assert varlen_lengths("long").count(VARLEN_LONG) == 8


def test_plans_the_gpu_test_relies_on():
    M, Wd, Lg = varlen_lengths("mixed"), varlen_lengths("wide"), varlen_lengths("long")
    p = aggv_slice_plan(M, 64)
    assert sum(x[3] for x in p) >= 3 and any(not x[3] for x in p) and {x[2] for x in p} == {"pairs", "bytes", "end"}
    assert [x[2] for x in aggv_slice_plan(M, 1000)] == ["bytes", "end"]
    assert {x[2] for x in aggv_slice_plan(Wd, 64)} == {"bytes", "end"} and len(aggv_slice_plan(Wd, 64)) > 64
    assert [x[2] for x in aggv_slice_plan(Wd, 1000)] == ["bytes"] * 6 + ["end"]
    p = aggv_slice_plan(Lg, 256)
    assert [x[2] for x in p] == ["bytes", "bytes", "end"] and all(b - a < 256 for a, b, _, _ in p)
    for name in VARLEN_CASES:
        for n in VARLEN_PREFIXES[name]:
            L = varlen_lengths(name)[:n]
            assert len(aggv_slice_plan(L, aggv_one_slice_cap(L))) == 1


def test_fixture_matches_the_rule():
    """keys are checked on the device side (the signer rebuilds them); lengths, messages and defects here"""
    fx = golden("aggv_varlen")
    assert [(c["name"], c["n"]) for c in fx["cases"]] == [(name, n) for name in VARLEN_CASES for n in VARLEN_PREFIXES[name]]
    for c in fx["cases"]:
        _, msgs = varlen_case(c["name"])
        msgs = msgs[:c["n"]]
        assert hashlib.sha256(b"".join(len(x).to_bytes(4, "little") for x in msgs)).hexdigest() == c["lengths_sha256"]
        h = hashlib.sha256()
        for x in msgs:
            h.update(len(x).to_bytes(4, "little"))
            h.update(x)
        assert h.hexdigest() == c["msgs_sha256"]
        assert c["valid"]["verdict"] is True and len(c["valid"]["gt"]) == 1152 and len(c["aggsig"]) == 384
        assert len(c["defects"]) >= 1
        for d in c["defects"]:
            bad = varlen_defect(msgs, d)
            assert bad != msgs and len(bad) == len(msgs)
            assert d["verdict"] is False and d["gt"] is not None and d["gt"] != c["valid"]["gt"]
            if d["kind"] == "shift":                             # same bytes, one interior offset moved by one
                assert b"".join(bad) == b"".join(msgs)
                assert [len(x) - len(y) for x, y in zip(bad, msgs) if len(x) != len(y)] == [1, -1]
