"""The launch plan of k MSMs in one pass with its G2 flag (csrc/plan.hpp msm_many_for(..., g2) and what follows from it, asked through
tests/host_emu/plan_msmmany_g2.cpp): every pass's extents fit msm_many_sizes_for, no pass exceeds the G2 bounds, the passes tile [0, k), and with
the flag off the plan is the G1 call's, word for word.  The plan of the Jacobian-to-affine calls (to_affine_for / to_affine_next) beside it.
The same sweep runs as a program of its own under AddressSanitizer and UBSan (nothing loaded into python is sanitized)."""
import os
import subprocess

import pytest

import g2many_helpers as h
from test_msm_many_plan import call_plan as g1_call_plan

RAGGED = [0, 1, 2, 31, 32, 33, 0, 100, 1]
SHARED = [(3, 5), (5, 33), (64, 256), (8, 4096), (64, 4096), (512, 4096), (4096, 2)]


def check_call(k, nbits, n=None, lengths=None):
    C = h.constants()
    head, passes = h.call_plan(k, nbits, n, lengths, g2=True)
    lens = lengths if lengths is not None else [n] * k
    nwin, cbk = head["nwin"], head["cbk"]
    assert 1 <= nwin <= C["MSM_WINDOWS_MAX"] == 64 and head["buckets_per_msm"] == nwin << cbk
    assert 1 <= head["tail_waves"] <= min(nwin, C["G2_TAIL_WAVES"]) and head["tail_lanes"] == head["tail_waves"] * C["WAVE"]
    assert head["msms_max"] >= 1 and head["msms_max"] * head["buckets_per_msm"] <= C["G2_BUCKETS_MAX"] == C["BUCKETS_MAX"] // 2
    at = 0
    for p in passes:
        assert p["j0"] == at and p["j1"] > p["j0"]                                    # the passes tile [0, k): no gap, no overlap
        at = p["j1"]
        if p["single"]:
            assert p["j1"] - p["j0"] == 1 and (len(lens) == 1 or lens[p["j0"]] > C["PAIRS_MAX"])
            assert all(p[b] == 0 for b in h.BUFFERS)
            continue
        kp = p["j1"] - p["j0"]
        assert p["pairs"] == sum(lens[p["j0"]:p["j1"]]) <= C["PAIRS_MAX"]
        assert kp <= head["msms_max"] and p["nv"] == kp * nwin <= C["VWIN_MAX"]
        assert p["total"] == kp * head["buckets_per_msm"] <= C["G2_BUCKETS_MAX"]      # the halved bucket bound
        assert p["team"] == 1 and p["segred_grid"] * C["WAVE"] >= p["nseg"]           # k_pip_segred<fp2> alone
        for b in h.BUFFERS:
            assert p[b] <= head["size_" + b], (b, p)                                  # every extent fits what the call reserves
        if p["pairs"]:
            # G2 points: 6 coordinates of 16 words in the SoA stores, 4 in the converted points
            assert p["buckets"] == p["total"] * C["G2_WORDS"] * 4 and p["segout"] == p["nseg"] * C["G2_WORDS"] * 4
            assert p["part"] == p["nv"] * head["nsplit"] * C["G2_WORDS"] * 4 and p["pts_int"] == p["points"] * (C["G2_WORDS"] // 3 * 2) * 4
            assert p["buckets"] <= C["BUCKETS_MAX"] * C["G1_WORDS"] * 4               # ... and the bucket store did not grow
    assert at == len(lens)
    return head, passes


@pytest.mark.parametrize("nbits", [5, 64, 255, 256])
def test_the_shapes_of_the_gpu_tests(nbits):
    check_call(len(RAGGED), nbits, lengths=RAGGED)
    for k, n in SHARED:
        check_call(k, nbits, n=n)
    check_call(1, nbits, n=33)
    check_call(1, nbits, lengths=[1])


def test_sweep():
    for nbits in (1, 5, 64, 255, 256):
        for n in (1, 2, 33, 4096, 65536, 1 << 20, (1 << 20) + 1):
            for k in (1, 2, 5, 64, 1500, 70000):
                if (n > 65536 and k > 5) or (n >= 4096 and k > 1500):
                    continue
                check_call(k, nbits, n=n)
                check_call(k, nbits, lengths=[(n, 0, 1)[j % 3] for j in range(k)])


def test_every_part_count_is_reachable():
    """nsplit = 1, 4 and 16 partial sums per window, by the member length: what tests/test_gpu_msm_many_g2.py runs on the device"""
    met = {n: check_call(2, 255, n=n)[0]["nsplit"] for n in (256, 4096, 1 << 15, 1 << 18)}
    assert met == {256: 1, 4096: 1, 1 << 15: 4, 1 << 18: 16}


def test_a_call_cut_into_two_passes_by_the_halved_bucket_bound():
    """what tests/test_gpu_msm_many_g2.py runs: k single-point MSMs at nbits = 64, k one above a pass's MSMs"""
    head, _ = h.call_plan(2, 64, lengths=[1, 1])
    k = head["msms_max"] + 1
    _, passes = check_call(k, 64, lengths=[1] * k)
    assert [(p["single"], p["j1"] - p["j0"]) for p in passes] == [(0, k - 1), (0, 1)]
    g1_head, _ = h.call_plan(2, 64, lengths=[1, 1], g2=False)
    assert head["msms_max"] <= g1_head["msms_max"]


def test_with_the_flag_off_the_plan_is_the_g1_plan():
    for nbits in (1, 64, 255, 256):
        for k, n in SHARED + [(70000, 1), (3, (1 << 20) + 1)]:
            assert h.call_plan(k, nbits, n=n, g2=False) == g1_call_plan(k, nbits, n=n)
        for lengths in (RAGGED, [1] * 5000, [100, 33, (1 << 20) + 1, 0, 100]):
            assert h.call_plan(0, nbits, lengths=lengths, g2=False) == g1_call_plan(0, nbits, lengths=lengths)


def test_to_affine_plan():
    C = h.to_affine_constants()
    assert C["RUN_MAX"] == 8
    for n in (1, 7, 63, 64, 65, 1000, 4096, C["DEVICE_LANES"], C["DEVICE_LANES"] + 1, 3 * C["DEVICE_LANES"], 1 << 20, C["CHUNK_POINTS"] + 5):
        for force in (0, 1, 2, 8, 100):
            run, chunk, launches = h.to_affine_plan(n, force)
            want = force if force else -(-n // C["DEVICE_LANES"])                     # one point per lane while lanes are idle, then more
            assert run == max(1, min(want, C["RUN_MAX"])) and chunk == C["CHUNK_POINTS"]
            at = 0
            for first, cnt, lanes, grid in launches:
                assert first == at and 1 <= cnt <= chunk and lanes == -(-cnt // run) and grid == -(-lanes // 64)
                at += cnt
            assert at == n
    assert h.to_affine_plan(0)[2] == []


def test_the_sweep_under_the_sanitizers():
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call([os.path.join(here, "host_emu", "build_msmmany_g2.sh"), "san"])
    out = subprocess.run([os.path.join(here, "host_emu", "_build", "plan_msmmany_g2_san")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.returncode, out.stdout, out.stderr[-2000:])
