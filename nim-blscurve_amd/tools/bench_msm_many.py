#!/usr/bin/env python3
"""Stand-alone benchmark of k G1 MSMs in one device pass (mi355_bls_p1s_mult_pippenger_many_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_msm_many.py [--out profiles/msm_many_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: points from a few thousand distinct public keys, repeated; 32 random scalar bytes each; nbits = 255.  Before anything is
timed the new call's results are compared, as points, with the single call's over the same members (a sample: the first eight and the last).
Times are host-clock medians of 5 blocking calls after one warm-up call, with min..max beside them.  Rows:
  shared  k MSMs over the same 4 096 points, k in {1, 8, 64, 512}
  ragged  k MSMs of 4 096 points each over distinct point ranges, the same k
  mixed   ragged k = 64 with member lengths 256 .. 16 384
and per row, in the same process on the same context:
  many       the new call
  one_each   k consecutive p1s_mult_pippenger_device calls over the same members: the route a caller has without the new call
  floor      ONE single-MSM call over all k n pairs (shared: the points repeated k times): the same bucket work without the per-MSM tails - a
             floor, not a rival
  ratio_one_each = one_each / many (above 1: the new call is faster), ratio_floor = many / floor."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N = 4096
KS = (1, 8, 64, 512)
MIXED = [256 << (j % 7) for j in range(64)]          # 256 .. 16 384
STEPS = ["shared:%d" % k for k in KS] + ["ragged:%d" % k for k in KS] + ["mixed:64"]


def load():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import __graft_entry__ as ge
    return ge.load_package()


def timed(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def step(name):
    import numpy as np
    import torch
    m = load()
    import bls12381_py as o
    import c_oracle as co
    from util import g1_jac_to_affine
    form, k = name.split(":")
    k = int(k)
    lengths = MIXED if form == "mixed" else [N] * k
    pairs = sum(lengths)
    rng = np.random.default_rng(20261019)
    import random
    r = random.Random(5)
    base = [co.sk_to_pk(r.getrandbits(96) | 1) for _ in range(4096)]
    npts = N if form == "shared" else pairs
    pts = b"".join(base[i % 4096] for i in range(npts))
    d_pts = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    d_all = d_pts if form != "shared" else torch.frombuffer(bytearray(pts * k), dtype=torch.uint8).cuda()      # the floor's points
    d_sc = torch.from_numpy(rng.integers(0, 256, size=(pairs, 32), dtype=np.uint8)).cuda()
    offs = [0]
    for v in lengths:
        offs.append(offs[-1] + v)
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    P, S = d_pts.data_ptr(), d_sc.data_ptr()

    def many():
        return m.p1s_mult_pippenger_many_device(c, P, npts, S, None if form == "shared" else offs, k, 255)

    def member(j):
        return m.p1s_mult_pippenger_device(c, P + (0 if form == "shared" else 96 * offs[j]), lengths[j], S + 32 * offs[j], 255)

    def one_each():
        for j in range(k):
            member(j)

    got = many()
    for j in list(range(min(8, k))) + [k - 1]:
        assert g1_jac_to_affine(got[j]) == g1_jac_to_affine(member(j)), "MSM %d differs from the single call" % j
    row = {"form": form, "k": k, "pairs": pairs, "lengths": "4096 each" if form != "mixed" else "256 << (j % 7), j < 64"}
    row["many"] = timed(many)
    row["stages_ms"] = None if k == 1 else {                                         # k == 1 takes the single path: no pass of the new kind
        n: round(v, 3) for n, v in zip(("sort_and_order", "bucket_accumulation", "reductions", "tails"), list(c.timings().values())[:4])}
    row["one_each"] = timed(one_each)
    row["floor"] = timed(lambda: m.p1s_mult_pippenger_device(c, d_all.data_ptr(), pairs, S, 255))
    row["ratio_one_each"] = round(row["one_each"]["median_ms"] / row["many"]["median_ms"], 2)
    row["ratio_floor"] = round(row["many"]["median_ms"] / row["floor"]["median_ms"], 2)
    torch.cuda.synchronize()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_msm_many: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows):
    k1 = [r for r in rows if r["k"] == 1]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up, min..max beside it; many = "
                   "p1s_mult_pippenger_many_device, one_each = k consecutive p1s_mult_pippenger_device calls over the same members, floor = one "
                   "p1s_mult_pippenger_device call over all pairs; ratio_one_each = one_each / many, ratio_floor = many / floor; stages_ms = the "
                   "event times of the first pass of the last timed `many` call",
            "rows": rows,
            "faster_than_one_each_at_every_k_from_8": all(r["ratio_one_each"] > 1 for r in rows if r["k"] >= 8),
            # k = 1 takes the single path: its median inside the single call's min..max of the same run, and the weaker "not above its max"
            "k1_within_spread_of_single": all(r["one_each"]["min_ms"] <= r["many"]["median_ms"] <= r["one_each"]["max_ms"] for r in k1),
            "k1_not_above_single_max": all(r["many"]["median_ms"] <= r["one_each"]["max_ms"] for r in k1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_many_bench.json"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    rows = [child(s, 120) for s in STEPS]
    res = summary(rows)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
