#!/usr/bin/env python3
"""Stand-alone benchmark of k G2 MSMs in one device pass (mi355_bls_p2s_mult_pippenger_many_device) and of the Jacobian-to-affine calls
(mi355_bls_p1s_to_affine_device / mi355_bls_p2s_to_affine_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_msm_g2_many.py [--out profiles/msm_g2_many_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: G2 points from 1 024 distinct signatures of one message, repeated; 32 random scalar bytes each; nbits = 255.  Before anything
is timed the new call's results are compared, as points, with the single call's over the same members (a sample: the first four and the last).
Times are host-clock medians of 5 blocking calls after one warm-up call, with min..max beside them.  Rows, each comparison in the same process
on the same context as the new call:
  shared:k / ragged:k   k G2 MSMs of 4 096 points, k in {8, 64, 512}
      many       the new call
      one_each   k consecutive p2s_mult_pippenger_device calls over the same members: the route a caller has without the new call
      floor      ONE single G2 MSM over all k x 4 096 pairs: the same bucket work without the per-MSM tails - a floor, not a rival
  opening:4096          4 096 MSMs of 2 points each (ragged), the shape of [tau - z_g]G2 for 4 096 openings
      one_each   k single calls, MEASURED ON THE FIRST 64 MEMBERS AND SCALED by k / 64 (said so in the row)
  to_affine:g:n         p1s_to_affine_device (g = 1) / p2s_to_affine_device (g = 2) over n images, n in {64, 4 096, 65 536}; the images have Z = 1
      copies     the device-to-host and host-to-device copies of the same bytes (pageable host memory): what a caller pays today before any host
                 arithmetic
  ratio_one_each = one_each / many and ratio_copies = copies / call (above 1: the new call is faster), ratio_floor = many / floor.
A to_affine call at these sizes takes about 0.1 ms: a blocking call that short is mostly launch and synchronise latency, so its row says
whether the call is slower than the copies, not by what factor.  --only STEP,STEP runs some rows; the file then says which, and that it is
partial."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N = 4096
KS = (8, 64, 512)
OPEN_SAMPLE = 64
STEPS = (["shared:%d" % k for k in KS] + ["ragged:%d" % k for k in KS] + ["opening:4096"] +
         ["to_affine:%d:%d" % (g, n) for g in (1, 2) for n in (64, 4096, 65536)])


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


def g2_base(count):
    import c_oracle as co
    r = random.Random(5)
    return [co.sign(r.getrandbits(96) | 1, b"bench g2 many") for _ in range(count)]


def msm_step(form, k):
    import numpy as np
    import torch
    m = load()
    from util import g2_jac_to_affine
    per = 2 if form == "opening" else N
    lengths = [per] * k
    pairs = per * k
    base = g2_base(1024)
    npts = N if form == "shared" else pairs
    pts = b"".join(base[i % 1024] for i in range(min(npts, 1 << 16)))
    d_pts = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    if npts > 1 << 16:
        d_pts = d_pts.repeat(npts // (1 << 16)).contiguous()
    d_all = d_pts if form != "shared" else d_pts.repeat(k).contiguous()             # the floor's points
    d_sc = torch.from_numpy(np.random.default_rng(20261020).integers(0, 256, size=(pairs, 32), dtype=np.uint8)).cuda()
    offs = [per * j for j in range(k + 1)]
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    P, S = d_pts.data_ptr(), d_sc.data_ptr()

    def many():
        return m.p2s_mult_pippenger_many_device(c, P, npts, S, None if form == "shared" else offs, k, 255)

    def member(j):
        return m.p2s_mult_pippenger_device(c, P + (0 if form == "shared" else 192 * offs[j]), per, S + 32 * offs[j], 255)

    sample = k if form != "opening" else OPEN_SAMPLE

    def one_each():
        for j in range(sample):
            member(j)

    got = many()
    for j in list(range(4)) + [k - 1]:
        assert g2_jac_to_affine(got[j]) == g2_jac_to_affine(member(j)), "MSM %d differs from the single call" % j
    row = {"form": form, "k": k, "pairs": pairs, "points_per_msm": per}
    row["many"] = timed(many)
    row["stages_ms"] = {n: round(v, 3) for n, v in zip(("sort_and_order", "bucket_accumulation", "reductions", "tails"), list(c.timings().values())[:4])}
    row["one_each"] = timed(one_each)
    if sample != k:
        row["one_each_measured_on"] = sample
        row["one_each"] = {n: round(v * k / sample, 3) for n, v in row["one_each"].items()}
        row["one_each"]["scaled"] = "measured on the first %d members, times %d / %d" % (sample, k, sample)
    row["floor"] = timed(lambda: m.p2s_mult_pippenger_device(c, d_all.data_ptr(), pairs, S, 255))
    row["ratio_one_each"] = round(row["one_each"]["median_ms"] / row["many"]["median_ms"], 2)
    row["ratio_floor"] = round(row["many"]["median_ms"] / row["floor"]["median_ms"], 2)
    torch.cuda.synchronize()
    return row


def to_affine_step(g, n):
    import torch
    m = load()
    import bls12381_py as o
    import c_oracle as co
    r = random.Random(6)
    one = o.fp_to_mont_bytes(1)
    if g == 1:
        base = [co.sk_to_pk(r.getrandbits(96) | 1) + one for _ in range(256)]
        call, jacb = m.p1s_to_affine_device, 144
    else:
        base = [s + one + bytes(48) for s in g2_base(256)]
        call, jacb = m.p2s_to_affine_device, 288
    d_in = torch.frombuffer(bytearray(b"".join(base[i % 256] for i in range(min(n, 256)))), dtype=torch.uint8).cuda()
    if n > 256:
        d_in = d_in.repeat(n // 256).contiguous()
    affb = jacb // 3 * 2
    d_out = torch.empty((n * affb,), dtype=torch.uint8, device="cuda")
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    call(c, d_in.data_ptr(), n, d_out.data_ptr())
    got = bytes(d_out[:affb * min(n, 256)].cpu().numpy())
    assert got == b"".join(b[:affb] for b in base[:min(n, 256)]), "to_affine of Z = 1 images is not the identity on x, y"

    def copies():
        host = d_in.cpu()                                                             # n Jacobian images out ...
        back = host[:n * affb].cuda()                                                 # ... and n affine images back in
        torch.cuda.synchronize()
        return back

    row = {"form": "to_affine", "group": g, "n": n, "bytes_in": n * jacb, "bytes_out": n * affb}
    row["call"] = timed(lambda: call(c, d_in.data_ptr(), n, d_out.data_ptr()))
    row["copies"] = timed(copies)
    row["ratio_copies"] = round(row["copies"]["median_ms"] / row["call"]["median_ms"], 2)
    return row


def step(name):
    parts = name.split(":")
    if parts[0] == "to_affine":
        return to_affine_step(int(parts[1]), int(parts[2]))
    return msm_step(parts[0], int(parts[1]))


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_msm_g2_many: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    msm = [r for r in rows if r["form"] != "to_affine"]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up, min..max beside it; many = "
                   "p2s_mult_pippenger_many_device, one_each = k consecutive p2s_mult_pippenger_device calls over the same members (opening: "
                   "measured on 64 members and scaled), floor = one p2s_mult_pippenger_device call over all pairs; call = p1s / p2s_to_affine_device, "
                   "copies = device-to-host + host-to-device copies of the same bytes; ratio_one_each = one_each / many, ratio_floor = many / floor, "
                   "ratio_copies = copies / call; stages_ms = the event times of the first pass of the last timed `many` call",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "many_faster_than_one_each_in_every_row": all(r["ratio_one_each"] > 1 for r in msm),
            "to_affine_faster_than_the_copies_in_every_row": all(r["ratio_copies"] > 1 for r in rows if r["form"] == "to_affine")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_g2_many_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--only", default=None, help="comma-separated steps instead of all of them")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    steps = a.only.split(",") if a.only else list(STEPS)
    rows = [child(s, 240) for s in steps]
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_msm_g2_many: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
