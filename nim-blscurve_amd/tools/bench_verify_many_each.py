#!/usr/bin/env python3
"""Stand-alone benchmark of the per-batch verdicts for many batches (mi355_bls_batch_verify_many_each_device / _locate_device); bench.py stays
the flagship's.

  python nim-blscurve_amd/tools/bench_verify_many_each.py [--out profiles/verify_many_each_bench.json]

Every GPU step (one per shape) runs in a child process of its own under `timeout`; the first step that fails ends the run.
Inputs: k x n = 65 536 sets with distinct keys and messages from the device signer, device-resident, on a 65 536-set context; the forged
input has one flipped message bit in batch k / 2.  Before anything is timed every call must give the right verdicts on both inputs.  Times
are host-clock medians of 5 blocking calls after one warm-up call; min and max of the same calls are the run-to-run spread.  Per shape:
  many_each   on the valid and on the forged input (its time should not depend on which);
  many_locate on both: the merged pass alone, and the merged pass plus one per-batch pass;
  mi355_bls_batch_verify_many_device on both, in the same run: its passing merged pass and its failing k-call fallback - the yardsticks.
Ratios: failing case = fallback / new call (above 1: the new call wins), passing case = new call / merged pass (what asking "which one?"
up front costs).  Nothing in the library switches on these numbers.  The item width (plan.hpp AGGV_C), the G2 multiplication chunk
(COMB_MUL_CHUNK) and the tail hand-over are the committed ones; no other value was tried, so there is no A/B row."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = ((16, 4096), (64, 1024), (256, 256), (1024, 64))
CAP = 65536


def load():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def ms_per_call(fn, reps=5):
    """-> {"median", "min", "max"} in ms of `reps` calls after one warm-up"""
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step(k, n):
    import numpy as np
    import torch
    m = load()
    total = k * n
    c = m.BatchedBLSVerifierCache.init(max_sets=CAP)
    rng = np.random.default_rng(20261019)
    sks = rng.integers(1, 255, size=(total, 32), dtype=np.uint8)
    sks[:, 31] = 0                                                           # below the group order
    msgs = b"".join(hashlib.sha256(b"bench verify_many_each %d" % i).digest() for i in range(total))
    ok, rec, _ = m.signSets(c, sks.tobytes(), msgs)
    assert ok
    valid = torch.from_numpy(np.frombuffer(rec, dtype=np.uint8).copy()).cuda()
    forged = valid.clone()
    bad_b = k // 2
    forged[320 * (bad_b * n + n // 2) + 96] ^= 1                             # one flipped message bit: batch k / 2 alone fails
    counts = [n] * k
    rnds = [hashlib.sha256(b"bench verify_many_each rnd %d" % b).digest() for b in range(k)]
    all_true, one_false = [True] * k, [b != bad_b for b in range(k)]
    calls = {"many_each": m.batchVerifyManyEach_device, "many_locate": m.batchVerifyManyLocate_device, "batch_verify_many": m.batchVerifyMany_device}
    row = {"k": k, "n": n, "sets": total}
    for name, fn in calls.items():
        assert fn(c, valid.data_ptr(), counts, rnds) == all_true, name
        assert fn(c, forged.data_ptr(), counts, rnds) == one_false, name
        row[name + "_valid_ms"] = ms_per_call(lambda: fn(c, valid.data_ptr(), counts, rnds))
        row[name + "_forged_ms"] = ms_per_call(lambda: fn(c, forged.data_ptr(), counts, rnds))
    fallback, merged = row["batch_verify_many_forged_ms"], row["batch_verify_many_valid_ms"]
    for name in ("many_each", "many_locate"):
        f, v = row[name + "_forged_ms"], row[name + "_valid_ms"]
        row[name + "_failing_fallback_over_new"] = round(fallback["median"] / f["median"], 2)
        row[name + "_passing_new_over_merged"] = round(v["median"] / merged["median"], 2)
        row[name + "_loses_failing_case"] = f["median"] >= fallback["median"]
    c.close()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_verify_many_each: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_many_each_bench.json"))
    ap.add_argument("--step", default=None, help="k x n, e.g. 256x256: run this shape in this process")
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES), help="the shapes to run, comma separated")
    a = ap.parse_args()
    if a.step:
        k, n = (int(x) for x in a.step.split("x"))
        print(json.dumps(step(k, n)))
        return
    rows = [child(s, 240) for s in a.shapes.split(",")]
    res = {"how": "ms per blocking call on device-resident records, host clock: median, min and max of 5 calls after a warm-up (min .. max is the "
                  "run-to-run spread), one 65 536-set context with the default numThreads; forged = one flipped message bit in batch k / 2; "
                  "*_failing_fallback_over_new = batch_verify_many_device's k-call fallback on the forged input over the new call on it (above 1: the "
                  "new call wins), *_passing_new_over_merged = the new call on the valid input over batch_verify_many_device's merged pass; "
                  "item width AGGV_C = 8, COMB_MUL_CHUNK = 65 536 and the per-group path's tail hand-over, no other values tried",
           "rows": rows,
           "many_each_loses_failing_case_at": ["%dx%d" % (r["k"], r["n"]) for r in rows if r["many_each_loses_failing_case"]],
           "many_locate_loses_failing_case_at": ["%dx%d" % (r["k"], r["n"]) for r in rows if r["many_locate_loses_failing_case"]]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
