#!/usr/bin/env python3
"""Stand-alone benchmark of the fixed-base table MSM (mi355_bls_p1s_table_create_device, mi355_bls_p1s_mult_table(_many)_device); bench.py
stays the flagship's.

  python nim-blscurve_amd/tools/bench_msm_table.py [--out profiles/msm_table_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: points from a few thousand distinct public keys, repeated; 32 random scalar bytes each; nbits = 255.  Before anything is
timed the table call's results are compared, as points, with the generic call's on the same arrays.  Times are host-clock medians of 5
blocking calls after one warm-up call, with min..max beside them.  Rows:
  single:n   one MSM over n points, n in {4 096, 2^16, 2^20}: mult_table_device against p1s_mult_pippenger_device
  many:k     k MSMs over the same 4 096 points, k in {8, 64, 512}: mult_table_many_device against p1s_mult_pippenger_many_device (shared form)
and per row, in the same process on the same context, the table call at wbits = 8, 12, 16 and at the rule's own choice (wbits = 0), each with
  create        table_create_device, and the table's bytes
  table         the table call; stages_ms: sort, buckets, reductions, sum (the event times of the last timed call's first pass); plan: (W, S,
                buckets per set)
  ratio         generic / table (above 1: the table call is faster)
  uses_to_pay   create / (generic - table): the table uses after which create has paid for itself (null where the table call is not faster)
The yardstick is `generic`, the generic call measured in the same run - never an earlier figure."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N_MANY = 4096
WBITS = (8, 12, 16, 0)
STEPS = ["single:%d" % n for n in (4096, 1 << 16, 1 << 20)] + ["many:%d" % k for k in (8, 64, 512)]


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
    import random

    import numpy as np
    import torch
    m = load()
    import c_oracle as co
    from util import g1_jac_to_affine
    form, v = name.split(":")
    n, k = (int(v), 1) if form == "single" else (N_MANY, int(v))
    r = random.Random(5)
    base = b"".join(co.sk_to_pk(r.getrandbits(96) | 1) for _ in range(4096))
    d_pts = torch.frombuffer(bytearray(base), dtype=torch.uint8).cuda().repeat(n // 4096 + 1)[:96 * n].contiguous()
    d_sc = torch.from_numpy(np.random.default_rng(20261020).integers(0, 256, size=(k * n, 32), dtype=np.uint8)).cuda()
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    P, S = d_pts.data_ptr(), d_sc.data_ptr()

    def generic():
        if form == "single":
            return [m.p1s_mult_pippenger_device(c, P, n, S, 255)]
        return m.p1s_mult_pippenger_many_device(c, P, n, S, None, k, 255)

    want = [g1_jac_to_affine(b) for b in generic()]
    row = {"form": form, "n": n, "k": k, "generic": timed(generic), "tables": []}
    for wbits in WBITS:
        made = []

        def create():
            if made:
                made.pop().destroy()
            made.append(m.p1s_table_create_device(c, P, n, wbits, 255))

        t = {"wbits": wbits, "create": timed(create), "table_bytes": m.p1s_table_sizeof(n, wbits, 255)}
        tab = made[0]

        def table():
            if form == "single":
                return [m.p1s_mult_table_device(c, tab, S, 255)]
            return m.p1s_mult_table_many_device(c, tab, S, k, 255)

        assert [g1_jac_to_affine(b) for b in table()] == want, "the table call differs from the generic call at wbits %d" % wbits
        t["table"] = timed(table)
        t["stages_ms"] = {s: round(x, 3) for s, x in zip(("sort", "buckets", "reductions", "sum"), list(c.timings().values())[:4])}
        t["plan"] = list(m.debug_p1s_table_last_plan(c))
        t["ratio"] = round(row["generic"]["median_ms"] / t["table"]["median_ms"], 2)
        gain = row["generic"]["median_ms"] - t["table"]["median_ms"]
        t["uses_to_pay"] = round(t["create"]["median_ms"] / gain, 1) if gain > 0 else None
        row["tables"].append(t)
        tab.destroy()
    torch.cuda.synchronize()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_msm_table: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows):
    rule = lambda r: next(t for t in r["tables"] if t["wbits"] == 0)
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up, min..max beside it; generic = "
                   "p1s_mult_pippenger_device (single) or p1s_mult_pippenger_many_device in the shared form (many) in the same run; ratio = generic / "
                   "table; stages_ms = the event times of the first pass of the last timed table call; uses_to_pay = create / (generic - table)",
            "rows": rows,
            "rule_faster_than_generic": {"%s:%d" % (r["form"], r["n"] if r["form"] == "single" else r["k"]): rule(r)["ratio"] > 1 for r in rows}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_table_bench.json"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    rows = [child(s, 240) for s in STEPS]
    res = summary(rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
