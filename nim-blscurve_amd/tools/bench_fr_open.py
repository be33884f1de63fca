#!/usr/bin/env python3
"""Stand-alone benchmark of the openings over Fr (mi355_bls_fr_open_many_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_fr_open.py [--out profiles/fr_open_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: k x n random images below 2^254, k random points; the evaluation form's domain is the n-th roots of unity in natural order.
Before anything is timed the first and the last polynomial's value and quotient are compared with Python integers mod r.  Times are
host-clock medians of 5 blocking calls after one warm-up call, with min..max beside them.  Rows (form:k:n), each comparison in the same
process on the same context:
  coef:1:4096 coef:64:4096 coef:512:4096 coef:64:256 coef:64:65536 and the same five for eval
      fr_open      the new call, values and quotients
      msm_table    p1s_mult_table_many_device over the same (k, n) - the MSM this call feeds (a table of n points, 1 024 distinct keys repeated)
      copy_h2d     ONE hipMemcpy host-to-device of k x n x 32 bytes from pageable memory - the copy the host route cannot avoid
  ratio_copy = copy_h2d / fr_open (above 1: the call costs less than the copy alone, the host route's floor with its field arithmetic
  counted as free), share_of_msm = fr_open / msm_table.  --only STEP,STEP runs some rows; the file then says which, and that it is partial."""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ["%s:%d:%d" % (f, k, n) for f in ("coef", "eval") for k, n in ((1, 4096), (64, 4096), (512, 4096), (64, 256), (64, 65536))]


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
    form, k, n = name.split(":")
    ev, k, n = form == "eval", int(k), int(n)
    m = load()
    import c_oracle as co
    import fropen_cases as fc
    rng = np.random.default_rng(20261020)
    polys_h = rng.integers(0, 256, size=(k * n, 32), dtype=np.uint8)
    polys_h[:, 31] &= 0x3f
    zs_h = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    zs_h[:, 31] &= 0x3f
    d_polys, d_zs = torch.from_numpy(polys_h).cuda(), torch.from_numpy(zs_h).cuda()
    xs = fc.domain(n) if ev else None
    d_dom = torch.frombuffer(bytearray(fc.pack([xs])), dtype=torch.uint8).cuda() if ev else None
    d_ys = torch.empty((k * 32,), dtype=torch.uint8, device="cuda")
    d_quot = torch.empty((k * n * 32,), dtype=torch.uint8, device="cuda")
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    flags = m.FR_OPEN_EVAL if ev else 0

    def fr_open():
        return m.frOpenMany_device(c, d_polys.data_ptr(), n, d_zs.data_ptr(), k, flags, d_dom.data_ptr() if ev else None, d_ys.data_ptr(), d_quot.data_ptr())

    assert fr_open()[0] == 0
    torch.cuda.synchronize()
    ys, quot = bytes(d_ys.cpu().numpy()), d_quot.cpu().numpy()
    for g in sorted({0, k - 1}):
        poly = fc.images(polys_h[g * n:(g + 1) * n].tobytes())
        want = fc.expected([poly], [int.from_bytes(zs_h[g].tobytes(), "little")], xs)
        assert ys[32 * g:32 * g + 32] == want[0] and quot[32 * g * n:32 * (g + 1) * n].tobytes() == want[1], "fr_open differs from Python integers at polynomial %d" % g
    row = {"form": form, "k": k, "n": n, "bytes": k * n * 32, "polynomials_compared": len({0, k - 1})}
    row["fr_open"] = timed(fr_open)

    r = random.Random(5)
    base = [co.sk_to_pk(r.getrandbits(96) | 1) for _ in range(min(n, 1024))]
    table = m.p1s_table_create(c, b"".join(base[i % len(base)] for i in range(n)), 0, 255)
    d_jac = torch.empty((k * 144,), dtype=torch.uint8, device="cuda")
    row["msm_table"] = timed(lambda: m.p1s_mult_table_many_device(c, table, d_quot.data_ptr(), k, 255, d_out=d_jac.data_ptr()))
    m.p1s_table_destroy(table)

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    d_copy = torch.empty((k * n * 32,), dtype=torch.uint8, device="cuda")

    def copy():
        assert hip.hipMemcpy(d_copy.data_ptr(), polys_h.ctypes.data, k * n * 32, 1) == 0      # 1: hipMemcpyHostToDevice

    row["copy_h2d"] = timed(copy)
    row["ratio_copy"] = round(row["copy_h2d"]["median_ms"] / row["fr_open"]["median_ms"], 2)
    row["share_of_msm"] = round(row["fr_open"]["median_ms"] / row["msm_table"]["median_ms"], 2)
    torch.cuda.synchronize()
    c.close()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_fr_open: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up, min..max beside it; fr_open = "
                   "fr_open_many_device (values and quotients), msm_table = p1s_mult_table_many_device over the same (k, n), copy_h2d = one hipMemcpy "
                   "host-to-device of k x n x 32 bytes from pageable memory; ratio_copy = copy_h2d / fr_open, share_of_msm = fr_open / msm_table; the "
                   "first and last polynomial of a row were compared with Python integers before timing",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "rows_where_fr_open_costs_more_than_the_copy": [s for s, r in zip(steps, rows) if r["ratio_copy"] <= 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_open_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--only", default=None, help="comma-separated steps instead of all of them")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    steps = a.only.split(",") if a.only else list(STEPS)
    rows = []
    for s in steps:
        rows.append(child(s, 240))
        print("bench_fr_open: %s %s" % (s, json.dumps(rows[-1])), file=sys.stderr, flush=True)
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_fr_open: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
