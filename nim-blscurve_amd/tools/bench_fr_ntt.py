#!/usr/bin/env python3
"""Stand-alone benchmark of the transforms over Fr (mi355_bls_fr_ntt_many_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_fr_ntt.py [--out profiles/fr_ntt_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: k x n random images below 2^254.  Before anything is timed the first and the last vector of the forward transform are
compared with Python integers mod r, and the inverse of the forward output with the input.  Times are host-clock medians of 5 blocking
calls after one warm-up call, with min..max beside them.  Rows (k:n), each comparison in the same process on the same context:
  1:4096 64:4096 512:4096 64:256 64:65536 1:1048576
      forward, inverse   the new call in natural order (the last store permutes), at the plan's tile
      tile_10, tile_12   the same two at each candidate default tile, set through mi355_bls_debug_frntt_set_tile
      forward_bitrev     the forward call with FR_NTT_BITREV (no permutation)
      fr_open            fr_open_many_device in coefficient form over the same (k, n), values and quotients
      copy_h2d           ONE hipMemcpy host-to-device of k x n x 32 bytes from pageable memory - the copy the host route cannot avoid
  products_per_s = (n / 2) log2 n k / the forward time; ratio_copy = copy_h2d / forward (above 1: the transform costs less than the copy
  alone).  --only STEP,STEP runs some rows; the file then says which, and that it is partial."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ["%d:%d" % (k, n) for k, n in ((1, 4096), (64, 4096), (512, 4096), (64, 256), (64, 65536), (1, 1 << 20))]
TILES = (10, 12)


def load():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
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
    k, n = (int(x) for x in name.split(":"))
    m = load()
    import frntt_cases as fc
    rng = np.random.default_rng(20261020)
    in_h = rng.integers(0, 256, size=(k * n, 32), dtype=np.uint8)
    in_h[:, 31] &= 0x3f
    d_in = torch.from_numpy(in_h).cuda()
    d_out = torch.empty((k * n * 32,), dtype=torch.uint8, device="cuda")
    d_back = torch.empty((k * n * 32,), dtype=torch.uint8, device="cuda")
    c = m.BatchedBLSVerifierCache.init(max_sets=64)

    def ntt(flags, src=d_in, dst=d_out):
        return m.frNttMany_device(c, src.data_ptr(), n, k, flags, None, dst.data_ptr())

    assert ntt(0)[0] == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for g in sorted({0, k - 1}):
        vec = fc.images(in_h[g * n:(g + 1) * n].tobytes())
        assert out[32 * g * n:32 * (g + 1) * n].tobytes() == fc.pack([fc.ntt(vec)]), "fr_ntt differs from Python integers at vector %d" % g
    assert ntt(m.FR_NTT_INVERSE, d_out, d_back)[0] == 0
    torch.cuda.synchronize()
    assert bytes(d_back.cpu().numpy()) == in_h.tobytes(), "the inverse of the forward transform is not the input"
    row = {"k": k, "n": n, "bytes": k * n * 32, "vectors_compared": len({0, k - 1})}
    row["forward"] = timed(lambda: ntt(0))
    row["inverse"] = timed(lambda: ntt(m.FR_NTT_INVERSE, d_out, d_back))
    row["forward_bitrev"] = timed(lambda: ntt(m.FR_NTT_BITREV))
    for t in TILES:
        m.debug_frntt_set_tile(c, t)
        row["tile_%d" % t] = {"forward": timed(lambda: ntt(0)), "inverse": timed(lambda: ntt(m.FR_NTT_INVERSE, d_out, d_back))}
    m.debug_frntt_set_tile(c, 0)
    log2n = n.bit_length() - 1
    row["products_per_s"] = round((n // 2) * log2n * k / (row["forward"]["median_ms"] * 1e-3)) if log2n else None

    d_zs = torch.from_numpy(in_h[:k].copy()).cuda()
    d_ys = torch.empty((k * 32,), dtype=torch.uint8, device="cuda")
    row["fr_open"] = timed(lambda: m.frOpenMany_device(c, d_in.data_ptr(), n, d_zs.data_ptr(), k, 0, None, d_ys.data_ptr(), d_out.data_ptr()))

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def copy():
        assert hip.hipMemcpy(d_back.data_ptr(), in_h.ctypes.data, k * n * 32, 1) == 0      # 1: hipMemcpyHostToDevice

    row["copy_h2d"] = timed(copy)
    row["ratio_copy"] = round(row["copy_h2d"]["median_ms"] / row["forward"]["median_ms"], 2)
    row["ratio_fr_open"] = round(row["fr_open"]["median_ms"] / row["forward"]["median_ms"], 2)
    torch.cuda.synchronize()
    c.close()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_fr_ntt: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up, min..max beside it; forward / inverse = "
                   "fr_ntt_many_device in natural order at the plan's tile, tile_T the same with a tile of 2^T elements set through the hook, "
                   "forward_bitrev with FR_NTT_BITREV, fr_open = fr_open_many_device in coefficient form over the same (k, n), copy_h2d = one hipMemcpy "
                   "host-to-device of k x n x 32 bytes from pageable memory; products_per_s = (n / 2) log2 n k / forward, ratio_copy = copy_h2d / forward, "
                   "ratio_fr_open = fr_open / forward; the first and last vector of a row were compared with Python integers before timing",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "rows_where_the_transform_costs_more_than_the_copy": [s for s, r in zip(steps, rows) if r["ratio_copy"] <= 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_ntt_bench.json"))
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
        print("bench_fr_ntt: %s %s" % (s, json.dumps(rows[-1])), file=sys.stderr, flush=True)
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_fr_ntt: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
