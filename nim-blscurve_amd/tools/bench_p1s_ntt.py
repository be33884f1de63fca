#!/usr/bin/env python3
"""Stand-alone benchmark of the transforms over G1 (mi355_bls_p1s_ntt_many_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_p1s_ntt.py [--out profiles/p1s_ntt_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: k x n points [a_j]G for random a_j, made by p1s_lincomb_many_device over a one-row table of G.  Before anything is timed
the forward transform of the first and the last vector is compared, byte for byte, with [fr_ntt(a)_i]G made the same way from Python
integers, and the inverse of the forward output with the input.  Times are host-clock medians of 5 blocking calls after one warm-up call,
with min..max beside them.  Rows (k:n), each comparison in the same process on the same context:
  1:128 64:128 1:4096 8:4096 1:65536
      forward, inverse, forward_bitrev   the new call (natural order: the last store permutes; BITREV: no permutation)
      definition_lincomb   n <= 128: ONE vector's transform by its definition, p1s_lincomb_many_device over n groups of n terms with the DFT
                           matrix as scalars (compared with the transform's output first); a row of k vectors pays it k times
  def:4096
      definition_msm       n = 4096, k = 1: p1s_mult_pippenger_many_device, n MSMs over the shared n points with the DFT matrix as scalars
                           (to affine and compared with the transform's output first), beside the forward call on the same points
  multiplications_per_s = ((n / 2) log2 n - (n - 1)) k / the forward time.  ratio_definition = definition x k / forward (above 1: the
  transform wins).  --only STEP,STEP runs some rows; the file then says which, and that it is partial."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ["%d:%d" % (k, n) for k, n in ((1, 128), (64, 128), (1, 4096), (8, 4096), (1, 65536))] + ["def:4096"]


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


def multiples_of_g(m, c, scalars):
    """[a]G for each scalar -> a device tensor of 96-byte affine images (p1s_lincomb_many_device over the one-row table of G)"""
    import torch
    import frntt_cases as fc
    import p1ntt_cases as pc
    count = len(scalars)
    d_tab = torch.frombuffer(bytearray(pc.G_IMAGE), dtype=torch.uint8).cuda()
    d_idx = torch.zeros(count, dtype=torch.int32, device="cuda")
    d_sc = torch.frombuffer(bytearray(b"".join(fc.le(a) for a in scalars)), dtype=torch.uint8).cuda()
    d_out = torch.empty((count * 96,), dtype=torch.uint8, device="cuda")
    m.p1sLincombMany_device(c, d_tab.data_ptr(), 1, d_idx.data_ptr(), list(range(count + 1)), d_sc.data_ptr(), d_out.data_ptr())
    return d_out


def dft_matrix(n):
    """the n x n scalars omega_n^(i j) as a numpy array of n^2 32-byte little-endian images, row i the scalars of output i"""
    import numpy as np
    import frntt_cases as fc
    w, p, powers = fc.omega(n), 1, []
    for _ in range(n):
        powers.append(fc.le(p))
        p = p * w % fc.R
    table = np.frombuffer(b"".join(powers), dtype=np.uint8).reshape(n, 32)
    i = np.arange(n, dtype=np.int64)
    return table[(i[:, None] * i[None, :]) % n].reshape(n * n, 32)


def setup(m, c, k, n):
    """-> (scalars, device points, device output buffers); the forward transform checked against Python integers, the inverse against the input"""
    import random
    import torch
    import frntt_cases as fc
    rng = random.Random(20261020 + n)
    vectors = [[rng.randrange(fc.R) for _ in range(n)] for _ in range(k)]
    d_in = multiples_of_g(m, c, [a for v in vectors for a in v])
    d_out, d_back = torch.empty_like(d_in), torch.empty_like(d_in)
    m.p1sNttMany_device(c, d_in.data_ptr(), n, k, 0, d_out.data_ptr())
    torch.cuda.synchronize()
    out = bytes(d_out.cpu().numpy())
    for g in sorted({0, k - 1}):
        want = bytes(multiples_of_g(m, c, fc.ntt(vectors[g])).cpu().numpy())
        assert out[96 * g * n:96 * (g + 1) * n] == want, "p1s_ntt differs from [fr_ntt(a)]G at vector %d" % g
    m.p1sNttMany_device(c, d_out.data_ptr(), n, k, m.P1S_NTT_INVERSE, d_back.data_ptr())
    torch.cuda.synchronize()
    assert bytes(d_back.cpu().numpy()) == bytes(d_in.cpu().numpy()), "the inverse of the forward transform is not the input"
    return vectors, d_in, d_out, d_back


def step(name):
    import torch
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    if name.startswith("def:"):
        n = int(name.split(":")[1])
        _, d_in, d_out, _ = setup(m, c, 1, n)
        d_sc = torch.from_numpy(dft_matrix(n)).cuda()
        d_jac = torch.empty((n * 144,), dtype=torch.uint8, device="cuda")
        d_aff = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
        msm = lambda: m.p1s_mult_pippenger_many_device(c, d_in.data_ptr(), n, d_sc.data_ptr(), None, n, 255, d_jac.data_ptr())      # noqa: E731
        msm()
        m.p1s_to_affine_device(c, d_jac.data_ptr(), n, d_aff.data_ptr())
        torch.cuda.synchronize()
        assert bytes(d_aff.cpu().numpy()) == bytes(d_out.cpu().numpy()), "the n MSMs of the definition differ from the transform"
        row = {"k": 1, "n": n, "definition_msm": timed(msm, 3), "forward": timed(lambda: m.p1sNttMany_device(c, d_in.data_ptr(), n, 1, 0, d_out.data_ptr()))}
        row["ratio_definition"] = round(row["definition_msm"]["median_ms"] / row["forward"]["median_ms"], 2)
    else:
        k, n = (int(x) for x in name.split(":"))
        _, d_in, d_out, d_back = setup(m, c, k, n)
        ntt = lambda flags, src=d_in, dst=d_out: m.p1sNttMany_device(c, src.data_ptr(), n, k, flags, dst.data_ptr())      # noqa: E731
        row = {"k": k, "n": n, "bytes": k * n * 96, "vectors_compared": len({0, k - 1})}
        row["forward"] = timed(lambda: ntt(0))
        row["inverse"] = timed(lambda: ntt(m.P1S_NTT_INVERSE, d_out, d_back))
        row["forward_bitrev"] = timed(lambda: ntt(m.P1S_NTT_BITREV))
        log2n = n.bit_length() - 1
        row["multiplications_per_s"] = round(((n // 2) * log2n - (n - 1)) * k / (row["forward"]["median_ms"] * 1e-3))
        if n <= 128:
            ntt(0)
            torch.cuda.synchronize()
            first = bytes(d_out[:n * 96].cpu().numpy())
            d_sc = torch.from_numpy(dft_matrix(n)).cuda()
            d_idx = torch.arange(n, dtype=torch.int32, device="cuda").repeat(n)
            d_def = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
            offs = [i * n for i in range(n + 1)]
            lin = lambda: m.p1sLincombMany_device(c, d_in.data_ptr(), n, d_idx.data_ptr(), offs, d_sc.data_ptr(), d_def.data_ptr())      # noqa: E731
            lin()
            torch.cuda.synchronize()
            assert bytes(d_def.cpu().numpy()) == first, "the definition by lincomb differs from the transform"
            row["definition_lincomb"] = timed(lin)
            row["ratio_definition"] = round(row["definition_lincomb"]["median_ms"] * k / row["forward"]["median_ms"], 2)
    torch.cuda.synchronize()
    c.close()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_p1s_ntt: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up (definition_msm: of 3), min..max beside it; "
                   "forward / inverse / forward_bitrev = p1s_ntt_many_device; definition_lincomb = ONE vector by p1s_lincomb_many_device over n groups of "
                   "n terms with the DFT matrix as scalars; definition_msm = p1s_mult_pippenger_many_device, n MSMs over the shared n points; "
                   "multiplications_per_s = ((n / 2) log2 n - (n - 1)) k / forward; ratio_definition = definition x k / forward; the outputs were "
                   "compared with [fr_ntt(a)]G and with the definition's before timing",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "rows_where_the_transform_loses_to_the_definition": [s for s, r in zip(steps, rows) if r.get("ratio_definition") is not None and r["ratio_definition"] <= 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p1s_ntt_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--only", default=None, help="comma-separated steps instead of all of them")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    steps = a.only.split(",") if a.only else list(STEPS)
    rows = []
    for s in steps:
        rows.append(child(s, 300))
        print("bench_p1s_ntt: %s %s" % (s, json.dumps(rows[-1])), file=sys.stderr, flush=True)
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_p1s_ntt: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
