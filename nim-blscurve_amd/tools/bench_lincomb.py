#!/usr/bin/env python3
"""Stand-alone benchmark of the short linear combinations per group (mi355_bls_p1s_lincomb_many_device / mi355_bls_p2s_lincomb_many_device);
bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_lincomb.py [--out profiles/lincomb_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs are
device-resident: G2 points from 1 024 distinct signatures of one message (G1: 1 024 distinct public keys), repeated, laid out contiguously;
the openings rows (4 096 x 2 on G2) address a ONE-ROW table, the G2 generator, through an index array of zeros.  32 random scalar bytes per
term.  Before anything is timed the images of the new call - both routes on G2 - are compared byte for byte with the many-MSM call followed
by to_affine over the same inputs (every group of the row).  Times are host-clock medians of 5 blocking calls after one warm-up call, with
min..max beside them.  Rows (curve:k:terms per group:nbits), each comparison in the same process on the same context:
  g2:4096:2:255  g2:4096:2:64  g2:256:3:255  g2:65536:1:255  g2:4096:16:255  g1:4096:2:255  g1:4096:2:64  g1:65536:1:255
      lincomb          the new call, flags 0 (the scalar as an integer)
      lincomb_psi      G2 only: the new call under LINCOMB_SUBGROUP
      many_to_affine   p?s_mult_pippenger_many_device + p?s_to_affine_device: the route a caller had
      recover          g2:256:3:255 only: recover_signature_sets_device over the same shares with random ids (it derives its own coefficients)
  ratio_many = many_to_affine / lincomb, ratio_many_psi = many_to_affine / lincomb_psi, ratio_psi = lincomb / lincomb_psi,
  ratio_recover = recover / lincomb (above 1: the call named second is faster).  --only STEP,STEP runs some rows; the file then says which,
and that it is partial."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ["g2:4096:2:255", "g2:4096:2:64", "g2:256:3:255", "g2:65536:1:255", "g2:4096:16:255", "g1:4096:2:255", "g1:4096:2:64", "g1:65536:1:255"]


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


def base_points(g2, count):
    import c_oracle as co
    r = random.Random(5)
    if g2:
        return [co.sign(r.getrandbits(96) | 1, b"bench lincomb") for _ in range(count)]
    return [co.sk_to_pk(r.getrandbits(96) | 1) for _ in range(count)]


def step(name):
    import numpy as np
    import torch
    curve, k, per, nbits = name.split(":")
    g2, k, per, nbits = curve == "g2", int(k), int(per), int(nbits)
    m = load()
    import bls12381_py as o
    row_b, jac_b = (192, 288) if g2 else (96, 144)
    terms = k * per
    openings = g2 and per == 2
    if openings:
        gen = o.g2_to_blst_affine(o.G2_GEN)
        d_table = torch.frombuffer(bytearray(gen), dtype=torch.uint8).cuda()
        d_idx = torch.zeros(terms, dtype=torch.int32, device="cuda")
        d_flat = d_table.repeat(terms).contiguous()                                  # what the many-MSM call needs: the point of every term
        n_table = 1
    else:
        base = base_points(g2, 1024)
        d_flat = torch.frombuffer(bytearray(b"".join(base[i % 1024] for i in range(min(terms, 1024)))), dtype=torch.uint8).cuda()
        if terms > 1024:
            d_flat = d_flat.repeat(terms // 1024).contiguous()
        d_table, d_idx, n_table = d_flat, None, terms
    rng = np.random.default_rng(20261020)
    d_sc = torch.from_numpy(rng.integers(0, 256, size=(terms, 32), dtype=np.uint8)).cuda()
    offs = [per * j for j in range(k + 1)]
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    d_out = torch.empty((k * row_b,), dtype=torch.uint8, device="cuda")
    d_jac = torch.empty((k * jac_b,), dtype=torch.uint8, device="cuda")
    d_aff = torch.empty((k * row_b,), dtype=torch.uint8, device="cuda")
    lincomb_dev = m.p2sLincombMany_device if g2 else m.p1sLincombMany_device
    I = d_idx.data_ptr() if d_idx is not None else None

    def lincomb(flags=0):
        return lincomb_dev(c, d_table.data_ptr(), n_table, I, offs, d_sc.data_ptr(), d_out.data_ptr(), nbits, flags)

    def many_to_affine():
        if g2:
            m.p2s_mult_pippenger_many_device(c, d_flat.data_ptr(), terms, d_sc.data_ptr(), offs, k, nbits, d_out=d_jac.data_ptr(), ret=False)
            m.p2s_to_affine_device(c, d_jac.data_ptr(), k, d_aff.data_ptr())
        else:
            m.p1s_mult_pippenger_many_device(c, d_flat.data_ptr(), terms, d_sc.data_ptr(), offs, k, nbits, d_out=d_jac.data_ptr())
            m.p1s_to_affine_device(c, d_jac.data_ptr(), k, d_aff.data_ptr())

    many_to_affine()
    torch.cuda.synchronize()
    want = bytes(d_aff.cpu().numpy())
    for flags in ((0, m.LINCOMB_SUBGROUP) if g2 else (0,)):
        d_out.zero_()
        ok, st = lincomb(flags)
        torch.cuda.synchronize()
        assert ok and bytes(d_out.cpu().numpy()) == want, "lincomb (flags %d) differs from many + to_affine" % flags
    row = {"curve": curve, "k": k, "terms_per_group": per, "terms": terms, "nbits": nbits, "one_row_table_idx_all_0": openings, "images_compared": k}
    row["lincomb"] = timed(lincomb)
    if g2:
        row["lincomb_psi"] = timed(lambda: lincomb(m.LINCOMB_SUBGROUP))
        row["ratio_psi"] = round(row["lincomb"]["median_ms"] / row["lincomb_psi"]["median_ms"], 2)
    row["many_to_affine"] = timed(many_to_affine)
    row["ratio_many"] = round(row["many_to_affine"]["median_ms"] / row["lincomb"]["median_ms"], 2)
    if g2:
        row["ratio_many_psi"] = round(row["many_to_affine"]["median_ms"] / row["lincomb_psi"]["median_ms"], 2)
    if g2 and (k, per, nbits) == (256, 3, 255):
        d_ids = torch.from_numpy(rng.integers(0, 256, size=(terms, 32), dtype=np.uint8)).cuda()
        row["recover"] = timed(lambda: m.recoverSignatureSets_device(c, d_flat.data_ptr(), terms, None, offs, d_ids.data_ptr(), d_out.data_ptr(), None))
        row["ratio_recover"] = round(row["recover"]["median_ms"] / row["lincomb"]["median_ms"], 2)
    torch.cuda.synchronize()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_lincomb: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up, min..max beside it; lincomb = "
                   "p?s_lincomb_many_device with flags 0, lincomb_psi = the same under LINCOMB_SUBGROUP (G2), many_to_affine = "
                   "p?s_mult_pippenger_many_device + p?s_to_affine_device over the same terms, recover = recover_signature_sets_device over the same "
                   "shares; ratio_many = many_to_affine / lincomb, ratio_many_psi = many_to_affine / lincomb_psi, ratio_psi = lincomb / lincomb_psi, "
                   "ratio_recover = recover / lincomb; every image of a row was compared with many_to_affine's before timing",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "rows_where_lincomb_loses_to_many_to_affine": [s for s, r in zip(steps, rows) if r["ratio_many"] <= 1],
            "rows_where_psi_loses_to_plain": [s for s, r in zip(steps, rows) if r.get("ratio_psi", 2) <= 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lincomb_bench.json"))
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
        print("bench_lincomb: %s %s" % (s, json.dumps(rows[-1])), file=sys.stderr, flush=True)
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_lincomb: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
