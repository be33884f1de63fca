#!/usr/bin/env python3
"""Stand-alone benchmark of the cell-proof call (mi355_bls_fk20_open_cells_many_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_fk20_cells.py [--out profiles/fk20_cells_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Everything is
device-resident: the SRS [tau^i]G comes from p1s_lincomb_many_device over a one-row table of G, the k polynomials are random.  Times are
host-clock medians of 5 blocking calls after one warm-up call, with min..max beside them.  Rows (k:n:l:ext; N = (n / l) 2^ext cells a
polynomial), everything of a row in the same process on the same context:
  1:4096:64:1 16:4096:64:1 64:4096:64:1 1:128:8:1 16:4096:1:0 1:65536:64:1
      setup_create   mi355_bls_fk20_setup_create_cells_device (once per SRS and cell size, not per call)
      open_cells     the proofs, flags 0
      open_cells_h   MI355_BLS_FK20_H: h instead of the proofs, the last transform not run
      open_all       (l = 1, ext = 0 only) mi355_bls_fk20_open_all_many_device on the same inputs, compared byte for byte with open_cells
                     before timing; ratio_open_all = open_cells / open_all (1: level)
      definition     the definition route: the quotients p(X) div (X^l - omega_N^j) by long division in Python (NOT timed), an MSM of n
                     points each through p1s_mult_pippenger_many_device over the SRS, p1s_to_affine_device - for the FIRST
                     `definition_proofs` of the row's k N proofs (all of them while their quotients fit 256 MiB, that is 8 Mi / n),
                     compared byte for byte with the new call's proofs before anything is timed.  definition_scaled_ms = the median x
                     k N / definition_proofs: where the subset is not the whole row the figure is SCALED, not measured, and
                     definition_is_scaled says so.
  ratio_definition = definition_scaled_ms / open_cells (above 1: the new call wins).  --only STEP,STEP runs some rows; the file then says
  which, and that it is partial."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ["1:4096:64:1", "16:4096:64:1", "64:4096:64:1", "1:128:8:1", "16:4096:1:0", "1:65536:64:1"]
QUOT_BYTES = 256 << 20


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


def quotient(c, l, a, r):
    """the n coefficients (the top l of them 0) of p(X) div (X^l - a)"""
    rem, quo = list(c), [0] * len(c)
    for d in range(len(c) - 1, l - 1, -1):
        quo[d - l] = rem[d]
        rem[d - l] = (rem[d - l] + a * rem[d]) % r
    return quo


def step(name):
    import random
    import torch
    m = load()
    import frntt_cases as fc
    import p1ntt_cases as pc
    k, n, l, ext = (int(x) for x in name.split(":"))
    cells = (n // l) << ext
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    rng = random.Random(20261021 + n + k + l)
    tau = rng.randrange(2, fc.R)
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()      # noqa: E731
    empty = lambda size: torch.empty((size,), dtype=torch.uint8, device="cuda")      # noqa: E731
    powers, p = [], 1
    for _ in range(n):
        powers.append(fc.le(p))
        p = p * tau % fc.R
    d_srs = empty(n * 96)
    d_g, d_zero, d_pow = dev(pc.G_IMAGE), torch.zeros(n, dtype=torch.int32, device="cuda"), dev(b"".join(powers))
    m.p1sLincombMany_device(c, d_g.data_ptr(), 1, d_zero.data_ptr(), list(range(n + 1)), d_pow.data_ptr(), d_srs.data_ptr())
    coefs = [[rng.randrange(fc.R) for _ in range(n)] for _ in range(k)]
    d_polys = dev(fc.pack(coefs))
    d_out, d_h = empty(k * cells * 96), empty(k * (n // l) * 96)
    made = []

    def create():
        for s in made:
            m.fk20_setup_destroy(s)
        made[:] = [m.fk20_setup_create_cells_device(c, d_srs.data_ptr(), n, l)]
    row = {"k": k, "n": n, "cell": l, "ext_log2": ext, "cells": cells, "setup_bytes": m.fk20_setup_sizeof(n), "setup_create": timed(create, 3)}
    setup = made[0]
    row["open_cells"] = timed(lambda: m.fk20OpenCellsMany_device(c, setup, d_polys.data_ptr(), k, d_out.data_ptr(), ext, 0, want_status=False))
    row["open_cells_h"] = timed(lambda: m.fk20OpenCellsMany_device(c, setup, d_polys.data_ptr(), k, d_h.data_ptr(), ext, m.FK20_H, want_status=False))
    if l == 1 and ext == 0:
        d_all = empty(k * n * 96)
        run_all = lambda: m.fk20OpenAllMany_device(c, setup, d_polys.data_ptr(), k, d_all.data_ptr(), 0, want_status=False)      # noqa: E731
        run_all()
        torch.cuda.synchronize()
        assert bytes(d_all.cpu().numpy()) == bytes(d_out.cpu().numpy()), "fk20_open_all_many's proofs differ from fk20_open_cells_many's at cell 1, ext 0"
        row["open_all"] = timed(run_all)
        row["ratio_open_all"] = round(row["open_cells"]["median_ms"] / row["open_all"]["median_ms"], 3)
    # the definition route over the first S proofs
    S = min(k * cells, max(1, QUOT_BYTES // (n * 32)))
    w = fc.omega(cells)
    d_quot = dev(fc.pack([quotient(coefs[e // cells], l, pow(w, e % cells, fc.R), fc.R) for e in range(S)]))
    d_jac, d_old = empty(S * 144), empty(S * 96)

    def definition():
        m.p1s_mult_pippenger_many_device(c, d_srs.data_ptr(), n, d_quot.data_ptr(), None, S, 255, d_out=d_jac.data_ptr())
        m.p1s_to_affine_device(c, d_jac.data_ptr(), S, d_old.data_ptr())
    definition()
    torch.cuda.synchronize()
    assert bytes(d_old.cpu().numpy()) == bytes(d_out[:S * 96].cpu().numpy()), "the definition route's proofs differ from fk20_open_cells_many's"
    row["definition"] = timed(definition, 3)
    row["definition_proofs"] = S
    row["definition_is_scaled"] = S != k * cells
    row["definition_scaled_ms"] = round(row["definition"]["median_ms"] * k * cells / S, 3)
    row["ratio_definition"] = round(row["definition_scaled_ms"] / row["open_cells"]["median_ms"], 2)
    torch.cuda.synchronize()
    m.fk20_setup_destroy(setup)
    c.close()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_fk20_cells: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up (setup_create, definition: of 3), min..max beside "
                   "it; rows k:n:l:ext_log2; open_cells / open_cells_h = fk20_open_cells_many_device with flags 0 / MI355_BLS_FK20_H; setup_create = "
                   "fk20_setup_create_cells_device; open_all (l = 1, ext 0) = fk20_open_all_many_device on the same inputs, ratio_open_all = open_cells / "
                   "open_all; definition = p1s_mult_pippenger_many_device + p1s_to_affine_device over the quotients (long division on the host, NOT timed) "
                   "of the first definition_proofs of the row's k N proofs, compared byte for byte with open_cells' proofs before timing; "
                   "definition_scaled_ms = definition x k N / definition_proofs (SCALED where definition_is_scaled); ratio_definition = "
                   "definition_scaled_ms / open_cells",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "rows_where_open_cells_loses_to_the_definition_route": [s for s, r in zip(steps, rows) if r["ratio_definition"] <= 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk20_cells_bench.json"))
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
        print("bench_fk20_cells: %s %s" % (s, json.dumps(rows[-1])), file=sys.stderr, flush=True)
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_fk20_cells: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:                                # a row a line
        head = {key: v for key, v in res.items() if key != "rows"}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "rows": [\n  %s\n ]\n}\n' % ",\n  ".join(json.dumps(r) for r in res["rows"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
