#!/usr/bin/env python3
"""Stand-alone benchmark of the all-openings call (mi355_bls_fk20_open_all_many_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_fk20.py [--out profiles/fk20_bench.json]

Every GPU step (one per row) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Everything is
device-resident: the SRS [tau^j]G comes from p1s_lincomb_many_device over a one-row table of G, the k polynomials are random.  Times are
host-clock medians of 5 blocking calls after one warm-up call, with min..max beside them.  Rows (k:n), everything of a row in the same
process on the same context:
  1:128 64:128 1:4096 16:4096 1:65536
      setup_create   mi355_bls_fk20_setup_create_device (once per SRS, not per call)
      open_all       the proofs, flags 0
      open_all_h     MI355_BLS_FK20_H: h instead of the proofs, the last transform not run
      n_fold         the existing route: fr_open_many_device over the polynomial replicated once per domain element and the domain, the
                     quotients through p1s_mult_pippenger_many_device over the SRS, p1s_to_affine_device - for the FIRST `n_fold_openings` of
                     the row's k n openings (all of them while their quotients fit 256 MiB, that is 8 Mi / n), compared byte for byte with
                     the new call's proofs before anything is timed.  n_fold_scaled_ms = the median x k n / n_fold_openings: where the
                     subset is not the whole row the figure is SCALED, not measured, and n_fold_is_scaled says so.
  ratio_n_fold = n_fold_scaled_ms / open_all (above 1: the new call wins).  --only STEP,STEP runs some rows; the file then says which, and
  that it is partial."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = ["%d:%d" % (k, n) for k, n in ((1, 128), (64, 128), (1, 4096), (16, 4096), (1, 65536))]
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


def step(name):
    import random
    import torch
    m = load()
    import frntt_cases as fc
    import p1ntt_cases as pc
    k, n = (int(x) for x in name.split(":"))
    c = m.BatchedBLSVerifierCache.init(max_sets=64)
    rng = random.Random(20261021 + n + k)
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
    d_polys = dev(b"".join(fc.le(rng.randrange(fc.R)) for _ in range(k * n)))
    d_out, d_h = empty(k * n * 96), empty(k * n * 96)
    made = []

    def create():
        for s in made:
            m.fk20_setup_destroy(s)
        made[:] = [m.fk20_setup_create_device(c, d_srs.data_ptr(), n)]
    row = {"k": k, "n": n, "setup_bytes": m.fk20_setup_sizeof(n), "setup_create": timed(create, 3)}
    setup = made[0]
    row["open_all"] = timed(lambda: m.fk20OpenAllMany_device(c, setup, d_polys.data_ptr(), k, d_out.data_ptr(), 0, want_status=False))
    row["open_all_h"] = timed(lambda: m.fk20OpenAllMany_device(c, setup, d_polys.data_ptr(), k, d_h.data_ptr(), m.FK20_H, want_status=False))
    # the n-fold route over the first S openings
    S = min(k * n, QUOT_BYTES // (n * 32))
    dom, w, x = [], fc.omega(n), 1
    for _ in range(n):
        dom.append(fc.le(x))
        x = x * w % fc.R
    d_zs = dev(b"".join(dom[e % n] for e in range(S)))
    which = torch.tensor([e // n for e in range(S)], device="cuda")
    d_rep = d_polys.view(k, n * 32)[which].contiguous()
    d_quot, d_jac, d_old = empty(S * n * 32), empty(S * 144), empty(S * 96)

    def n_fold():
        m.frOpenMany_device(c, d_rep.data_ptr(), n, d_zs.data_ptr(), S, 0, None, None, d_quot.data_ptr(), want_status=False)
        m.p1s_mult_pippenger_many_device(c, d_srs.data_ptr(), n, d_quot.data_ptr(), None, S, 255, d_out=d_jac.data_ptr())
        m.p1s_to_affine_device(c, d_jac.data_ptr(), S, d_old.data_ptr())
    n_fold()
    torch.cuda.synchronize()
    assert bytes(d_old.cpu().numpy()) == bytes(d_out[:S * 96].cpu().numpy()), "the n-fold route's proofs differ from fk20_open_all_many's"
    row["n_fold"] = timed(n_fold, 3)
    row["n_fold_openings"] = S
    row["n_fold_is_scaled"] = S != k * n
    row["n_fold_scaled_ms"] = round(row["n_fold"]["median_ms"] * k * n / S, 3)
    row["ratio_n_fold"] = round(row["n_fold_scaled_ms"] / row["open_all"]["median_ms"], 2)
    torch.cuda.synchronize()
    m.fk20_setup_destroy(setup)
    c.close()
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_fk20: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def summary(rows, steps):
    missing = [x for x in STEPS if x not in steps]
    return {"how": "ms per blocking call on device-resident input, host clock, median of 5 after a warm-up (setup_create, n_fold: of 3), min..max beside it; "
                   "open_all / open_all_h = fk20_open_all_many_device with flags 0 / MI355_BLS_FK20_H; setup_create = fk20_setup_create_device; n_fold = "
                   "fr_open_many_device + p1s_mult_pippenger_many_device + p1s_to_affine_device over the first n_fold_openings of the row's k n openings, "
                   "compared byte for byte with open_all's proofs before timing; n_fold_scaled_ms = n_fold x k n / n_fold_openings (SCALED where "
                   "n_fold_is_scaled); ratio_n_fold = n_fold_scaled_ms / open_all.  The pointwise product runs as a kernel of its own; the form fused "
                   "into the inverse's first stage was not built",
            "steps": list(steps),
            "partial": ("only %d of the tool's %d rows ran (--only); not run: %s" % (len(steps), len(STEPS), ", ".join(missing))) if missing else None,
            "rows": rows,
            "rows_where_open_all_loses_to_the_n_fold_route": [s for s, r in zip(steps, rows) if r["ratio_n_fold"] <= 1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk20_bench.json"))
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
        print("bench_fk20: %s %s" % (s, json.dumps(rows[-1])), file=sys.stderr, flush=True)
    res = summary(rows, steps)
    if res["partial"]:
        print("bench_fk20: PARTIAL table: " + res["partial"], file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
