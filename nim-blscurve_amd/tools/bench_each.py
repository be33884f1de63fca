#!/usr/bin/env python3
"""Stand-alone benchmark of per-set verification (mi355_bls_verify_each, mi355_bls_batch_verify_locate); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_each.py [--out profiles/verify_each_bench.json] [--sweep profiles/verify_each_sweep.txt]

Every GPU step runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs come from the device signer.
Rows: ms per blocking call of verify_each at 64 / 4 096 / 65 536 sets, all valid and with 1 % bad sets (there is no data-dependent path: the two
must agree); batch_verify_locate at 65 536 sets with one bad set beside the same run's batchVerify; and the only way the library had to produce
the same verdict vector before - mi355_bls_batch_verify_many with k = n batches of one set, failing case - measured at 1 024 sets and
extrapolated linearly to 65 536 (one device call per set).  --sweep: verify_each around the hand-over sizes of the plan, latency mode (the
engine forms below them) against throughput mode (one lane per item at every size)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = (64, 4096, 65536)


def load():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.load_package()


def inputs(m, cache, n, bad_every=0):
    sks = b"".join(hashlib.sha256(b"bench each sk %d" % i).digest()[:31] + b"\x00" for i in range(n))
    msgs = b"".join(hashlib.sha256(b"bench each msg %d" % i).digest() for i in range(n))
    ok, rec, _ = m.signSets(cache, sks, msgs)
    assert ok
    if bad_every:
        b = bytearray(rec)
        for i in range(0, n, bad_every):
            b[320 * i + 96] ^= 1
        rec = bytes(b)
    return rec


def ms_per_call(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3)


def step_each(n, bad_every):
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=max(n, 64), numThreads=4096)
    rec = inputs(m, c, n, bad_every)
    v = m.verifyEach(c, rec)
    assert v.count(False) == (len(range(0, n, bad_every)) if bad_every else 0)
    return {"ms": ms_per_call(lambda: m.verifyEach(c, rec), 5), "device_ms": round(c.timings()["total"], 3), "bad": v.count(False)}


def step_locate(n):
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4096)
    rnd = hashlib.sha256(b"bench each rnd").digest()
    good = inputs(m, c, n)
    bad = bytearray(good)
    bad[320 * (n // 2) + 96] ^= 1
    bad = bytes(bad)
    assert m.batchVerify(c, good, rnd) is True
    ok, v = m.batchVerifyLocate(c, bad, rnd)
    assert ok is False and [i for i, x in enumerate(v) if not x] == [n // 2]
    return {"batch_verify_ms": ms_per_call(lambda: m.batchVerify(c, good, rnd), 5),
            "verify_each_ms": ms_per_call(lambda: m.verifyEach(c, bad), 5),
            "locate_one_bad_ms": ms_per_call(lambda: m.batchVerifyLocate(c, bad, rnd), 5),
            "locate_all_valid_ms": ms_per_call(lambda: m.batchVerifyLocate(c, good, rnd), 5)}


def step_parent(n):
    """k = n batches of one set through batch_verify_many, one of them bad: the merged pass fails, then one device call per set"""
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4096)
    rec = inputs(m, c, n, bad_every=n)              # set 0 bad
    batches = [rec[320 * i:320 * i + 320] for i in range(n)]
    rnds = [hashlib.sha256(b"bench each many %d" % i).digest() for i in range(n)]
    v = m.batchVerifyMany(c, batches, rnds)
    assert v == [False] + [True] * (n - 1)
    return {"n": n, "ms": ms_per_call(lambda: m.batchVerifyMany(c, batches, rnds), 2)}


def step_sweep():
    import torch
    m = load()
    S = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    c = m.BatchedBLSVerifierCache.init(max_sets=16384, numThreads=4096)
    rec = inputs(m, c, 16384)
    rows = []
    for n in (1, 64, S // 2, S, 2 * S, 4 * S, 6 * S, 7 * S, 7 * S + 1, 8 * S, 9 * S, 9 * S + 1, 11 * S, 11 * S + 1, 16384):
        row = {"n": n}
        for coop in (True, False):
            c.set_cooperative(coop)
            row["latency_mode_ms" if coop else "throughput_mode_ms"] = ms_per_call(lambda: m.verifyEach(c, rec[:320 * n]), 3)
        rows.append(row)
    return {"slots": S, "rows": rows}


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_each: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_each_bench.json"))
    ap.add_argument("--sweep", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        kind, _, arg = a.step.partition(":")
        if kind == "each":
            n, bad = arg.split(",")
            r = step_each(int(n), int(bad))
        elif kind == "locate":
            r = step_locate(int(arg))
        elif kind == "parent":
            r = step_parent(int(arg))
        else:
            r = step_sweep()
        print(json.dumps(r))
        return
    if a.sweep:
        r = child("sweep", 300)
        with open(a.sweep, "w") as f:
            f.write("verify_each, ms per blocking call (median of 3), wave slots S = %d.  latency mode: the tail on the Fp12 engine up to 7 S sets, Miller lines on\n"
                    "the lane-team engine up to 9 S sets (18 S pairs), cofactor clearing up to 11 S; throughput mode: one lane per item in every stage at every size\n" % r["slots"])
            f.write("%8s %16s %18s\n" % ("n", "latency_mode_ms", "throughput_mode_ms"))
            for row in r["rows"]:
                f.write("%8d %16.3f %18.3f\n" % (row["n"], row["latency_mode_ms"], row["throughput_mode_ms"]))
        print(open(a.sweep).read())
        return
    res = {"verify_each_ms": {}, "verify_each_1pct_bad_ms": {}}
    for n in SIZES:
        res["verify_each_ms"][str(n)] = child("each:%d,0" % n, 240)
        res["verify_each_1pct_bad_ms"][str(n)] = child("each:%d,100" % n, 240)
    res["at_65536"] = child("locate:65536", 300)
    par = child("parent:1024", 300)
    res["parent_commit_path"] = {"measured_sets": par["n"], "measured_ms": par["ms"], "extrapolated_65536_ms": round(par["ms"] * 65536 / par["n"], 1),
                                 "how": "mi355_bls_batch_verify_many, k = n batches of one set, one bad: the merged pass, then one device call per set"}
    res["ratio_parent_over_verify_each_65536"] = round(res["parent_commit_path"]["extrapolated_65536_ms"] / res["at_65536"]["verify_each_ms"], 1)
    res["ratio_verify_each_over_batch_verify_65536"] = round(res["at_65536"]["verify_each_ms"] / res["at_65536"]["batch_verify_ms"], 2)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
