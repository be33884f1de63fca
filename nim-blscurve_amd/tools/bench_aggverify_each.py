#!/usr/bin/env python3
"""Stand-alone benchmark of the batched aggregateVerify (mi355_bls_aggregate_verify_each_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_aggverify_each.py [--out profiles/aggregate_verify_each_bench.json]

Every GPU step (one per number of pairs) runs in a child process of its own under `timeout`; the first step that fails ends the run.
Inputs: `pairs` sets with distinct keys and messages from the device signer, cut into groups of 1, 4 and 16 pairs; the groups' signatures
come from mi355_bls_aggregate_signature_sets_device and stay on the device, like keys and messages.  Every verdict must be 1, and a group
with one wrong message must be the only 0, before anything is timed.  Times are host-clock medians around blocking calls (each ends in a
stream synchronise), after one warm-up call; min and max of the same calls are the run-to-run spread.  Rows per pairs x group size:
  (a) aggregate_verify_each_device alone: k = pairs / size groups in one call;
  (b) the only route before this call, one mi355_bls_aggregate_verify call per group - the one-shot path, which this library leaves as
      the parent commit had it: timed on at most 256 groups and SCALED to k;
  (c) mi355_bls_verify_each_device over the same number of pairs (as many sets): what the same pairs cost when each carries its own signature.
The item width (plan.hpp AGGV_C) and the tail hand-over are the committed ones; no other value was tried, so there is no A/B row."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PAIRS = (256, 16384, 65536)
SIZES = (1, 4, 16)
ONE_SHOT_GROUPS_MAX = 256


def load():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def ms_per_call(fn, reps):
    """-> {"median", "min", "max"} in ms of `reps` calls after one warm-up"""
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step(pairs):
    import numpy as np
    import torch
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=max(pairs, 64), numThreads=4096)
    rng = np.random.default_rng(20261018)
    sks = rng.integers(1, 255, size=(pairs, 32), dtype=np.uint8)
    sks[:, 31] = 0                                                           # below the group order
    msgs = b"".join(hashlib.sha256(b"bench aggverify_each %d" % i).digest() for i in range(pairs))
    ok, rec, _ = m.signSets(c, sks.tobytes(), msgs)
    assert ok
    r = np.frombuffer(rec, dtype=np.uint8).reshape(pairs, 320)
    d_rec = torch.from_numpy(r.copy()).cuda()
    d_keys = torch.from_numpy(np.ascontiguousarray(r[:, :96])).cuda()
    d_msgs = torch.from_numpy(np.ascontiguousarray(r[:, 96:128])).cuda()
    d_sigs = torch.from_numpy(np.ascontiguousarray(r[:, 128:])).cuda()
    rows = []
    for size in SIZES:
        k = pairs // size
        offs = [g * size for g in range(k + 1)]
        d_agg = torch.zeros((k, 192), dtype=torch.uint8, device="cuda")
        ok, st = m.aggregateSignatureSets_device(c, d_sigs.data_ptr(), pairs, None, offs, d_agg.data_ptr(), None)
        assert ok and st == bytes(k)
        row = {"pairs": pairs, "group_size": size, "k": k}

        def each():
            return m.aggregateVerifyEach_device(c, d_keys.data_ptr(), pairs, None, offs, d_msgs.data_ptr(), d_agg.data_ptr())
        assert each() == [True] * k
        bad = d_msgs.clone()
        bad[(k // 2) * size + size - 1, 0] ^= 1                              # one wrong message: its group alone fails
        assert m.aggregateVerifyEach_device(c, d_keys.data_ptr(), pairs, None, offs, bad.data_ptr(), d_agg.data_ptr()) == [g != k // 2 for g in range(k)]
        row["a_aggregate_verify_each_ms"] = ms_per_call(each, 5)
        nb = min(k, ONE_SHOT_GROUPS_MAX)
        agg = d_agg.cpu().numpy()
        groups = [([r[j, :96].tobytes() for j in range(g * size, g * size + size)], [r[j, 96:128].tobytes() for j in range(g * size, g * size + size)],
                   agg[g].tobytes()) for g in range(nb)]

        def one_shot():
            for pks, ms, sig in groups:
                assert m.aggregateVerify(c, pks, ms, sig)
        t = ms_per_call(one_shot, 2)
        row["b_one_call_per_group"] = {"measured_groups": nb, "measured_ms": t, "scaled_to_k_ms": round(t["median"] * k / nb, 1), "scaled": nb != k}
        row["c_verify_each_same_pairs_ms"] = ms_per_call(lambda: m.verifyEach_device(c, d_rec.data_ptr(), pairs), 5)
        a = row["a_aggregate_verify_each_ms"]
        row["one_call_per_group_over_each"] = round(row["b_one_call_per_group"]["scaled_to_k_ms"] / a["median"], 1)
        row["verify_each_over_each"] = round(row["c_verify_each_same_pairs_ms"]["median"] / a["median"], 2)
        row["beats_one_call_per_group_beyond_spread"] = row["b_one_call_per_group"]["scaled_to_k_ms"] > a["max"] + (a["max"] - a["min"])
        rows.append(row)
        del d_agg, bad
    return rows


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_aggverify_each: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_verify_each_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--pairs", default=",".join(str(k) for k in PAIRS), help="the pair counts to run, comma separated")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = []
    for n in (int(x) for x in a.pairs.split(",")):
        rows += child(str(n), 420)
    res = {"how": "ms per blocking call, host clock: median, min and max of 5 calls after a warm-up (b: of 2) - min .. max is the run-to-run spread; "
                  "b is the one-shot mi355_bls_aggregate_verify (unchanged from the parent commit) on at most 256 groups, scaled linearly to k "
                  "where `scaled` is true; item width AGGV_C = 8 and verify_each's tail hand-over, no other values tried",
           "rows": rows,
           "every_row_beats_one_call_per_group": all(r["beats_one_call_per_group_beyond_spread"] for r in rows)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
