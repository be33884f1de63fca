#!/usr/bin/env python3
"""Stand-alone benchmark of the per-group signature aggregation (mi355_bls_aggregate_signature_sets_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_aggsigs.py [--out profiles/aggregate_signatures_bench.json]

Every GPU step (one per k) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs: a table of
65 536 signatures on ONE message from the device signer (50-bit secret keys, so that a group's secret sum fits 64 bits), groups drawn by a
seeded RNG with lengths uniform in [mean / 2, 3 mean / 2] as indices into the table.  Every aggregate is compared byte for byte with the
signer's signature by the group's secret sum, and every wire form with c_oracle.compress_sets on a prefix, before anything is timed.  Times
are host-clock medians around blocking calls (each ends in a stream synchronise), after one warm-up call; min and max of the same calls are
the run-to-run spread.  Rows per k x mean group size:
  (a) aggregate_signature_sets_device alone, both outputs, signatures through an index array into the resident table;
  (b) the only route before this call, one mi355_bls_g2_aggregate_device call per group (which still leaves a Jacobian point for the host to
      finish): timed on at most 256 groups and SCALED to k;
  (c) c_oracle.g2_sum per group on 16 host threads: timed on at most 2 048 groups and SCALED to k.
Level 0 keeps plan.hpp's AGG_C signatures per item; no other per-item count was tried, so there is no A/B row."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KS = (64, 4096, 65536)
MEANS = (4, 16, 128)
TABLE = 65536
PARENT_GROUPS_MAX, CPU_GROUPS_MAX, CPU_THREADS = 256, 2048, 16


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


def sign(m, cache, sks, msg):
    """the device signer's signatures (n x 192 bytes, numpy) of one message for 64-bit secret keys (numpy uint64)"""
    import numpy as np
    n = len(sks)
    sk32 = np.zeros((n, 32), dtype=np.uint8)
    sk32[:, :8] = sks.astype("<u8").view(np.uint8).reshape(n, 8)
    ok, rec, _ = m.signSets(cache, sk32.tobytes(), msg * n)
    assert ok
    return np.ascontiguousarray(np.frombuffer(rec, dtype=np.uint8).reshape(n, 320)[:, 128:])


def step(k):
    import numpy as np
    import torch
    from multiprocessing.pool import ThreadPool
    m = load()
    import c_oracle as co
    c = m.BatchedBLSVerifierCache.init(max_sets=max(k, 64), numThreads=4096)
    big = c if k >= TABLE else m.BatchedBLSVerifierCache.init(max_sets=TABLE, numThreads=4096)
    rng = np.random.default_rng(20261018)
    msg = hashlib.sha256(b"bench aggsigs msg").digest()
    sks = rng.integers(1, 1 << 50, size=TABLE, dtype=np.uint64)
    table = sign(m, big, sks, msg)
    d_table = torch.from_numpy(table).cuda()
    L = m.lib()
    rows = []
    for mean in MEANS:
        lengths = rng.integers(mean // 2, mean + mean // 2 + 1, size=k)
        offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
        n_sigs = int(offsets[-1])
        idx = rng.integers(0, TABLE, size=n_sigs, dtype=np.int64)
        sums = np.add.reduceat(sks[idx], offsets[:-1])                       # < 2^50 * 192: no wrap
        want = sign(m, c, sums, msg)
        d_idx = torch.from_numpy(idx.astype(np.int32)).cuda()
        d192 = torch.zeros((k, 192), dtype=torch.uint8, device="cuda")
        d96 = torch.zeros((k, 96), dtype=torch.uint8, device="cuda")
        offs = [int(x) for x in offsets]
        row = {"k": k, "mean_group": mean, "signatures": n_sigs}

        def agg():
            return m.aggregateSignatureSets_device(c, d_table.data_ptr(), TABLE, d_idx.data_ptr(), offs, d192.data_ptr(), d96.data_ptr())
        ok, st = agg()
        assert ok and st == bytes(k)
        assert np.array_equal(d192.cpu().numpy(), want), "aggregates differ from the signer's"
        nb, nc = min(k, PARENT_GROUPS_MAX), min(k, CPU_GROUPS_MAX)
        assert d96.cpu().numpy()[:nb].tobytes() == co.compress_sets(b"".join(bytes(128) + want[g].tobytes() for g in range(nb)))[2]
        row["a_aggregate_signature_sets_ms"] = ms_per_call(agg, 5)
        # (b) one device call per group, (c) the host: a prefix of the groups, scaled
        d_lists = [d_table[torch.from_numpy(idx[offsets[g]:offsets[g + 1]]).cuda()].contiguous() for g in range(nb)]
        out = ctypes.create_string_buffer(288)

        def parent():
            for g in range(nb):
                m._check(L.mi355_bls_g2_aggregate_device(c._h, d_lists[g].data_ptr(), int(lengths[g]), None, out))
        t = ms_per_call(parent, 2)
        row["b_one_call_per_group"] = {"measured_groups": nb, "measured_ms": t, "scaled_to_k_ms": round(t["median"] * k / nb, 1), "scaled": nb != k}
        lists = [table[idx[offsets[g]:offsets[g + 1]]].tobytes() for g in range(nc)]
        with ThreadPool(CPU_THREADS) as pool:
            assert pool.map(co.g2_sum, lists[:64]) == [want[g].tobytes() for g in range(min(64, nc))]
            t = ms_per_call(lambda: pool.map(co.g2_sum, lists), 3)
        row["c_cpu_g2_sum_16_threads"] = {"measured_groups": nc, "measured_ms": t, "scaled_to_k_ms": round(t["median"] * k / nc, 1), "scaled": nc != k}
        a = row["a_aggregate_signature_sets_ms"]
        row["one_call_per_group_over_aggregate"] = round(row["b_one_call_per_group"]["scaled_to_k_ms"] / a["median"], 1)
        row["cpu_16_threads_over_aggregate"] = round(row["c_cpu_g2_sum_16_threads"]["scaled_to_k_ms"] / a["median"], 2)
        row["beats_one_call_per_group_beyond_spread"] = row["b_one_call_per_group"]["scaled_to_k_ms"] > a["max"] + (a["max"] - a["min"])
        rows.append(row)
        del d_idx, d192, d96, d_lists
    return rows


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_aggsigs: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_signatures_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--ks", default=",".join(str(k) for k in KS), help="the k values to run, comma separated")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = []
    for k in (int(x) for x in a.ks.split(",")):
        rows += child(str(k), 420)
    res = {"how": "ms per blocking call, host clock: median, min and max of 5 calls after a warm-up (b: of 2, c: of 3) - min .. max is the run-to-run "
                  "spread; b and c are measured on a prefix of the groups and scaled linearly to k where `scaled` is true; level 0 at AGG_C = 8 "
                  "signatures per item, no other count tried",
           "rows": rows,
           "every_row_beats_one_call_per_group": all(r["beats_one_call_per_group_beyond_spread"] for r in rows)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
