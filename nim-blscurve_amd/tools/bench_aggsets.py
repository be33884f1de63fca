#!/usr/bin/env python3
"""Stand-alone benchmark of the per-set key aggregation (mi355_bls_aggregate_sets_device, mi355_bls_batch_fast_aggregate_verify_device);
bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_aggsets.py [--out profiles/aggregate_sets_bench.json]

Every GPU step (one per k) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs: a table of
65 536 keys from the device signer (50-bit secret keys, so that a committee's secret sum fits 64 bits), committees drawn by a seeded RNG with
lengths uniform in [mean / 2, 3 mean / 2], one message per committee and the committee's aggregate signature from the device signer.  Every
aggregated record is compared byte for byte with the signer's record of the secret sum before anything is timed.  Times are host-clock
medians around blocking calls (each ends in a stream synchronise), after one warm-up call.  Rows per k x mean committee size:
  (a) aggregate_sets_device alone, keys through an index array into the resident table, and as one contiguous key array (skipped where
      that array would exceed 2 GiB);
  (b) the only route before this call, one mi355_bls_fast_aggregate_verify per set: timed on at most 256 sets and SCALED to k;
  (c) c_oracle.g1_sum per set on 16 host threads: timed on at most 2 048 sets and SCALED to k;
  (d) batch_fast_aggregate_verify_device end to end beside batchVerify (device form) on the k finished records."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KS = (64, 4096, 65536)
MEANS = (16, 128, 512)
TABLE = 65536
CONTIGUOUS_MAX_BYTES = 2 << 30
PARENT_SETS_MAX, CPU_SETS_MAX, CPU_THREADS = 256, 2048, 16


def load():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    return ge.load_package()


def ms_per_call(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3)


def sign(m, cache, sks, tag):
    """records of the device signer for 64-bit secret keys (numpy uint64) and messages derived from tag"""
    import numpy as np
    n = len(sks)
    sk32 = np.zeros((n, 32), dtype=np.uint8)
    sk32[:, :8] = sks.astype("<u8").view(np.uint8).reshape(n, 8)
    msgs = b"".join(hashlib.sha256(b"bench aggsets %s %d" % (tag, i)).digest() for i in range(n))
    ok, rec, _ = m.signSets(cache, sk32.tobytes(), msgs)
    assert ok
    return np.frombuffer(rec, dtype=np.uint8).reshape(n, 320)


def step(k):
    import numpy as np
    import torch
    from multiprocessing.pool import ThreadPool
    m = load()
    import c_oracle as co
    c = m.BatchedBLSVerifierCache.init(max_sets=max(k, 64), numThreads=4096)
    big = c if k >= TABLE else m.BatchedBLSVerifierCache.init(max_sets=TABLE, numThreads=4096)
    rng = np.random.default_rng(20261017)
    sks = rng.integers(1, 1 << 50, size=TABLE, dtype=np.uint64)
    table = np.ascontiguousarray(sign(m, big, sks, b"table")[:, :96])
    d_table = torch.from_numpy(table).cuda()
    rnd = hashlib.sha256(b"bench aggsets rnd").digest()
    rows = []
    for mean in MEANS:
        lengths = rng.integers(mean // 2, mean + mean // 2 + 1, size=k)
        offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
        n_keys = int(offsets[-1])
        idx = rng.integers(0, TABLE, size=n_keys, dtype=np.int64)
        sums = np.add.reduceat(sks[idx], offsets[:-1])                       # < 2^50 * 768: no wrap
        want = sign(m, c, sums, b"k%d mean%d" % (k, mean))
        d_idx = torch.from_numpy(idx.astype(np.int32)).cuda()
        d_msgs = torch.from_numpy(np.ascontiguousarray(want[:, 96:128])).cuda()
        d_sigs = torch.from_numpy(np.ascontiguousarray(want[:, 128:])).cuda()
        d_out = torch.zeros((k, 320), dtype=torch.uint8, device="cuda")
        offs = [int(x) for x in offsets]
        row = {"k": k, "mean_committee": mean, "keys": n_keys}

        def agg_indexed():
            return m.aggregateSets_device(c, d_table.data_ptr(), TABLE, d_idx.data_ptr(), offs, d_msgs.data_ptr(), d_sigs.data_ptr(), d_out.data_ptr())
        ok, st = agg_indexed()
        assert ok and st == bytes(k)
        assert np.array_equal(d_out.cpu().numpy(), want), "aggregated records differ from the signer's"
        row["a_aggregate_indexed_ms"] = ms_per_call(agg_indexed, 5)
        if n_keys * 96 <= CONTIGUOUS_MAX_BYTES:
            d_keys = d_table[torch.from_numpy(idx).cuda()].contiguous()

            def agg_contiguous():
                return m.aggregateSets_device(c, d_keys.data_ptr(), n_keys, None, offs, d_msgs.data_ptr(), d_sigs.data_ptr(), d_out.data_ptr())
            d_out.zero_()
            ok, st = agg_contiguous()
            assert ok and np.array_equal(d_out.cpu().numpy(), want)
            row["a_aggregate_contiguous_ms"] = ms_per_call(agg_contiguous, 5)
            del d_keys
        else:
            row["a_aggregate_contiguous_ms"] = None                          # the key array alone would exceed CONTIGUOUS_MAX_BYTES
        # (d) end to end beside the plain batch pass on the finished records
        assert m.batchFastAggregateVerify_device(c, d_table.data_ptr(), TABLE, d_idx.data_ptr(), offs, d_msgs.data_ptr(), d_sigs.data_ptr(), rnd) is True
        row["d_batch_fast_aggregate_verify_ms"] = ms_per_call(
            lambda: m.batchFastAggregateVerify_device(c, d_table.data_ptr(), TABLE, d_idx.data_ptr(), offs, d_msgs.data_ptr(), d_sigs.data_ptr(), rnd), 5)
        assert c.verify_device(d_out.data_ptr(), k, rnd) is True
        row["d_batch_verify_ms"] = ms_per_call(lambda: c.verify_device(d_out.data_ptr(), k, rnd), 5)
        # (b) one device call per set, (c) the host: a prefix of the sets, scaled
        nb, nc = min(k, PARENT_SETS_MAX), min(k, CPU_SETS_MAX)
        lists = [table[idx[offsets[s]:offsets[s + 1]]].tobytes() for s in range(nc)]
        msg_b, sig_b = [want[s, 96:128].tobytes() for s in range(nb)], [want[s, 128:].tobytes() for s in range(nb)]

        def parent():
            return [m.fastAggregateVerify(c, lists[s], msg_b[s], sig_b[s]) for s in range(nb)]
        assert all(parent())
        t = ms_per_call(parent, 2)
        row["b_one_call_per_set"] = {"measured_sets": nb, "measured_ms": t, "scaled_to_k_ms": round(t * k / nb, 1), "scaled": nb != k}
        co.g1_sum(lists[0])
        with ThreadPool(CPU_THREADS) as pool:
            assert pool.map(co.g1_sum, lists[:64]) == [want[s, :96].tobytes() for s in range(min(64, nc))]
            t = ms_per_call(lambda: pool.map(co.g1_sum, lists), 3)
        row["c_cpu_g1_sum_16_threads"] = {"measured_sets": nc, "measured_ms": t, "scaled_to_k_ms": round(t * k / nc, 1), "scaled": nc != k}
        rows.append(row)
        del d_idx, d_msgs, d_sigs, d_out
    return rows


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_aggsets: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_sets_bench.json"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = []
    for k in KS:
        rows += child(str(k), 420)
    res = {"how": "ms per blocking call, host clock, median of 5 after a warm-up (b: of 2, c: of 3); b and c are measured on a prefix of the sets and "
                  "scaled linearly to k where `scaled` is true; a_aggregate_contiguous_ms null: the contiguous key array would exceed 2 GiB",
           "rows": rows}
    at = [r for r in rows if r["k"] == 65536 and r["mean_committee"] == 128]
    if at:
        r = at[0]
        res["at_65536x128"] = {"aggregate_ms": r["a_aggregate_indexed_ms"], "batch_verify_ms": r["d_batch_verify_ms"],
                               "one_call_per_set_over_aggregate": round(r["b_one_call_per_set"]["scaled_to_k_ms"] / r["a_aggregate_indexed_ms"], 1),
                               "cpu_16_threads_over_aggregate": round(r["c_cpu_g1_sum_16_threads"]["scaled_to_k_ms"] / r["a_aggregate_indexed_ms"], 2)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
