#!/usr/bin/env python3
"""Stand-alone benchmark of the threshold-signature recovery (mi355_bls_recover_signature_sets_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_recover.py [--out profiles/recover_signatures_bench.json]

Every GPU step (one per k) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs: up to 4 096
validators per group size t, each key split t-of-t by a polynomial over Fr (host side, Python integers) with random 255-bit ids; the device
signer signs every share and every whole key.  A call of k groups addresses those shares through a resident index array, so every recovered
signature is compared byte for byte with the whole key's own signature before anything is timed.  Times are host-clock medians around
blocking calls (each ends in a stream synchronise), after one warm-up call; min and max of the same calls are the run-to-run spread.
Rows per k x t:
  (a) recover_signature_sets_device alone, the 192-byte output, everything resident;
  (b) the same call's kernels by torch.profiler: k_recover_mul, the sums (k_combsets_g2_sum), k_recover_finish (null when the profiler
      does not see them);
  (c) the route available before this call: coefficients on the host (Python integers, timed too), then one
      mi355_bls_p2s_mult_pippenger_device call per group; timed on at most 256 groups and SCALED to k;
  (d) the device signer over k t lanes (mi355_bls_sign_sets_device: k_sign_pk and k_sign_sig) and k_sign_sig's own kernel time from the
      profiler: its bit-serial 255-bit G2 multiplication (with a hash-to-G2 in front) is the only same-box yardstick for k_recover_mul's
      windowed one."""
import argparse
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KS = (1, 256, 16384, 65536)
TS = (3, 5, 7)
DISTINCT_MAX, PARENT_GROUPS_MAX = 4096, 256
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


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


def kernel_ms(fn, names):
    """device time in ms of the kernels whose name holds one of `names` during one call of fn, by torch.profiler; None where it sees none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
        out = {}
        for ev in prof.key_averages():
            for n in names:
                if n in ev.key:
                    t = getattr(ev, "device_time_total", None)
                    if t is None:
                        t = getattr(ev, "cuda_time_total", 0)
                    out[n] = round(out.get(n, 0.0) + t / 1e3, 3)
        return out or None
    except Exception as e:                                                   # a profiler that is not there is not a benchmark failure
        return {"error": repr(e)}


def coefficients(ids):
    xs = [x % R for x in ids]
    a = 1
    for x in xs:
        a = a * x % R
    out = []
    for i, xi in enumerate(xs):
        b = xi
        for j, x in enumerate(xs):
            if j != i:
                b = b * (x - xi) % R
        out.append(a * pow(b, R - 2, R) % R)
    return out


def step(k):
    import numpy as np
    import torch
    m = load()
    rows = []
    for t in TS:
        G = min(k, DISTINCT_MAX)
        c = m.BatchedBLSVerifierCache.init(max_sets=max(G * (t + 1), 64), numThreads=4096)
        rng = random.Random(20261018 + t)
        sks, ids, masters = [], [], []
        for g in range(G):
            cfs = [rng.randrange(1, R) for _ in range(t)]
            xs = [rng.getrandbits(255) for _ in range(t)]
            for x in xs:
                y = 0
                for cf in reversed(cfs):
                    y = (y * x + cf) % R
                sks.append(y.to_bytes(32, "little"))
                ids.append(x)
            masters.append(cfs[0].to_bytes(32, "little"))
        msgs = [hashlib.sha256(b"bench recover %d" % g).digest() for g in range(G)]
        n = G * t
        sk_all, msg_all = b"".join(sks + masters), b"".join([msgs[g] for g in range(G) for _ in range(t)] + msgs)
        ok, rec, _ = m.signSets(c, sk_all, msg_all)
        assert ok
        rec = np.frombuffer(rec, dtype=np.uint8).reshape(n + G, 320)
        table, whole = np.ascontiguousarray(rec[:n, 128:]), np.ascontiguousarray(rec[n:, 128:])
        reps = (k + G - 1) // G
        idx = np.tile(np.arange(n, dtype=np.int32), reps)[:k * t]
        idb = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in ids), dtype=np.uint8)
        d_table, d_idx = torch.from_numpy(table).cuda(), torch.from_numpy(idx).cuda()
        d_ids = torch.from_numpy(np.tile(idb, reps)[:k * t * 32].copy()).cuda()
        d192 = torch.zeros((k, 192), dtype=torch.uint8, device="cuda")
        offs = list(range(0, k * t + 1, t))
        row = {"k": k, "t": t, "members": k * t}

        def rec_call():
            return m.recoverSignatureSets_device(c, d_table.data_ptr(), n, d_idx.data_ptr(), offs, d_ids.data_ptr(), d192.data_ptr(), None)
        ok, st = rec_call()
        assert ok and st == bytes(k)
        assert np.array_equal(d192.cpu().numpy(), np.tile(whole, (reps, 1))[:k]), "recovered signatures differ from the whole keys' own"
        row["a_recover_signature_sets_ms"] = ms_per_call(rec_call, 5)
        row["b_kernels_ms"] = kernel_ms(rec_call, ("k_recover_mul", "k_combsets_g2_sum", "k_recover_finish"))
        # (c) host coefficients + one Pippenger call per group, on a prefix of the groups, scaled
        nb = min(k, PARENT_GROUPS_MAX)
        t0 = time.perf_counter()
        coef = [coefficients(ids[(g % G) * t:(g % G) * t + t]) for g in range(nb)]
        host_ms = (time.perf_counter() - t0) * 1e3
        d_pts = [d_table[(g % G) * t:(g % G) * t + t].contiguous() for g in range(nb)]
        d_sc = [torch.from_numpy(np.frombuffer(b"".join(x.to_bytes(32, "little") for x in cs), dtype=np.uint8).copy()).cuda() for cs in coef]

        def parent():
            for g in range(nb):
                m.p2s_mult_pippenger_device(c, d_pts[g].data_ptr(), t, d_sc[g].data_ptr())
        tm = ms_per_call(parent, 2)
        row["c_one_pippenger_call_per_group"] = {"measured_groups": nb, "measured_ms": tm, "host_coefficients_ms": round(host_ms, 3),
                                                 "scaled_to_k_ms": round((tm["median"] + host_ms) * k / nb, 1), "scaled": nb != k}
        # (d) the bit-serial signer over the same number of lanes
        lanes = k * t
        sk_l = np.frombuffer(sk_all, dtype=np.uint8).reshape(-1, 32)
        ms_l = np.frombuffer(msg_all, dtype=np.uint8).reshape(-1, 32)
        pick = np.arange(lanes) % n
        d_sk, d_ms = torch.from_numpy(sk_l[pick].copy()).cuda(), torch.from_numpy(ms_l[pick].copy()).cuda()
        d_out = torch.zeros((lanes, 320), dtype=torch.uint8, device="cuda")
        big = c if lanes <= G * (t + 1) else m.BatchedBLSVerifierCache.init(max_sets=lanes, numThreads=4096)

        def signer():
            return m.signSets_device(big, d_sk.data_ptr(), d_ms.data_ptr(), lanes, d_out.data_ptr())
        row["d_sign_sets_device_ms"] = ms_per_call(signer, 2)
        row["d_kernels_ms"] = kernel_ms(signer, ("k_sign_sig", "k_sign_pk"))
        a = row["a_recover_signature_sets_ms"]
        row["one_call_per_group_over_recover"] = round(row["c_one_pippenger_call_per_group"]["scaled_to_k_ms"] / a["median"], 1)
        row["beats_one_call_per_group_beyond_spread"] = row["c_one_pippenger_call_per_group"]["scaled_to_k_ms"] > a["max"] + (a["max"] - a["min"])
        rows.append(row)
        if big is not c:
            big.close()
        c.close()
        del d_table, d_idx, d_ids, d192, d_pts, d_sc, d_sk, d_ms, d_out
    return rows


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_recover: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_signatures_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--ks", default=",".join(str(k) for k in KS), help="the k values to run, comma separated")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = []
    for k in (int(x) for x in a.ks.split(",")):
        rows += child(str(k), 420)
    res = {"how": "ms per blocking call, host clock: median, min and max of 5 calls after a warm-up (c, d: of 2) - min .. max is the run-to-run spread; "
                  "c is measured on a prefix of the groups, host coefficients included, and scaled linearly to k where `scaled` is true; the kernel "
                  "rows are device times of one call by torch.profiler",
           "rows": rows,
           "every_row_beats_one_call_per_group": all(r["beats_one_call_per_group_beyond_spread"] for r in rows)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
