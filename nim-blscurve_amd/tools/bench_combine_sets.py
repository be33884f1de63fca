#!/usr/bin/env python3
"""Stand-alone benchmark of the same-message pre-aggregation (mi355_bls_combine_sets_device, mi355_bls_batch_verify_combined_device);
bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_combine_sets.py [--out profiles/combine_sets_bench.json]

Every GPU step (one per group size) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs:
65 536 members from the device signer, cut into groups of 2, 4, 16, 64 or 512 members that share a message.  The combined records of a
sample of groups (the first eight and the last) are compared byte for byte with c_oracle.combine before anything is timed.  Times are
host-clock medians around blocking calls (each ends in a stream synchronise), after one warm-up call.  Rows per group size:
  (a) combine_sets_device alone;
  (b) one mi355_bls_combine per group: timed on at most 256 groups and SCALED to k;
  (c) c_oracle.combine per group on 16 host threads: timed on groups of at most 4 096 members in all and SCALED to k;
  (d) batch_verify_combined_device end to end beside batch_verify_device over the n uncombined sets - the route a host takes today - on the
      same context in the same process.
`crossover_group_size`: the smallest measured group size from which (d)'s combined route is the faster one at every larger measured size
(null: at none); `combined_loses_at`: the measured group sizes at which it is slower."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MEMBERS = 65536
GROUP_SIZES = (2, 4, 16, 64, 512)
PARENT_GROUPS_MAX, CPU_MEMBERS_MAX, CPU_THREADS = 256, 4096, 16


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


def step(L):
    import numpy as np
    import torch
    from multiprocessing.pool import ThreadPool
    m = load()
    import c_oracle as co
    n, k = MEMBERS, MEMBERS // L
    c = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4096)
    rng = np.random.default_rng(20261017)
    sk32 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sk32[:, 31] &= 0x3f
    sk32[:, 0] |= 1
    msgs = b"".join(hashlib.sha256(b"bench combine sets %d %d" % (L, g)).digest() * L for g in range(k))
    ok, rec, _ = m.signSets(c, sk32.tobytes(), msgs)
    assert ok
    sets = np.frombuffer(rec, dtype=np.uint8).reshape(n, 320)
    d_sets = torch.from_numpy(sets.copy()).cuda()
    d_out = torch.zeros((k, 320), dtype=torch.uint8, device="cuda")
    offs = [g * L for g in range(k + 1)]
    rnds = b"".join(hashlib.sha256(b"bench combine sets rnd %d" % g).digest() for g in range(k))
    rnd = hashlib.sha256(b"bench combine sets batch").digest()
    row = {"group_size": L, "groups": k, "members": n}

    def pks_sigs(g):
        s = sets[g * L:(g + 1) * L]
        return np.ascontiguousarray(s[:, :96]).tobytes(), np.ascontiguousarray(s[:, 128:]).tobytes()

    def combine():
        return m.combineSets_device(c, d_sets.data_ptr(), n, None, offs, rnds, d_out.data_ptr())
    ok, st = combine()
    assert ok and st == bytes(k)
    got = d_out.cpu().numpy()
    for g in list(range(min(8, k))) + [k - 1]:
        pk, sg, _ = co.combine(rnds[32 * g:32 * g + 32], *pks_sigs(g))
        assert got[g].tobytes() == pk + sets[g * L, 96:128].tobytes() + sg, "combined record %d differs from c_oracle.combine" % g
    row["a_combine_sets_ms"] = ms_per_call(combine, 5)
    # (d) end to end beside the plain batch pass over the uncombined sets, same context
    assert m.batchVerifyCombined_device(c, d_sets.data_ptr(), n, None, offs, rnds, rnd) is True
    row["d_batch_verify_combined_ms"] = ms_per_call(lambda: m.batchVerifyCombined_device(c, d_sets.data_ptr(), n, None, offs, rnds, rnd), 5)
    assert c.verify_device(d_sets.data_ptr(), n, rnd) is True
    row["d_batch_verify_uncombined_ms"] = ms_per_call(lambda: c.verify_device(d_sets.data_ptr(), n, rnd), 5)
    assert c.verify_device(d_out.data_ptr(), k, rnd) is True
    row["d_batch_verify_of_k_records_ms"] = ms_per_call(lambda: c.verify_device(d_out.data_ptr(), k, rnd), 5)
    # (b) one device call per group, (c) the host: a prefix of the groups, scaled
    nb, nc = min(k, PARENT_GROUPS_MAX), max(1, min(k, CPU_MEMBERS_MAX // L))
    groups = [pks_sigs(g) for g in range(max(nb, nc))]
    L_ = m.lib()
    import ctypes
    out_pk, out_sig = ctypes.create_string_buffer(96), ctypes.create_string_buffer(192)

    def parent():
        for g in range(nb):
            assert L_.mi355_bls_combine(c._h, rnds[32 * g:32 * g + 32], groups[g][0], groups[g][1], L, out_pk, out_sig) == 0
    parent()
    assert out_pk.raw + out_sig.raw == got[nb - 1, :96].tobytes() + got[nb - 1, 128:].tobytes()
    t = ms_per_call(parent, 2)
    row["b_one_combine_per_group"] = {"measured_groups": nb, "measured_ms": t, "scaled_to_k_ms": round(t * k / nb, 1), "scaled": nb != k}

    def cpu_one(g):
        return co.combine(rnds[32 * g:32 * g + 32], *groups[g])[:2]
    with ThreadPool(CPU_THREADS) as pool:
        assert pool.map(cpu_one, range(min(4, nc))) == [(got[g, :96].tobytes(), got[g, 128:].tobytes()) for g in range(min(4, nc))]
        t = ms_per_call(lambda: pool.map(cpu_one, range(nc)), 3)
    row["c_cpu_combine_16_threads"] = {"measured_groups": nc, "measured_ms": t, "scaled_to_k_ms": round(t * k / nc, 1), "scaled": nc != k}
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_combine_sets: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_sets_bench.json"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = [child(str(L), 240) for L in GROUP_SIZES]
    wins = [r["d_batch_verify_combined_ms"] < r["d_batch_verify_uncombined_ms"] for r in rows]
    cross = None
    for i in range(len(rows) - 1, -1, -1):
        if not wins[i]:
            break
        cross = rows[i]["group_size"]
    res = {"how": "ms per blocking call, host clock, median of 5 after a warm-up (b: of 2, c: of 3); b and c are measured on a prefix of the groups and "
                  "scaled linearly to k where `scaled` is true; d compares batch_verify_combined_device with batch_verify_device over the same 65 536 "
                  "uncombined sets on one context",
           "rows": rows, "crossover_group_size": cross, "combined_loses_at": [r["group_size"] for r, w in zip(rows, wins) if not w]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
