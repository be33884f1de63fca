#!/usr/bin/env python3
"""Stand-alone benchmark of batchVerify by message (mi355_bls_batch_verify_by_message_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_by_message.py [--out profiles/by_message_bench.json]

Every GPU step (one per group size) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs:
65 536 members from the device signer, in groups of L = 1, 2, 4, 16, 64 or 512 members that share a message (consecutive members, as
combine_sets takes them).  Everything is device-resident; times are host-clock medians of 5 blocking calls after one warm-up call.  Per
group size, over the same sets on the same context in the same process:
  by_message_ms   mi355_bls_batch_verify_by_message_device (groups found on the device);
  plain_ms        mi355_bls_batch_verify_device, the pass that repeats the per-pair work for every set;
  combined_ms     mi355_bls_batch_verify_combined_device with the offsets the layout gives (its host grouping is NOT timed: the sets are
                  already in group order, which flatters it).
The three verdicts must be true, and the by-message call's final value must equal the plain call's, before anything is timed.  No
acceptance number: the two existing calls are the yardsticks."""
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
GROUP_SIZES = (1, 2, 4, 16, 64, 512)


def load():
    sys.path.insert(0, ROOT)
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
    m = load()
    n, k = MEMBERS, MEMBERS // L
    c = m.BatchedBLSVerifierCache.init(max_sets=n, numThreads=4096)
    rng = np.random.default_rng(20261019)
    sk32 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sk32[:, 31] &= 0x3f
    sk32[:, 0] |= 1
    msgs = b"".join(hashlib.sha256(b"bench by message %d %d" % (L, g)).digest() * L for g in range(k))
    ok, rec, _ = m.signSets(c, sk32.tobytes(), msgs)
    assert ok
    d_sets = torch.from_numpy(np.frombuffer(rec, dtype=np.uint8).reshape(n, 320).copy()).cuda()
    offs = [g * L for g in range(k + 1)]
    rnds = b"".join(hashlib.sha256(b"bench by message rnd %d" % g).digest() for g in range(k))
    rnd = hashlib.sha256(b"bench by message batch").digest()
    row = {"group_size": L, "groups": k, "members": n}

    def by_message():
        return m.batchVerifyByMessage_device(c, d_sets.data_ptr(), n, rnd)

    def plain():
        return c.verify_device(d_sets.data_ptr(), n, rnd)

    def combined():
        return m.batchVerifyCombined_device(c, d_sets.data_ptr(), n, None, offs, rnds, rnd)

    assert by_message() is True and m.lastMessageGroups(c) == k
    gt = c.fetch(4, 576)
    assert plain() is True and c.fetch(4, 576) == gt, "the by-message call's final value differs from batch_verify's"
    assert combined() is True
    row["by_message_ms"] = ms_per_call(by_message, 5)
    row["by_message_stage_ms"] = {s: round(v, 3) for s, v in c.timings().items()}
    row["plain_ms"] = ms_per_call(plain, 5)
    row["combined_ms"] = ms_per_call(combined, 5)
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_by_message: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "by_message_bench.json"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = [child(str(L), 240) for L in GROUP_SIZES]
    res = {"how": "ms per blocking call, host clock, median of 5 after a warm-up; 65 536 device-resident sets from the device signer in groups of "
                  "`group_size` consecutive members that share a message; the three calls run over the same sets on one context in one process "
                  "(combined: the host grouping it needs is not timed)",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
