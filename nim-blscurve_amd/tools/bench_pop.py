#!/usr/bin/env python3
"""Stand-alone benchmark of the proof-of-possession calls (mi355_bls_pop_verify_each, mi355_bls_batch_pop_verify) beside their ordinary
counterparts; bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_pop.py [--n 65536] [--out profiles/pop_verify_bench.json]

The GPU step runs in a child process of its own under `timeout`.  In ONE process, on one context: n keys and proofs from the device prover, and n
ordinary signed sets over the SAME keys from the device signer; then ms per blocking host-pointer call (median of 5 after a warm-up call) of
pop_verify_each, batch_pop_verify, verify_each and batch_verify, with the device time of the last call of each (HIP events) and, for the two batch
calls, the stage and per-kernel split.  The two ratios PoP / ordinary are the result: the PoP passes differ from the ordinary ones by the record
kernel (one pass over 320 n bytes) and by two field multiplications and a comparison per key in the hash-map kernel, against some 15 000 per set,
so each should land within 5 % of its counterpart."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.load_package()


def ms_per_call(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3)


def step(n):
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=max(n, 64), numThreads=4096)
    sks = b"".join(hashlib.sha256(b"bench pop sk %d" % i).digest()[:31] + b"\x00" for i in range(n))
    msgs = b"".join(hashlib.sha256(b"bench pop msg %d" % i).digest() for i in range(n))
    ok, pks, proofs, _ = m.popProve(c, sks)
    assert ok
    ok, rec, _ = m.signSets(c, sks, msgs)
    assert ok and all(rec[320 * i:320 * i + 96] == pks[96 * i:96 * i + 96] for i in range(0, n, max(1, n // 64)))      # the same keys
    rnd = hashlib.sha256(b"bench pop rnd").digest()
    assert all(m.popVerifyEach(c, pks, proofs)) and all(m.verifyEach(c, rec))
    assert m.batchPopVerify(c, pks, proofs, rnd) is True and m.batchVerify(c, rec, rnd) is True
    r = {"n": n}
    for name, fn, batch in (("pop_verify_each", lambda: m.popVerifyEach(c, pks, proofs), False), ("verify_each", lambda: m.verifyEach(c, rec), False),
                            ("batch_pop_verify", lambda: m.batchPopVerify(c, pks, proofs, rnd), True), ("batch_verify", lambda: m.batchVerify(c, rec, rnd), True)):
        row = {"ms": ms_per_call(fn), "device_ms": round(c.timings()["total"], 3)}
        if batch:
            row["stage_ms"] = {k: round(v, 3) for k, v in c.timings().items()}
            row["kernel_ms"] = {k: round(v, 3) for k, v in c.kernel_timings().items()}
        r[name] = row
    r["ratio_pop_verify_each_over_verify_each"] = round(r["pop_verify_each"]["ms"] / r["verify_each"]["ms"], 3)
    r["ratio_batch_pop_verify_over_batch_verify"] = round(r["batch_pop_verify"]["ms"] / r["batch_verify"]["ms"], 3)
    r["device_ratio_pop_verify_each_over_verify_each"] = round(r["pop_verify_each"]["device_ms"] / r["verify_each"]["device_ms"], 3)
    r["device_ratio_batch_pop_verify_over_batch_verify"] = round(r["batch_pop_verify"]["device_ms"] / r["batch_verify"]["device_ms"], 3)
    c.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pop_verify_bench.json"))
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.n)))
        return
    p = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", "--n", str(a.n)], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_pop: the GPU step failed with exit status %d" % p.returncode)
    res = json.loads(p.stdout.decode().strip().splitlines()[-1])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
