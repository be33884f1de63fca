#!/usr/bin/env python3
"""Stand-alone benchmark of the key-table calls (mi355_bls_deserialize_public_keys, mi355_bls_admit_keys) beside the routes a caller had
before them; bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_key_table.py [--sizes 4096,65536,1048576] [--out profiles/key_table_bench.json]

Every size runs in a child process of its own under `timeout`.  In ONE process, on one context (capacity min(n, 65536): larger tables run in
slices), with the inputs resident in device memory: n keys and proofs from the device prover (popProve), compressed on the device
(compressPublicKeys, compressSignatures).  Per call: median, min and max of 5 blocking calls after a warm-up call, in ms.

  (a) deserialize_public_keys over the n keys, and deserialize_sets_ex_device over the same keys with one valid signature repeated in
      every row and zero messages - the only device decoder of a key before this call.  Same run, same context.
  (b) admit_keys on the all-valid table; on the same table with 1 % of the keys replaced by an undecodable encoding; and the three-call
      sequence a caller writes without it on both tables: deserialize_sets_ex_device over keys and proofs (records to the host), the host
      glue that splits the records into the key and the proof column and sends them back, batch_pop_verify_locate_device.  On the 1 % table
      the zeroed rows fail the blinded batch, so that sequence takes the per-pair pass over every row.  The parts are reported beside the sum.
  (c) a CPU row only if oracle/bls_oracle.c has a key decoder of its own: it has none (its one decoder, oracle_deserialize_sets_ex, takes
      tuples and decodes a signature beside every key), and the file says so instead of inventing one.

checks: (i) deserialize_public_keys is no slower than deserialize_sets_device beyond the run's own min..max spread; (ii) admit_keys on the 1 %
table is faster than the three-call sequence.  Both are reported as they come out, never asserted."""
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
CAPACITY = 65536


def load():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.load_package()


def timed(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def step(n):
    import numpy as np
    import torch
    m = load()
    L = m.lib()
    c = m.BatchedBLSVerifierCache.init(max_sets=max(min(n, CAPACITY), 64), numThreads=4096)

    def dev(b):
        t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        return t

    def empty(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    sks = b"".join(hashlib.sha256(b"bench key table sk %d" % i).digest()[:31] + b"\x00" for i in range(n))
    d_sk, d_pk96, d_pr192, d_pk48, d_pr96 = dev(sks), empty(96 * n), empty(192 * n), empty(48 * n), empty(96 * n)
    ok, st = m.popProve_device(c, d_sk.data_ptr(), n, d_pk96.data_ptr(), d_pr192.data_ptr())
    assert ok and st == bytes(n)
    m.compressPublicKeys_device(c, d_pk96.data_ptr(), n, d_pk48.data_ptr())
    m.compressSignatures_device(c, d_pr192.data_ptr(), n, d_pr96.data_ptr())
    torch.cuda.synchronize()
    rnd = hashlib.sha256(b"bench key table rnd").digest()
    r = {"n": n, "capacity": max(min(n, CAPACITY), 64)}

    # (a) the key decoder beside the tuple decoder over the same keys
    d_tab, d_msgs = empty(96 * n), empty(32 * n)
    d_sig_rep = d_pr96[:96].repeat(n)
    status = ctypes.create_string_buffer(n)
    torch.cuda.synchronize()
    assert m.deserializePublicKeys_device(c, d_pk48.data_ptr(), n, d_tab.data_ptr()) == (True, bytes(n))
    assert torch.equal(d_tab, d_pk96)
    r["deserialize_public_keys"] = timed(lambda: m.deserializePublicKeys_device(c, d_pk48.data_ptr(), n, d_tab.data_ptr()))

    def deser_sets(d_keys, d_sigs, out=None):
        rc = L.mi355_bls_deserialize_sets_ex_device(c._h, d_keys.data_ptr(), d_msgs.data_ptr(), d_sigs.data_ptr(), n, 0, None, out, status)
        assert rc >= 0
        return rc

    assert deser_sets(d_pk48, d_sig_rep) == 1
    r["deserialize_sets_device_same_keys"] = timed(lambda: deser_sets(d_pk48, d_sig_rep))

    # (b) admission: all valid, then 1 % undecodable, against the three calls of before
    bad = np.arange(50, n, 100)
    keys1 = d_pk48.clone().view(n, 48)
    keys1[torch.from_numpy(bad).cuda()] = 0                         # 48 zero bytes: the compressed bit is not set
    keys1 = keys1.view(-1).contiguous()
    torch.cuda.synchronize()
    want1 = bytearray(n)
    for i in bad:
        want1[i] = 1
    assert m.admitKeys_device(c, d_pk48.data_ptr(), d_pr96.data_ptr(), n, rnd, d_tab.data_ptr()) == (True, bytes(n))
    assert torch.equal(d_tab, d_pk96)
    passes = m.verifyEachPasses(c)
    assert m.admitKeys_device(c, keys1.data_ptr(), d_pr96.data_ptr(), n, rnd, d_tab.data_ptr()) == (False, bytes(want1))
    assert m.verifyEachPasses(c) == passes                             # the survivors passed as a batch
    r["admit_keys_all_valid"] = timed(lambda: m.admitKeys_device(c, d_pk48.data_ptr(), d_pr96.data_ptr(), n, rnd, d_tab.data_ptr()))
    r["admit_keys_1pct_undecodable"] = timed(lambda: m.admitKeys_device(c, keys1.data_ptr(), d_pr96.data_ptr(), n, rnd, d_tab.data_ptr()))

    rec = np.empty(320 * n, dtype=np.uint8)
    parts = {}

    def three_calls(d_keys, tag, expect_ok):
        t0 = time.perf_counter()
        deser_sets(d_keys, d_pr96, rec.ctypes.data)
        t1 = time.perf_counter()
        rows = rec.reshape(n, 320)
        dk, dp = torch.from_numpy(np.ascontiguousarray(rows[:, :96])).cuda(), torch.from_numpy(np.ascontiguousarray(rows[:, 128:])).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ok, v = m.batchPopVerifyLocate_device(c, dk.data_ptr(), dp.data_ptr(), n, rnd)
        t3 = time.perf_counter()
        assert ok is expect_ok and (expect_ok or sum(1 for x in v if not x) == len(bad))
        parts.setdefault(tag, []).append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))

    for tag, d_keys, expect in (("three_calls_all_valid", d_pk48, True), ("three_calls_1pct_undecodable", keys1, False)):
        row = timed(lambda: three_calls(d_keys, tag, expect))
        last = parts[tag][1:]                                          # without the warm-up call
        for k, name in enumerate(("deserialize_sets_ex_ms", "host_glue_ms", "batch_pop_verify_locate_ms")):
            row[name] = round(statistics.median(p[k] for p in last), 3)
        r[tag] = row
    assert m.verifyEachPasses(c) > passes                              # the 1 % table sent that sequence to the per-pair pass
    a, b = r["deserialize_public_keys"], r["deserialize_sets_device_same_keys"]
    r["check_i_decoder_no_slower"] = bool(a["ms"] <= b["ms"] + max(a["max"] - a["min"], b["max"] - b["min"]))
    r["ratio_deserialize_public_keys_over_sets"] = round(a["ms"] / b["ms"], 3)
    r["check_ii_admit_faster_on_1pct"] = bool(r["admit_keys_1pct_undecodable"]["ms"] < r["three_calls_1pct_undecodable"]["ms"])
    r["ratio_admit_over_three_calls_1pct"] = round(r["admit_keys_1pct_undecodable"]["ms"] / r["three_calls_1pct_undecodable"]["ms"], 3)
    r["ratio_admit_over_device_parts_1pct"] = round(r["admit_keys_1pct_undecodable"]["ms"] / (r["three_calls_1pct_undecodable"]["deserialize_sets_ex_ms"]
                                                                                              + r["three_calls_1pct_undecodable"]["batch_pop_verify_locate_ms"]), 3)
    c.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_table_bench.json"))
    ap.add_argument("--step", type=int, default=0)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    res = {"comment": "nim-blscurve_amd/tools/bench_key_table.py: ms per blocking call, median / min / max of 5 after a warm-up call, inputs resident in "
                      "device memory, one MI355X",
           "cpu": {"measured": False, "reason": "oracle/bls_oracle.c has no key decoder of its own (oracle_deserialize_sets_ex decodes a signature beside "
                                                "every key), so there is no CPU row"},
           "sizes": {}}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        limit = 120 if n <= 4096 else 240 if n <= 65536 else 480
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(n)], stdout=subprocess.PIPE)
        if p.returncode != 0:
            sys.exit("bench_key_table: the GPU step for n = %d failed with exit status %d" % (n, p.returncode))      # nothing more is started on the GPU
        res["sizes"][str(n)] = json.loads(p.stdout.decode().strip().splitlines()[-1])
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
