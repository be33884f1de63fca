#!/usr/bin/env python3
"""Stand-alone benchmark of the key aggregation by participation bits (mi355_bls_aggregate_sets_bits_device,
mi355_bls_batch_fast_aggregate_verify_bits_device); bench.py stays the flagship's.

  python nim-blscurve_amd/tools/bench_aggbits.py [--out profiles/aggregate_bits_bench.json]

Every GPU step (one per shape) runs in a child process of its own under `timeout`; the first step that fails ends the run.  Inputs: a
table of 65 536 keys from the device signer (50-bit secret keys, so that a set's secret sum fits 64 bits), 64 committees of the shape's size
drawn by a seeded RNG as index lists into the table, k sets that name the committees in turn, every bit drawn with the shape's
participation.  The yardstick is mi355_bls_aggregate_sets_device over the expanded index lists of the same sets - the only route before
this call - measured in the same process; every record of the new call, with and without the committees' aggregates, is compared byte for
byte with the yardstick's before anything is timed.  Everything is device-resident.  Times are host-clock medians of 5 blocking calls (each
ends in a stream synchronise) after one warm-up call, with min .. max.  Shapes marked `verify` also time
batch_fast_aggregate_verify_bits_device end to end beside batch_fast_aggregate_verify_device, with signatures of the device signer.
staged_bytes: what the host forms of the two calls would copy to the device for the shape."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {  # name: (sets, committee size, participation in percent, also the verification end to end)
    "65536x128_p50": (65536, 128, 50, False), "65536x128_p95": (65536, 128, 95, True), "65536x128_p99": (65536, 128, 99, False),
    "65536x512_p99": (65536, 512, 99, False), "4096x128_p95": (4096, 128, 95, True), "64x128_p95": (64, 128, 95, False)}
TABLE, COMMITTEES = 65536, 64


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


def sign(m, cache, sks, tag):
    """records of the device signer for 64-bit secret keys (numpy uint64) and messages derived from tag"""
    import numpy as np
    n = len(sks)
    sk32 = np.zeros((n, 32), dtype=np.uint8)
    sk32[:, :8] = sks.astype("<u8").view(np.uint8).reshape(n, 8)
    msgs = b"".join(hashlib.sha256(b"bench aggbits %s %d" % (tag, i)).digest() for i in range(n))
    ok, rec, _ = m.signSets(cache, sk32.tobytes(), msgs)
    assert ok
    return np.frombuffer(rec, dtype=np.uint8).reshape(n, 320)


def step(name):
    import numpy as np
    import torch
    k, L, pct, verify = SHAPES[name]
    m = load()
    c = m.BatchedBLSVerifierCache.init(max_sets=TABLE, numThreads=4096)
    rng = np.random.default_rng(20261019)
    sks = rng.integers(1, 1 << 50, size=TABLE, dtype=np.uint64)
    d_table = torch.from_numpy(np.ascontiguousarray(sign(m, c, sks, b"table")[:, :96])).cuda()
    c_idx = rng.integers(0, TABLE, size=(COMMITTEES, L), dtype=np.int64)
    c_offsets = [L * i for i in range(COMMITTEES + 1)]
    which = np.arange(k) % COMMITTEES
    flags = rng.integers(0, 100, size=(k, L)) < pct
    flags[~flags.any(axis=1), 0] = True
    bits = np.packbits(flags, axis=1, bitorder="little")                        # SSZ order; L is a multiple of 8
    members = c_idx[which]                                                      # k x L table indices
    idx = members[flags]                                                        # the expanded lists, set after set
    offs = [int(x) for x in np.concatenate(([0], np.cumsum(flags.sum(axis=1))))]
    if verify:
        sums = (sks[members] * flags).sum(axis=1, dtype=np.uint64)
        rec = sign(m, c, sums, name.encode())
        msgs, sigs = np.ascontiguousarray(rec[:, 96:128]), np.ascontiguousarray(rec[:, 128:])
    else:
        msgs, sigs = np.zeros((k, 32), dtype=np.uint8), np.zeros((k, 192), dtype=np.uint8)
    d_cidx, d_idx = torch.from_numpy(c_idx.astype(np.int32).reshape(-1)).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda()
    d_bits, d_msgs, d_sigs = torch.from_numpy(bits.reshape(-1)).cuda(), torch.from_numpy(msgs).cuda(), torch.from_numpy(sigs).cuda()
    d_want, d_out = torch.zeros((k, 320), dtype=torch.uint8, device="cuda"), torch.zeros((k, 320), dtype=torch.uint8, device="cuda")
    d_bases = torch.zeros((COMMITTEES, 320), dtype=torch.uint8, device="cuda")
    zm, zs = torch.zeros(COMMITTEES * 32, dtype=torch.uint8, device="cuda"), torch.zeros(COMMITTEES * 192, dtype=torch.uint8, device="cuda")
    ok, st = m.aggregateSets_device(c, d_table.data_ptr(), TABLE, d_cidx.data_ptr(), c_offsets, zm.data_ptr(), zs.data_ptr(), d_bases.data_ptr())
    assert ok and st == bytes(COMMITTEES)                                       # the committees' own aggregates: once per epoch
    # the timed calls go to the C ABI with the host arrays built once: converting 65 536 Python integers would cost more than the kernels
    import ctypes
    lib, st_buf = m.lib(), ctypes.create_string_buffer(k)
    offs_a, coffs_a = (ctypes.c_size_t * (k + 1))(*offs), (ctypes.c_size_t * (COMMITTEES + 1))(*c_offsets)
    wh_a = (ctypes.c_uint32 * k)(*[int(x) for x in which])

    def yardstick():
        ok = m._check(lib.mi355_bls_aggregate_sets_device(c._h, d_table.data_ptr(), TABLE, d_idx.data_ptr(), offs_a, k, d_msgs.data_ptr(), d_sigs.data_ptr(),
                                                          d_want.data_ptr(), st_buf, None))
        return bool(ok), st_buf.raw

    def bits_call(d_aggs, stride):
        ok = m._check(lib.mi355_bls_aggregate_sets_bits_device(c._h, d_table.data_ptr(), TABLE, d_cidx.data_ptr(), coffs_a, COMMITTEES, d_aggs, stride, wh_a,
                                                               d_bits.data_ptr(), k, d_msgs.data_ptr(), d_sigs.data_ptr(), d_out.data_ptr(), st_buf, None))
        return bool(ok), st_buf.raw

    def with_bases():
        return bits_call(d_bases.data_ptr(), 320)

    def without_bases():
        return bits_call(None, 96)
    ok, st = yardstick()
    assert ok and st == bytes(k)
    row = {"shape": name, "sets": k, "committee": L, "participation_percent": pct, "keys_added_directly": int(len(idx))}
    for fn, label in ((with_bases, "bits_with_bases"), (without_bases, "bits_without_bases")):
        d_out.zero_()
        ok, st = fn()
        assert ok and st == bytes(k) and torch.equal(d_out, d_want), "records differ from the yardstick's"
        row[label + "_routes"] = list(m.debug_aggregate_bits_routes(c))
    row["aggregate_sets_expanded"] = timed(yardstick)
    row["bits_with_bases"] = timed(with_bases)
    row["bits_without_bases"] = timed(without_bases)
    row["with_bases_over_expanded"] = round(row["bits_with_bases"]["median_ms"] / row["aggregate_sets_expanded"]["median_ms"], 3)
    row["without_bases_over_expanded"] = round(row["bits_without_bases"]["median_ms"] / row["aggregate_sets_expanded"]["median_ms"], 3)
    fixed = TABLE * 96 + k * 224
    row["staged_bytes"] = {"aggregate_sets": fixed + 4 * len(idx), "aggregate_sets_bits": fixed + 4 * COMMITTEES * L + 96 * COMMITTEES + bits.size}
    if verify:
        rnd = hashlib.sha256(b"bench aggbits rnd").digest()

        def v_bits():
            return m._check(lib.mi355_bls_batch_fast_aggregate_verify_bits_device(c._h, d_table.data_ptr(), TABLE, d_cidx.data_ptr(), coffs_a, COMMITTEES,
                                                                                  d_bases.data_ptr(), 320, wh_a, d_bits.data_ptr(), k, d_msgs.data_ptr(),
                                                                                  d_sigs.data_ptr(), rnd, None)) == 1

        def v_expanded():
            return m._check(lib.mi355_bls_batch_fast_aggregate_verify_device(c._h, d_table.data_ptr(), TABLE, d_idx.data_ptr(), offs_a, k, d_msgs.data_ptr(),
                                                                             d_sigs.data_ptr(), rnd, None)) == 1
        assert v_bits() is True and v_expanded() is True
        row["batch_fast_aggregate_verify_bits"] = timed(v_bits)
        row["batch_fast_aggregate_verify"] = timed(v_expanded)
    return row


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_aggbits: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_bits_bench.json"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)))
        return
    rows = [child(name, 240) for name in SHAPES]
    res = {"how": "ms per blocking call, host clock, median of 5 after a warm-up with min .. max; everything device-resident; the yardstick "
                  "(aggregate_sets_expanded) is mi355_bls_aggregate_sets_device over the expanded index lists of the same sets, same process; "
                  "AGGB_P = 8, no other value tried", "rows": rows}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
