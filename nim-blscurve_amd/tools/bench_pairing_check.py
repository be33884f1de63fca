#!/usr/bin/env python3
"""Stand-alone benchmark of the pairing-product checks (mi355_bls_pairing_check_each_device, mi355_bls_batch_pairing_check_device); bench.py
stays the flagship's.

  python nim-blscurve_amd/tools/bench_pairing_check.py [--out profiles/pairing_check_bench.json]

Every GPU step (one per number of pairs) runs in a child process of its own under `timeout`; the first step that fails ends the run.
Inputs, device-resident: pairs / 2 signed sets over ONE message from the device signer, laid out as the verifiers' own pairs - pair 2i =
(pk_i, H(m)), pair 2i + 1 = (-G1, sig_i), H(m) from mi355_bls_debug_hash_to_g2 - cut into groups of 2 and of 16 pairs, so every group is valid;
one signature swapped for its neighbour's must make exactly its group fail before anything is timed.  Times are host-clock medians of 5
blocking calls (each ends in a stream synchronise) after one warm-up call; min .. max of the same calls is the run-to-run spread.  Rows per
pairs x group size, all from the same process:
  pairing_check_each and batch_pairing_check, without and with MI355_BLS_PAIR_VALIDATE (validate_over_plain: the cost of validation);
  the parent's nearest calls: verify_each over pairs / 2 sets (the same pair structure plus hashing), aggregate_verify_each over the same sets
  in groups of group_size / 2 keys (the same number of groups), batch_verify_device over pairs / 2 sets (the blinded form's neighbour: pairs / 2 key pairs plus its signature buckets).
No ratio is asserted.  The item width (plan.hpp AGGV_C = 8) and the tail hand-over are inherited and were not re-measured."""
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
PAIRS = (256, 16384, 65536)
SIZES = (2, 16)


def load():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import __graft_entry__ as ge
    return ge.load_package()


def ms_per_call(fn, reps=5):
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
    import bls12381_py as o
    from util import g2_jac_to_affine
    sets = pairs // 2
    c = m.BatchedBLSVerifierCache.init(max_sets=max(pairs, 64), numThreads=4096)
    rng = np.random.default_rng(20261020)
    sks = rng.integers(1, 255, size=(sets, 32), dtype=np.uint8)
    sks[:, 31] = 0                                                           # below the group order
    msg = hashlib.sha256(b"bench pairing_check").digest()
    ok, rec, _ = m.signSets(c, sks.tobytes(), msg * sets)
    assert ok
    r = np.frombuffer(rec, dtype=np.uint8).reshape(sets, 320)
    out = ctypes.create_string_buffer(288)
    m._check(m.lib().mi355_bls_debug_hash_to_g2(c._h, msg, 32, o.DST_SIG, len(o.DST_SIG), out))
    hm = np.frombuffer(o.g2_to_blst_affine(g2_jac_to_affine(out.raw)), dtype=np.uint8)
    neg_g1 = np.frombuffer(o.g1_to_blst_affine(o.g1_neg(o.G1_GEN)), dtype=np.uint8)
    p1 = np.empty((pairs, 96), dtype=np.uint8)
    q2 = np.empty((pairs, 192), dtype=np.uint8)
    p1[0::2], p1[1::2], q2[0::2], q2[1::2] = r[:, :96], neg_g1, hm, r[:, 128:]
    d_p1, d_q2 = torch.from_numpy(p1).cuda(), torch.from_numpy(q2).cuda()
    d_rec = torch.from_numpy(r.copy()).cuda()
    d_keys = torch.from_numpy(np.ascontiguousarray(r[:, :96])).cuda()
    d_msgs = torch.from_numpy(np.ascontiguousarray(r[:, 96:128])).cuda()
    d_sigs = torch.from_numpy(np.ascontiguousarray(r[:, 128:])).cuda()
    rnd = hashlib.sha256(b"bench pairing_check rnd").digest()
    rows = []
    for size in SIZES:
        k = pairs // size
        offs = [g * size for g in range(k + 1)]
        row = {"pairs": pairs, "group_size": size, "k": k}
        assert m.pairingCheckEach_device(c, d_p1.data_ptr(), d_q2.data_ptr(), offs, flags=m.PAIR_VALIDATE) == ([True] * k, [0] * pairs)
        assert m.batchPairingCheck_device(c, d_p1.data_ptr(), d_q2.data_ptr(), offs, rnd) is True
        bad = d_q2.clone()
        at = (k // 2) * size + 1                                             # a signature pair of group k // 2 gets its neighbour's signature
        bad[at] = d_q2[(at + 2) % pairs]
        assert m.pairingCheckEach_device(c, d_p1.data_ptr(), bad.data_ptr(), offs)[0] == [g != k // 2 for g in range(k)]
        assert m.batchPairingCheck_device(c, d_p1.data_ptr(), bad.data_ptr(), offs, rnd) is False
        del bad
        for name, flags in (("plain", 0), ("validate", m.PAIR_VALIDATE)):
            row["pairing_check_each_%s_ms" % name] = ms_per_call(lambda: m.pairingCheckEach_device(c, d_p1.data_ptr(), d_q2.data_ptr(), offs, flags=flags))
            row["batch_pairing_check_%s_ms" % name] = ms_per_call(lambda: m.batchPairingCheck_device(c, d_p1.data_ptr(), d_q2.data_ptr(), offs, rnd, flags=flags))
        # the parent's nearest calls
        row["verify_each_half_as_many_sets_ms"] = ms_per_call(lambda: m.verifyEach_device(c, d_rec.data_ptr(), sets))
        gk = size // 2                                                       # keys per group: the same number of groups
        goffs = [g * gk for g in range(k + 1)]
        d_agg = torch.zeros((k, 192), dtype=torch.uint8, device="cuda")
        ok, st = m.aggregateSignatureSets_device(c, d_sigs.data_ptr(), sets, None, goffs, d_agg.data_ptr(), None)
        assert ok and st == bytes(k)
        row["aggregate_verify_each_same_groups_ms"] = ms_per_call(
            lambda: m.aggregateVerifyEach_device(c, d_keys.data_ptr(), sets, None, goffs, d_msgs.data_ptr(), d_agg.data_ptr()))
        row["batch_verify_half_as_many_sets_ms"] = ms_per_call(lambda: c.verify_device(d_rec.data_ptr(), sets, rnd))
        e, b = row["pairing_check_each_plain_ms"]["median"], row["batch_pairing_check_plain_ms"]["median"]
        row["each_validate_over_plain"] = round(row["pairing_check_each_validate_ms"]["median"] / e, 2)
        row["batch_validate_over_plain"] = round(row["batch_pairing_check_validate_ms"]["median"] / b, 2)
        row["each_over_verify_each"] = round(e / row["verify_each_half_as_many_sets_ms"]["median"], 2)
        row["each_over_aggregate_verify_each"] = round(e / row["aggregate_verify_each_same_groups_ms"]["median"], 2)
        row["batch_over_batch_verify"] = round(b / row["batch_verify_half_as_many_sets_ms"]["median"], 2)
        rows.append(row)
        del d_agg
    return rows


def child(name, seconds):
    """one GPU step in a fresh process under its own time limit -> its JSON result; any failure ends the whole run"""
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", name], stdout=subprocess.PIPE)
    if p.returncode != 0:
        sys.exit("bench_pairing_check: step %s failed with exit status %d: stopping here" % (name, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_check_bench.json"))
    ap.add_argument("--step", default=None)
    ap.add_argument("--pairs", default=",".join(str(k) for k in PAIRS), help="the pair counts to run, comma separated")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(int(a.step))))
        return
    rows = []
    for n in (int(x) for x in a.pairs.split(",")):
        rows += child(str(n), 300)
    res = {"how": "ms per blocking call, host clock: median, min and max of 5 calls after a warm-up - min .. max is the run-to-run spread; device-resident "
                  "inputs; the neighbours (verify_each over pairs / 2 sets, aggregate_verify_each over the same number of groups, batch_verify_device over "
                  "pairs / 2 sets) run in the same process; x_over_y is new / neighbour (above 1: the new call is slower); item "
                  "width AGGV_C = 8 and the tail hand-over inherited, not re-measured",
           "rows": rows,
           "slower_than_a_neighbour": [[r["pairs"], r["group_size"], key] for r in rows
                                       for key in ("each_over_verify_each", "each_over_aggregate_verify_each", "batch_over_batch_verify") if r[key] > 1]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
