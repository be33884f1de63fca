#!/usr/bin/env python3
"""Generates tests/golden/latency_handover.json: the C restatement's results for blocking batch calls at the sizes where a latency-mode
context hands a stage over to another executor (tests/util.py latency_hand_overs; at S = 4 x 256 CUs = 1024 wave slots: 4 S, 11 S, 16 S,
18 S, 32 S), one valid and one defective batch per size.  tests/test_gpu_latency_handover.py rebuilds the inputs on the device and compares.

Run once in the build container:  python tests/golden/gen_latency_handover.py
Inputs: one batch oracle_make_batch(32 769, seed=SEED) (sk_i = SHA256("sk" || LE64(SEED + i)), msg_i = SHA256("msg" || decimal(i))); the case
of n sets is its first n records.  rnd = SHA256("Mr F was here"), numThreads = 64 throughout.
"""
import hashlib
import json
import os
import random
import struct
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import c_oracle as co  # noqa: E402
from util import apply_defect, latency_hand_overs, latency_plan  # noqa: E402

SEED = 0x1A7E_0000
NT = 64
S = 1024                                     # MI355X: 256 CUs
RND = hashlib.sha256(b"Mr F was here").digest()
# both sides of every hand-over, and one size inside the WIDE range away from both of its ends
SIZES = sorted({t + d for _, t in latency_hand_overs(S) for d in (0, 1)} | {8 * S})
KINDS = ["swap", "msg", "infpk", "infsig"]   # encoded as in tests/gpu_soak.py


def hx(b):
    return bytes(b).hex()


def sample_indices(n, rng):
    idx = {0, 1, n - 2, n - 1} | {i for i in (4 * S - 1, 4 * S, 4 * S + 1) if i < n}
    while len(idx) < 16:
        idx.add(rng.randrange(n))
    return sorted(idx)


def main():
    assert SIZES == [4096, 4097, 8192, 11264, 11265, 16384, 16385, 18432, 18433, 32768, 32769], SIZES
    t0 = time.time()
    nmax = SIZES[-1]
    recs = co.make_batch(nmax, seed=SEED)
    print("make_batch(%d): %.1f s" % (nmax, time.time() - t0), flush=True)
    rng = random.Random(SEED)
    cases = []
    for k, n in enumerate(SIZES):
        rec = recs[:320 * n]
        ok, st = co.batch_verify(rec, RND, NT, stages=True)
        assert ok, n
        valid = {"verdict": ok, "gt": hx(st["gt"]), "aggsig": hx(st["aggsig"]),
                 "r_sha256": hashlib.sha256(struct.pack("<%dQ" % n, *st["r"])).hexdigest(),
                 "samples": [[i, hx(st["H"][192 * i:192 * i + 192]), hx(st["rPK"][96 * i:96 * i + 96])] for i in sample_indices(n, rng)]}
        # the defect: kinds in rotation; at index n - 1 for every n = 1 mod 4 (the lone live team of a partly filled last wave) and every
        # other size besides (seven of eleven), at a random index otherwise
        kind = KINDS[k % 4]
        at = n - 1 if n % 4 == 1 or k % 2 == 0 else rng.randrange(1, n - 1)
        d = {"kind": kind, "indices": [at]}
        if kind == "swap":
            d["indices"] = [at, rng.randrange(0, at)]
        elif kind == "msg":
            d["byte"], d["bit"] = rng.randrange(32), rng.randrange(8)
        bad = bytearray(rec)
        apply_defect(bad, d)
        ok, st = co.batch_verify(bytes(bad), RND, NT, stages=True)
        assert not ok, (n, d)
        d["verdict"] = ok
        d["gt"] = None if kind == "infpk" else hx(st["gt"])           # the reference stops early at an infinity key: no comparable GT value
        cases.append({"n": n, "records_sha256": hashlib.sha256(rec).hexdigest(), "plan_s1024": latency_plan(n, S), "valid": valid, "defect": d})
        print("n=%d  defect %s at %s  %.1f s" % (n, kind, d["indices"], time.time() - t0), flush=True)
    # every kind of defect on both sides of at least one hand-over
    for kind in KINDS:
        ns = [c["n"] for c in cases if c["defect"]["kind"] == kind]
        assert any(min(ns) <= t < max(ns) for _, t in latency_hand_overs(S)), (kind, ns)
    assert 2 * sum(c["defect"]["indices"][0] == c["n"] - 1 for c in cases) >= len(cases)
    out = {"note": "C restatement's batch verification at the latency-mode hand-over sizes; inputs: first n of oracle_make_batch(%d, seed), "
                   "rnd = SHA256('Mr F was here'), numThreads = %d; H / rPK samples are blst affine images" % (nmax, NT),
           "seed": SEED, "num_threads": NT, "rnd": hx(RND), "slots": S, "records": nmax, "cases": cases}
    path = os.path.join(HERE, "latency_handover.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
    print("wrote %s: %d bytes, %.1f s" % (path, os.path.getsize(path), time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
