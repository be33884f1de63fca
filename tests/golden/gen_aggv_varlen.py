#!/usr/bin/env python3
"""Generates tests/golden/aggv_varlen.json: the C restatement's aggregateVerify (verdict and GT value) on messages of many lengths - the
cases of tests/util.py varlen_case - valid and with defects that move one message boundary, one byte or two messages.
tests/test_gpu_aggv_varlen.py rebuilds keys and messages from the same rule and compares; tests/test_c_oracle.py pins the restatement's
hash-to-G2 over the same lengths, and its aggregateVerify on the `wave` case, to the Python oracle.

Run in the build container:  python tests/golden/gen_aggv_varlen.py        (about 45 s on 8 cores: 5 200 signatures at 4.4 ms each, then
26 aggregate verifications of up to 4 097 pairs).  The output is reproducible byte for byte: no clock, no `random`.

Per case and size: SHA-256 of the public keys (the restatement's sk_to_pk) and of the messages, the aggregate signature (sum of the
restatement's signatures), and verdict + GT for the valid input and every defect.  No defect makes the restatement stop early (none touches a
key), so every GT value is comparable; a `null` GT would mean "not comparable", as in latency_handover.json.
"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import c_oracle as co  # noqa: E402
from util import VARLEN_CASES, VARLEN_PREFIXES, varlen_case, varlen_defect  # noqa: E402

# (case, size) -> defects.  shift: the boundary between messages i and i + 1; trail: one byte appended; flip: last byte of a message of >= 4 096
# bytes; swap: two messages of different lengths.  `mixed` and `wide` carry all four kinds (and both trailing bytes).
DEFECTS = {
    ("one", 1): [{"kind": "trail", "index": 0, "byte": 0x00}],
    ("wave", 63): [{"kind": "shift", "index": 61}],                                   # into the last live lane of a partly filled wave
    ("wave", 64): [{"kind": "swap", "index": 0, "other": 63}],                        # first and last lane of a full wave
    ("wave", 65): [{"kind": "flip", "index": 64}, {"kind": "trail", "index": 64, "byte": 0x80}, {"kind": "shift", "index": 63}],      # the lone lane of block 1
    ("mixed", 1000): [{"kind": "shift", "index": 400},                                # inside the run of 32-byte messages: 33 | 31
                      {"kind": "trail", "index": 7, "byte": 0x00},                    # the empty message
                      {"kind": "trail", "index": 17, "byte": 0x80},                   # 8 bytes: the padding edge
                      {"kind": "flip", "index": 4},
                      {"kind": "swap", "index": 2, "other": 999}],
    ("wide", 4097): [{"kind": "shift", "index": 4095},                                # last lane of block 63 | the lone lane of block 64
                     {"kind": "trail", "index": 4096, "byte": 0x00},
                     {"kind": "trail", "index": 17, "byte": 0x80},
                     {"kind": "flip", "index": 6},
                     {"kind": "swap", "index": 0, "other": 4095}],
    ("long", 40): [{"kind": "flip", "index": 0}, {"kind": "shift", "index": 3}, {"kind": "trail", "index": 20, "byte": 0x00}],
}


def msgs_digest(msgs):
    h = hashlib.sha256()
    for x in msgs:
        h.update(len(x).to_bytes(4, "little"))
        h.update(x)
    return h.hexdigest()


def main():
    t0 = time.time()
    cases = []
    for name in VARLEN_CASES:
        sks, msgs = varlen_case(name)
        pks = [co.sk_to_pk(sk) for sk in sks]
        sigs = [co.sign(sk, x) for sk, x in zip(sks, msgs)]
        print("%s: %d pairs signed  %.1f s" % (name, len(sks), time.time() - t0), flush=True)
        for n in VARLEN_PREFIXES[name]:
            p, x = pks[:n], msgs[:n]
            agg = co.g2_sum(b"".join(sigs[:n]))
            ok, gt = co.aggregate_verify(p, x, agg, gt=True)
            assert ok is True, (name, n)
            defects = []
            for d in DEFECTS[(name, n)]:
                bad = varlen_defect(x, d)
                okd, gtd = co.aggregate_verify(p, bad, agg, gt=True)
                assert okd is False and gtd != gt, (name, n, d)
                defects.append(dict(d, verdict=okd, gt=gtd.hex()))
            cases.append({"name": name, "n": n, "lengths_sha256": hashlib.sha256(b"".join(len(y).to_bytes(4, "little") for y in x)).hexdigest(),
                          "pks_sha256": hashlib.sha256(b"".join(p)).hexdigest(), "msgs_sha256": msgs_digest(x), "aggsig": agg.hex(),
                          "valid": {"verdict": ok, "gt": gt.hex()}, "defects": defects})
            print("%s n=%d: valid + %d defects  %.1f s" % (name, n, len(defects), time.time() - t0), flush=True)
    for name in ("mixed", "wide"):
        kinds = {(d["kind"], d.get("byte")) for c in cases if c["name"] == name for d in c["defects"]}
        assert kinds == {("shift", None), ("trail", 0), ("trail", 0x80), ("flip", None), ("swap", None)}, (name, kinds)
    out = {"note": "C restatement's aggregateVerify on the inputs of tests/util.py varlen_case (keys and messages are regenerated from that rule); "
                   "GT values are 576-byte blst_fp12 images, signatures blst affine images",
           "cases": cases}
    path = os.path.join(HERE, "aggv_varlen.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
    print("wrote %s: %d bytes, %.1f s" % (path, os.path.getsize(path), time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
