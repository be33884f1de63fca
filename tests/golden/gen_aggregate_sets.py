#!/usr/bin/env python3
"""Generates tests/golden/aggregate_sets.json: key lists ("segments") with the aggregate key, status byte and fastAggregateVerify verdict of
each (bls_sig_min_pubkey.nim:234-258; aggregateAll, blst_min_pubkey_sig_core.nim:179-195), from oracle/bls12381_py.py alone: sk_to_pk,
aggregate_g1, sign with the sum of the secret keys, fast_aggregate_verify, g1_to_blst_affine.  C = 8 is the plan's operands per item
(csrc/plan.hpp AGG_C; tests/test_aggsets_plan.py holds the two together).

Segments: lengths 1, 2, C - 1, C, C + 1, C^2 + 1, 64, 65; an empty one (status 1); (P, P); (P, -P) (status 2); C copies of P then C copies
of P (two equal partials meet at level 1); (P, Q, -P, -Q, R); one with a wrong signature; one with a wrong message.  Status: 0 ok, 1 empty,
2 aggregate at infinity.  `indexed`: the same segments as indices into a shuffled table of the distinct keys (repeats where a segment
repeats a key), and one position whose index, replaced by a value past the table, gives its segment status 3.

Run:  python tests/golden/gen_aggregate_sets.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

C = 8
_next = [0]


def fresh(n):
    """n new (secret key, public key) pairs"""
    out = []
    for _ in range(n):
        sk = int.from_bytes(hashlib.sha256(b"aggregate_sets sk %d" % _next[0]).digest(), "little") % o.R or 1
        _next[0] += 1
        out.append((sk, o.sk_to_pk(sk)))
    return out


def neg(pair):
    return (o.R - pair[0], o.g1_neg(pair[1]))


def main():
    segs = []                                                   # (kind, [(sk, pk)], message or None = the segment's own, signing key or None = the sum)
    for n in (1, 2, C - 1, C, C + 1, C * C + 1, 64, 65):
        segs.append(("len_%d" % n, fresh(n)))
    segs.append(("empty", []))
    p, = fresh(1)
    segs.append(("p_p", [p, p]))
    p, = fresh(1)
    segs.append(("p_negp", [p, neg(p)]))
    p, = fresh(1)
    segs.append(("c_p_c_p", [p] * (2 * C)))
    p, q, r = fresh(3)
    segs.append(("p_q_negp_negq_r", [p, q, neg(p), neg(q), r]))
    segs.append(("wrong_signature", fresh(3)))
    segs.append(("wrong_message", fresh(3)))
    out = []
    for i, (kind, pairs) in enumerate(segs):
        msg = hashlib.sha256(b"aggregate_sets msg %d" % i).digest()
        sk = sum(s for s, _ in pairs) % o.R
        pts = [pk for _, pk in pairs]
        agg = o.aggregate_g1(pts)
        assert agg == (o.sk_to_pk(sk) if sk else None), kind
        status = 1 if not pts else 2 if agg is None else 0
        if kind == "wrong_signature":
            sig = o.sign((sk + 1) % o.R, msg)
        elif kind == "wrong_message":
            sig = o.sign(sk, hashlib.sha256(b"another message").digest())
        else:
            sig = o.sign(sk or 1, msg)                         # empty / infinity: a well-formed signature that cannot verify
        verdict = o.fast_aggregate_verify(pts, msg, sig)
        assert verdict == (status == 0 and not kind.startswith("wrong")), (kind, verdict)
        out.append({"kind": kind, "keys": b"".join(o.g1_to_blst_affine(x) for x in pts).hex(), "message": msg.hex(),
                    "signature": o.g2_to_blst_affine(sig).hex(), "aggregate": o.g1_to_blst_affine(agg if status == 0 else None).hex(),
                    "status": status, "verdict": int(verdict)})
        print(kind, status, verdict, flush=True)
    # the indexed form: distinct keys, shuffled by the hash of their bytes
    distinct = sorted({bytes.fromhex(s["keys"])[96 * j:96 * j + 96] for s in out for j in range(len(s["keys"]) // 192)}, key=lambda b: hashlib.sha256(b).digest())
    where = {b: j for j, b in enumerate(distinct)}
    idx, offsets = [], [0]
    for s in out:
        kb = bytes.fromhex(s["keys"])
        idx += [where[kb[96 * j:96 * j + 96]] for j in range(len(kb) // 96)]
        offsets.append(len(idx))
    assert len(set(idx)) < len(idx)                             # repeated indices
    bad_seg = [s["kind"] for s in out].index("len_%d" % (C + 1))
    bad = {"segment": bad_seg, "position": offsets[bad_seg] + C, "value": len(distinct) + 5, "status": 3}      # the one key of the segment's second item
    doc = {"comment": "tests/golden/gen_aggregate_sets.py: per-segment aggregate key (blst_p1_affine image), status and fastAggregateVerify verdict from oracle/bls12381_py.py",
           "C": C, "segments": out, "indexed": {"table": b"".join(distinct).hex(), "idx": idx, "offsets": offsets, "bad_index": bad}}
    with open(os.path.join(HERE, "aggregate_sets.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "segments,", len(distinct), "distinct keys")


if __name__ == "__main__":
    main()
