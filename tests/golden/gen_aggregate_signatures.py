#!/usr/bin/env python3
"""Generates tests/golden/aggregate_signatures.json: signature groups with the aggregate of each (aggregateAll on signatures,
blst_min_pubkey_sig_core.nim:142-211), finished to its blst_p2_affine image and serialised (bls_sig_io.nim:225-234), and its status byte, from
oracle/bls12381_py.py alone: hash_to_g2, g2_mul, g2_neg, aggregate_g2, g2_to_blst_affine, g2_compress.  C = 8 is the plan's operands per
item (csrc/plan.hpp AGG_C).

The signatures are [s_i] H(m) for one message m (signers of one attestation), kept once in `table` (entry 0 is the all-zero affine infinity
image); a group is a list of table indices, so the contiguous form of a call is the groups' table entries laid end to end, and the indexed
form is (table, the groups' indices end to end, offsets) - the table is ordered by the hash of its entries, so the indices are shuffled, and
groups share entries, so indices repeat.  Groups: lengths 1, 2, C - 1, C, C + 1, C^2 + 1, 64, 65; an empty one (status 1); (S, S); (S, -S)
(status 2: the sum is the point at infinity, its valid encodings are expected); C copies of S then C more (two equal partials meet at level
1); one with an all-zero member; one of all-zero members only (status 2).  `bad_index`: one position whose index, replaced by a value past
the table, gives its group status 3 and the infinity encodings.  Each aggregate is also checked against [sum of the s_i] H(m).

Run:  python tests/golden/gen_aggregate_signatures.py      (pure Python, about a minute).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

C = 8


def main():
    q = o.hash_to_g2(hashlib.sha256(b"aggregate_signatures msg").digest())
    sks = [int.from_bytes(hashlib.sha256(b"aggregate_signatures sk %d" % i).digest(), "little") % o.R or 1 for i in range(C * C + 1 + 4)]
    pool = [(s, o.g2_mul(q, s)) for s in sks]
    base, (p1, p2, p3, p4) = pool[:C * C + 1], pool[C * C + 1:]
    neg = (o.R - p2[0], o.g2_neg(p2[1]))
    zero = (0, None)
    groups = []
    for j, n in enumerate((1, 2, C - 1, C, C + 1, C * C + 1, 64, 65)):
        members = [base[(5 * j + t) % len(base)] for t in range(n)]          # another start in the pool for every length
        groups.append(("len_%d" % n, members[::-1] if j == 7 else members))
    groups += [("empty", []), ("s_s", [p1, p1]), ("s_negs", [p2, neg]), ("c_s_c_s", [p3] * (2 * C)), ("with_zero", [p4, zero, base[0]]),
               ("only_zero", [zero, zero])]
    # the table: entry 0 the infinity image, then the distinct signatures by the hash of their bytes
    images = {o.g2_to_blst_affine(pt) for _, members in groups for _, pt in members if pt is not None}
    table = [bytes(192)] + sorted(images, key=lambda b: hashlib.sha256(b).digest())
    where = {b: i for i, b in enumerate(table)}
    out, idx, offsets = [], [], [0]
    for kind, members in groups:
        agg = o.aggregate_g2([pt for _, pt in members])
        sk = sum(s for s, _ in members) % o.R
        assert agg == (o.g2_mul(q, sk) if sk else None), kind
        status = 1 if not members else 2 if agg is None else 0
        mi = [where[o.g2_to_blst_affine(pt)] for _, pt in members]
        out.append({"kind": kind, "members": mi, "out192": o.g2_to_blst_affine(agg).hex(), "out96": o.g2_compress(agg).hex(), "status": status})
        assert o.g2_decompress(o.g2_compress(agg)) == agg
        idx += mi
        offsets.append(len(idx))
        print(kind, len(members), status, flush=True)
    assert len(set(idx)) < len(idx) and idx != sorted(idx)
    bad_group = [g["kind"] for g in out].index("len_%d" % (C + 1))
    bad = {"group": bad_group, "position": offsets[bad_group] + C, "value": len(table) + 5, "status": 3}      # the one member of the group's second item
    doc = {"comment": "tests/golden/gen_aggregate_signatures.py: per-group aggregate signature (blst_p2_affine image and compressed wire form) and status from oracle/bls12381_py.py",
           "C": C, "table": b"".join(table).hex(), "groups": out, "indexed": {"idx": idx, "offsets": offsets, "bad_index": bad}}
    with open(os.path.join(HERE, "aggregate_signatures.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "groups,", len(table), "table entries")


if __name__ == "__main__":
    main()
