#!/usr/bin/env python3
"""Generates tests/golden/aggregate_bits.json: small committees (index lists into one shuffled key table) and sets given as a committee number
and one bit per committee position, with the aggregate key of the participants, the status byte, the fastAggregateVerify verdict
(bls_sig_min_pubkey.nim:234-258; aggregateAll, blst_min_pubkey_sig_core.nim:179-195) and the route mi355_bls_aggregate_sets_bits must take
when the committees' own aggregates are given - from oracle/bls12381_py.py alone: sk_to_pk, aggregate_g1, sign with the sum of the secret
keys, fast_aggregate_verify, g1_to_blst_affine.

Bits: SSZ order, position i at bit i % 8 of byte i // 8, ceil(L / 8) bytes per set.  Route: 1 (the absentees are subtracted from the
committee's aggregate) iff that aggregate is not the all-zero image and 2 * popcount > L, else 0.  A committee's aggregate is all zero when
its sum is the point at infinity or when it holds an out-of-range index (what aggregateSets writes for it).

Sets: no bit / every bit / exactly half / half + 1 / only the last / only the first position; every unused bit of the last byte set; L in
{1, 7, 8, 9, 64, 65}; two sets on one committee; (P, -P) participating on both routes (status 2); (P, -P, R) with bits 110 (exclusion meets
base == sum); (P, P, -P) with bits 110 (exclusion meets the doubling branch); a committee with a repeated index; an out-of-range index at a
participating position (status 3) and at an absent one (status 0); a committee whose aggregate is infinity (the all-zero base forces the
direct route); a wrong signature; a wrong message.

Run:  python tests/golden/gen_aggregate_bits.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

_next = [0]
OOR = "oor"                                                     # a committee member that is an index past the table


def fresh(n):
    """n new (secret key, public key) pairs"""
    out = []
    for _ in range(n):
        sk = int.from_bytes(hashlib.sha256(b"aggregate_bits sk %d" % _next[0]).digest(), "little") % o.R or 1
        _next[0] += 1
        out.append((sk, o.sk_to_pk(sk)))
    return out


def neg(pair):
    return (o.R - pair[0], o.g1_neg(pair[1]))


def pack(bits, junk=False):
    """bits: a list of 0 / 1 by position -> the field; junk: every unused bit of the last byte set"""
    L = len(bits)
    b = bytearray((L + 7) // 8)
    for i, v in enumerate(bits):
        b[i // 8] |= v << (i % 8)
    if junk:
        assert L % 8
        b[-1] |= (0xff << (L % 8)) & 0xff
    return bytes(b)


def main():
    com = {}                                                    # name -> [(sk, pk) or OOR]
    for n in (1, 7, 8, 9, 64, 65):
        com["len_%d" % n] = fresh(n)
    p, q, r, s = fresh(4)
    com["p_negp"] = [p, neg(p)]                                  # aggregate at infinity: an all-zero base
    com["p_negp_q_negq"] = [p, neg(p), q, neg(q)]                # the same, longer
    com["p_negp_r"] = [p, neg(p), r]
    com["p_negp_r_s"] = [p, neg(p), r, s]
    com["p_p_negp"] = [q, q, neg(q)]
    a, b, c, d = fresh(4)
    com["repeated"] = [a, b, a, c, d, a]
    com["oor"] = [a, b, OOR, c]
    names = list(com)

    def ones(n, at):
        return [1 if i in at else 0 for i in range(n)]
    sets = [                                                    # (kind, committee, bits by position, junk)
        ("none_set", "len_9", [0] * 9, False),
        ("all_set", "len_9", [1] * 9, False),
        ("all_set_unused_bits_set", "len_9", [1] * 9, True),
        ("none_set_unused_bits_set", "len_9", [0] * 9, True),
        ("half", "len_8", ones(8, {0, 2, 5, 7}), False),
        ("half_plus_1", "len_8", ones(8, {0, 2, 3, 5, 7}), False),
        ("only_last", "len_64", ones(64, {63}), False),
        ("only_first", "len_64", ones(64, {0}), False),
        ("all_but_last", "len_64", ones(64, set(range(63))), False),
        ("len_1_set", "len_1", [1], False),
        ("len_1_delimiter_only", "len_1", [0], True),
        ("len_7_all_and_delimiter", "len_7", [1] * 7, True),
        ("len_7_three", "len_7", ones(7, {1, 4, 6}), False),
        ("len_65_most", "len_65", ones(65, set(range(65)) - {3, 40, 64}), True),
        ("len_65_last_only", "len_65", ones(65, {64}), False),
        ("len_65_33", "len_65", ones(65, set(range(0, 65, 2))), False),
        ("p_negp_direct", "p_negp", [1, 1], False),
        ("p_negp_tie_direct", "p_negp_r_s", [1, 1, 0, 0], False),
        ("p_negp_r_110", "p_negp_r", [1, 1, 0], False),
        ("p_p_negp_110", "p_p_negp", [1, 1, 0], False),
        ("infinity_base_forces_direct", "p_negp_q_negq", [1, 1, 1, 0], False),
        ("repeated_index_most", "repeated", [1, 0, 1, 1, 1, 1], False),
        ("repeated_index_few", "repeated", [1, 0, 1, 0, 0, 0], False),
        ("oor_participating", "oor", [1, 1, 1, 0], False),
        ("oor_absent", "oor", [1, 1, 0, 1], False),
        ("wrong_signature", "len_8", ones(8, set(range(7))), False),
        ("wrong_message", "len_8", ones(8, {1, 2}), False),
    ]
    # the table: the distinct keys, shuffled by the hash of their bytes
    img = {}
    for members in com.values():
        for x in members:
            if x != OOR:
                img[o.g1_to_blst_affine(x[1])] = None
    distinct = sorted(img, key=lambda k: hashlib.sha256(k).digest())
    where = {k: j for j, k in enumerate(distinct)}
    oor_value = len(distinct) + 5
    idx, c_offsets, bases = [], [0], {}
    for name in names:
        members = com[name]
        idx += [oor_value if x == OOR else where[o.g1_to_blst_affine(x[1])] for x in members]
        c_offsets.append(len(idx))
        agg = None if OOR in members else o.aggregate_g1([x[1] for x in members])
        bases[name] = o.g1_to_blst_affine(agg)
    assert len(set(idx)) < len(idx) and idx != sorted(idx)
    out = []
    for i, (kind, cname, bits, junk) in enumerate(sets):
        members = com[cname]
        assert len(bits) == len(members)
        part = [x for x, v in zip(members, bits) if v]
        pop, L = len(part), len(members)
        msg = hashlib.sha256(b"aggregate_bits msg %d" % i).digest()
        if OOR in part:
            status, agg, sk = 3, None, 1
        else:
            sk = sum(x[0] for x in part) % o.R
            agg = o.aggregate_g1([x[1] for x in part]) if part else None
            assert agg == (o.sk_to_pk(sk) if sk else None), kind
            status = 1 if not part else 2 if agg is None else 0
        if kind == "wrong_signature":
            sig = o.sign((sk + 1) % o.R, msg)
        elif kind == "wrong_message":
            sig = o.sign(sk, hashlib.sha256(b"another message").digest())
        else:
            sig = o.sign(sk or 1, msg)                           # no key: a well-formed signature that cannot verify
        verdict = status == 0 and o.fast_aggregate_verify([x[1] for x in part], msg, sig)
        assert verdict == (status == 0 and not kind.startswith("wrong")), (kind, verdict)
        route = int(bases[cname] != bytes(96) and 2 * pop > L)
        out.append({"kind": kind, "committee": names.index(cname), "bits": pack(bits, junk).hex(), "popcount": pop, "message": msg.hex(),
                    "signature": o.g2_to_blst_affine(sig).hex(), "aggregate": o.g1_to_blst_affine(agg if status == 0 else None).hex(),
                    "status": status, "verdict": int(verdict), "route": route})
        print(kind, status, verdict, route, flush=True)
    doc = {"comment": "tests/golden/gen_aggregate_bits.py: per-set aggregate key of the participants (blst_p1_affine image), status, fastAggregateVerify verdict "
                      "and route from oracle/bls12381_py.py",
           "table": b"".join(distinct).hex(), "idx": idx, "c_offsets": c_offsets, "oor_value": oor_value,
           "committees": [{"kind": n, "aggregate": bases[n].hex()} for n in names], "sets": out}
    with open(os.path.join(HERE, "aggregate_bits.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "sets,", len(names), "committees,", len(distinct), "distinct keys")


if __name__ == "__main__":
    main()
