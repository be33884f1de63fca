#!/usr/bin/env python3
"""Generates tests/golden/recover_signatures.json: groups of threshold-signature shares with their ids and the signature recover(signs, ids)
(blst_recovery.nim:150-156) gives for each, as its blst_p2_affine image, its compressed wire form and its status byte.  lagrangeInterpolation
(blst_recovery.nim:90-121) is restated here over Python integers and oracle/bls12381_py.py's g2_mul / g2_add; nothing else is used.

An id is 32 little-endian bytes; its value is that integer mod r (the library's contract, include/blscurve_mi355x.h).  Shares are kept once in
`table` (entry 0 is the all-zero affine infinity image, the rest ordered by the hash of their bytes); a group is a list of table indices with
one id per member, so the contiguous form of a call lays the groups' entries end to end and the indexed form is (table, indices, offsets):
indices repeat and are shuffled.

Groups
  ref_*      the cases of the reference's tests/secret_sharing.nim: sk, msg = bytes 0..7, ids x 2^224 for x = 1..3 (ID.fromUint32 of
             [0, .., 0, x]); 1/1, 3/3, the 2-of-3 set in all pairs, all three, reversed, rekeyed, and the too-few-shares groups.  `verify` is
             core_verify(pk, msg, recovered), asserted true where the reference test asserts it and false where it asserts the opposite.
             The polynomials' higher coefficients are fixed scalars (the Nim keyGen(seed) values are not needed for the property).
  edge_*     empty (status 1); t = 1 with id 0 (status 0, the share itself); t = 2 with an id 0 (6); ids (5, 9, 5) (7); ids 1 and r + 1 (7);
             ids (r + 3, 7) and (3, 7) with the same shares (identical outputs); an id of 2^256 - 1; a member that is the infinity image;
             two shares with S1 = -[l0 / l1] S0 (status 2: the recovered point is infinity)
  len_*      8, 9, 64 and 65 members (the edges of the sum's levels, AGG_C = 8) with random 255-bit ids
  coeff_*    t = 2 with ids (1, c / (c - 1)): the first member's coefficient is exactly c, so the windowed multiplication is driven with
             chosen scalars (see CHOSEN)
`bad_index`: one position whose index, replaced by a value past the table, gives its group status 3.
`w4`: 256-bit scalars, found by the search below, at which the windowed multiplication's accumulator EQUALS its table operand (the complete
addition's doubling branch) or its negative (the cancelling branch); the first is below r and is also a coeff_ group, the second is not
(k = 0 mod r), so only the direct multiplication test can use it.

Run:  python tests/golden/gen_recover_signatures.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

R = o.R
SK = int("1b500388741efd98239a9b3a689721a89a92e8b209aabb10fb7dc3f844976dc2", 16)
MSG = bytes(range(8))


def h(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "little")


def lagrange(ys, ids):
    """lagrangeInterpolation over G2 points: -> (status, point)"""
    xs = [x % R for x in ids]                      # toFr
    k = len(xs)
    if k == 0 or k != len(ys):
        return 1, None                             # "invalid inputs"
    if k == 1:
        return 0, ys[0]
    a = 1
    for x in xs:
        a = a * x % R
    if a == 0:
        return 6, None                             # "zero secret share id"
    acc = None
    for i in range(k):
        b = xs[i]
        for j in range(k):
            if j != i:
                v = (xs[j] - xs[i]) % R
                if v == 0:
                    return 7, None                 # "duplicate secret share id"
                b = b * v % R
        acc = o.g2_add(acc, o.g2_mul(ys[i], a * pow(b, R - 2, R) % R))
    return 0, acc


def coefficient(ids, i):
    xs = [x % R for x in ids]
    a, b = 1, xs[i]
    for j, x in enumerate(xs):
        a = a * x % R
        if j != i:
            b = b * (x - xs[i]) % R
    return a * pow(b, R - 2, R) % R


def poly(cfs, x):
    y = 0
    for c in reversed(cfs):
        y = (y * x + c) % R
    return y


def recode_hits(k):
    """the signed 4-bit recoding of curve.hpp jac_mul_256_w4 walked over integers mod r: -> the set of 'double' / 'cancel' events"""
    digs, carry = [], 0
    for j in range(64):
        d = ((k >> (4 * j)) & 15) + carry
        carry = int(d > 8)
        digs.append(d - 16 if carry else d)
    acc, hits = carry, set()
    for j in reversed(range(64)):
        acc = acc * 16 % R
        d = digs[j]
        if d:
            if acc and acc == d % R:
                hits.add("double")
            if acc and acc == (-d) % R:
                hits.add("cancel")
            acc = (acc + d) % R
    assert acc == k % R
    return hits


CHOSEN = [("two", 2), ("all_8", int("73" + "88" * 31, 16)), ("all_7", int("73" + "77" * 31, 16)), ("all_9", int("73" + "99" * 31, 16)),
          ("carry_chain", int("0f" + "ff" * 31, 16)), ("one_digit", int("01" + "00" * 31, 16)), ("r_minus_1", R - 1)] + \
         [("8_at_%d" % j, 8 * 16 ** j) for j in (0, 1, 31, 62)]


def main():
    w4 = {}
    for m in (0, 1, 2):
        for e in range(-40, 41):
            k = m * R + e
            if 0 < k < 1 << 256:
                for kind in recode_hits(k):
                    if kind not in w4 or (w4[kind] >= R > k):
                        w4[kind] = k
    assert set(w4) == {"double", "cancel"} and w4["double"] < R, w4
    chosen = CHOSEN + [("accumulator_equals_entry", w4["double"])]
    assert all(1 < c < R for _, c in chosen)

    q = o.hash_to_g2(MSG)
    pk = o.sk_to_pk(SK)
    x224 = [x << 224 for x in (1, 2, 3)]
    share = lambda s: (o.g2_mul(q, s % R) if s % R else None)                # noqa: E731
    p3, p2, pz = [SK, h(b"recover c1") % R, h(b"recover c2") % R], [SK, h(b"recover d1") % R], [0, h(b"recover e1") % R]
    s11 = share(SK)
    s33 = [share(poly(p3, x)) for x in x224]
    k23 = [poly(p2, x) for x in x224]
    s23 = [share(s) for s in k23]
    srk = [share(s + poly(pz, x)) for s, x in zip(k23, x224)]
    pool = [share(h(b"recover pool %d" % i)) for i in range(65)]
    print("shares made", flush=True)

    groups = []          # (kind, [points], [ids], verify or None)
    groups.append(("ref_1_of_1", [s11], x224[:1], True))
    groups.append(("ref_3_of_3", s33, x224, True))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        groups.append(("ref_3_of_3_too_few_%d%d" % (a, b), [s33[a], s33[b]], [x224[a], x224[b]], False))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        groups.append(("ref_2_of_3_pair_%d%d" % (a, b), [s23[a], s23[b]], [x224[a], x224[b]], True))
    groups.append(("ref_2_of_3_all", s23, x224, True))
    groups.append(("ref_2_of_3_reversed", s23[::-1], x224[::-1], True))
    groups.append(("ref_rekeyed", srk, x224, True))
    for a in range(3):
        groups.append(("ref_2_of_3_too_few_%d" % a, [s23[a]], [x224[a]], False))
    groups.append(("edge_empty", [], [], None))
    groups.append(("edge_one_id_zero", [pool[0]], [0], None))
    groups.append(("edge_zero_id", [pool[0], pool[1]], [4, 0], None))
    groups.append(("edge_dup_595", [pool[0], pool[1], pool[2]], [5, 9, 5], None))
    groups.append(("edge_dup_mod_r", [pool[0], pool[1]], [1, R + 1], None))
    groups.append(("edge_r_plus_3", [pool[3], pool[4]], [R + 3, 7], None))
    groups.append(("edge_3", [pool[3], pool[4]], [3, 7], None))
    groups.append(("edge_id_all_ones", [pool[5], pool[6]], [(1 << 256) - 1, 11], None))
    groups.append(("edge_infinity_member", [pool[7], None, pool[8]], [2, 3, 4], None))
    ids = [h(b"recover inf id 0") >> 1, h(b"recover inf id 1") >> 1]
    l0, l1 = coefficient(ids, 0), coefficient(ids, 1)
    groups.append(("edge_result_infinity", [pool[9], o.g2_neg(o.g2_mul(pool[9], l0 * pow(l1, R - 2, R) % R))], ids, None))
    for n in (8, 9, 64, 65):
        groups.append(("len_%d" % n, [pool[(7 * n + t) % 65] for t in range(n)], [h(b"recover id %d %d" % (n, t)) >> 1 for t in range(n)], None))
    for name, c in chosen:
        ids = [1, c * pow(c - 1, R - 2, R) % R]
        assert coefficient(ids, 0) == c
        groups.append(("coeff_" + name, [pool[10], pool[11]], ids, None))

    images = {o.g2_to_blst_affine(pt) for _, pts, _, _ in groups for pt in pts if pt is not None}
    table = [bytes(192)] + sorted(images, key=lambda b: hashlib.sha256(b).digest())
    where = {b: i for i, b in enumerate(table)}
    out, idx, offsets = [], [], [0]
    for kind, pts, ids, verify in groups:
        status, rec = lagrange(pts, ids)
        if status == 0 and rec is None:
            status = 2
        if verify is not None:
            assert status == 0 and o.core_verify(pk, MSG, rec) is verify and (rec == s11) is verify, kind
        mi = [where[o.g2_to_blst_affine(pt)] for pt in pts]
        g = {"kind": kind, "members": mi, "ids": [x.to_bytes(32, "little").hex() for x in ids], "out192": o.g2_to_blst_affine(rec).hex(),
             "out96": o.g2_compress(rec).hex(), "status": status, "verify": verify}
        if kind.startswith("coeff_"):
            g["coeff"] = coefficient(ids, 0).to_bytes(32, "little").hex()
        out.append(g)
        idx += mi
        offsets.append(len(idx))
        print(kind, len(pts), status, flush=True)
    by = {g["kind"]: g for g in out}
    assert by["edge_r_plus_3"]["out192"] == by["edge_3"]["out192"] and by["edge_result_infinity"]["status"] == 2
    assert by["edge_one_id_zero"]["out192"] == o.g2_to_blst_affine(pool[0]).hex() and by["edge_one_id_zero"]["status"] == 0
    assert [by[n]["status"] for n in ("edge_empty", "edge_zero_id", "edge_dup_595", "edge_dup_mod_r")] == [1, 6, 7, 7]
    assert len(set(idx)) < len(idx) and idx != sorted(idx)
    bad_group = [g["kind"] for g in out].index("len_9")
    bad = {"group": bad_group, "position": offsets[bad_group] + 8, "value": len(table) + 5, "status": 3}      # the one member of the group's second sum item
    doc = {"comment": "tests/golden/gen_recover_signatures.py: recovered threshold signatures (blst_p2_affine image, compressed wire form, status) from oracle/bls12381_py.py",
           "r": "%x" % R, "sk": "%x" % SK, "msg": MSG.hex(), "pk": o.g1_to_blst_affine(pk).hex(), "table": b"".join(table).hex(), "groups": out,
           "indexed": {"idx": idx, "offsets": offsets, "bad_index": bad}, "w4": {k: v.to_bytes(32, "little").hex() for k, v in sorted(w4.items())}}
    with open(os.path.join(HERE, "recover_signatures.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "groups,", len(table), "table entries")


if __name__ == "__main__":
    main()
