#!/usr/bin/env python3
"""Generates tests/golden/combine_sets.json: groups of same-message SignatureSet records ("segments") with the record, status byte and
`verify` verdict MultiSignatureSet.combine gives for each (bls_batch_verifier.nim:47-106, blst_min_pubkey_sig_core.nim:570-647), from
oracle/bls12381_py.py alone: sk_to_pk, hash_to_g2, g2_mul, combine_scalars, combine, core_verify.  C = 8 is the plan's operands per item
(csrc/plan.hpp AGG_C; tests/test_combsets_plan.py holds the two together).

`table`: the distinct member records, shuffled by the hash of their bytes; a segment's `members` are indices into it, so the contiguous
form of a test is the members' records laid end to end and the indexed form is the table with the members as the index array (the
`twice` segment repeats an index).  Segments: lengths 1, 2, 3, 4, 5 (crosses a digest: four scalars each), C - 1, C, C + 1, C^2 + 1, 64, 65;
`twice` (the same record twice); `inf_sig` (a member whose signature is the infinity image); `equal_terms` (sk_1 = s_0 sk_0 / s_1, so
s_0 PK_0 = s_1 PK_1 and s_0 S_0 = s_1 S_1: the sums meet P = Q on both curves); `cancel` (sk_1 = -s_0 sk_0 / s_1: key and signature sum to
infinity, status 2); `wrong_signature` (one bad member among C + 1: a well-formed record that verifies false); `empty` (status 1);
`mixed` (one member signs another message, status 4); `inf_key` (a member with the infinity key, status 5).  `bad_index`: one position of
the C + 1 segment whose index, replaced by a value past the table, gives status 3.  A record whose status is not 0: the infinity key, the
first member's message (zero if there is none), the infinity signature.

Run:  python tests/golden/gen_combine_sets.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
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


def fresh_sk():
    sk = int.from_bytes(hashlib.sha256(b"combine_sets sk %d" % _next[0]).digest(), "little") % o.R or 1
    _next[0] += 1
    return sk


def main():
    segs = []       # (kind, rnd, message, [(pk point or None, message, signature point or None)])

    def seg(kind, build):
        i = len(segs)
        msg = hashlib.sha256(b"combine_sets msg %d" % i).digest()
        rnd = hashlib.sha256(b"combine_sets rnd %d" % i).digest()
        h = o.hash_to_g2(msg)
        segs.append((kind, rnd, build(msg, h, rnd)))
        print("built", kind, flush=True)

    def signed(sks):
        return lambda msg, h, rnd: [(o.sk_to_pk(sk), msg, o.g2_mul(h, sk)) for sk in sks]

    for n in sorted({1, 2, 3, 4, 5, C - 1, C, C + 1, C * C + 1, 64, 65}):
        seg("len_%d" % n, signed([fresh_sk() for _ in range(n)]))
    sk = fresh_sk()
    seg("twice", signed([sk, sk]))

    def inf_sig(msg, h, rnd):
        m = signed([fresh_sk() for _ in range(3)])(msg, h, rnd)
        m[1] = (m[1][0], msg, None)
        return m
    seg("inf_sig", inf_sig)

    def related(sign):
        def build(msg, h, rnd):
            s0, s1 = o.combine_scalars(rnd, 2)
            sk0 = fresh_sk()
            sk1 = sign * s0 * sk0 * pow(s1, -1, o.R) % o.R
            assert (s0 * sk0 - sign * s1 * sk1) % o.R == 0
            return signed([sk0, sk1])(msg, h, rnd)
        return build
    seg("equal_terms", related(1))
    seg("cancel", related(-1))

    def wrong_signature(msg, h, rnd):
        sks = [fresh_sk() for _ in range(C + 1)]
        m = signed(sks)(msg, h, rnd)
        m[C - 2] = (m[C - 2][0], msg, o.g2_mul(h, (sks[C - 2] + 1) % o.R))
        return m
    seg("wrong_signature", wrong_signature)
    seg("empty", lambda msg, h, rnd: [])

    def mixed(msg, h, rnd):
        sks = [fresh_sk() for _ in range(3)]
        m = signed(sks)(msg, h, rnd)
        other = hashlib.sha256(b"another message").digest()
        m[2] = (m[2][0], other, o.sign(sks[2], other))
        return m
    seg("mixed", mixed)

    def inf_key(msg, h, rnd):
        m = signed([fresh_sk() for _ in range(3)])(msg, h, rnd)
        m[1] = (None, msg, m[1][2])
        return m
    seg("inf_key", inf_key)

    def image(member):
        pk, msg, sig = member
        return o.g1_to_blst_affine(pk) + msg + o.g2_to_blst_affine(sig)

    def no_record(members):
        return bytes(96) + (members[0][1] if members else bytes(32)) + bytes(192)

    out, images = [], []
    for kind, rnd, members in segs:
        pks, sigs = [m[0] for m in members], [m[2] for m in members]
        status = (1 if not members else 4 if any(m[1] != members[0][1] for m in members) else 5 if any(p is None for p in pks) else 0)
        verdict = False
        if status == 0:
            pk, sig = o.combine(rnd, pks, sigs)
            if len(members) >= 2:                                  # the sums again, term by term with the chain's scalars
                ss = o.combine_scalars(rnd, len(members))
                assert pk == o.aggregate_g1([o.g1_mul(p, s) for p, s in zip(pks, ss)])
                assert sig == o.aggregate_g2([o.g2_mul(q, s) for q, s in zip(sigs, ss) if q is not None])
            if pk is None:
                status = 2
        if status == 0:
            record = image((pk, members[0][1], sig))
            verdict = sig is not None and o.core_verify(pk, members[0][1], sig)
        else:
            record = no_record(members)
        want = {"cancel": (2, False), "wrong_signature": (0, False), "inf_sig": (0, False), "empty": (1, False), "mixed": (4, False), "inf_key": (5, False)}
        assert (status, verdict) == want.get(kind, (0, True)), (kind, status, verdict)
        if kind == "cancel":
            assert o.combine(rnd, pks, sigs) == (None, None)
        imgs = [image(m) for m in members]
        images.append(imgs)
        out.append({"kind": kind, "rnd": rnd.hex(), "record": record.hex(), "status": status, "verdict": int(verdict)})
        print(kind, len(members), status, verdict, flush=True)
    distinct = sorted({b for imgs in images for b in imgs}, key=lambda b: hashlib.sha256(b).digest())
    where = {b: j for j, b in enumerate(distinct)}
    for s, imgs in zip(out, images):
        s["members"] = [where[b] for b in imgs]
    flat = [j for s in out for j in s["members"]]
    assert len(set(flat)) < len(flat) and flat != sorted(flat)      # repeated indices, a shuffled table
    bad_seg = [s["kind"] for s in out].index("len_%d" % (C + 1))
    bad = {"segment": bad_seg, "position": C, "value": len(distinct) + 5, "status": 3,                 # the one member of the segment's second item
           "record": no_record(segs[bad_seg][2]).hex()}
    doc = {"comment": "tests/golden/gen_combine_sets.py: per-segment combined record (320-byte SignatureSet image), status and verify verdict from oracle/bls12381_py.py",
           "C": C, "table": b"".join(distinct).hex(), "segments": out, "bad_index": bad}
    with open(os.path.join(HERE, "combine_sets.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "segments,", len(distinct), "distinct records")


if __name__ == "__main__":
    main()
