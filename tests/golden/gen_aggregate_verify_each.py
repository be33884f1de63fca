#!/usr/bin/env python3
"""Generates tests/golden/aggregate_verify_each.json: twelve groups of (public key, message) pairs with one aggregate signature each, and the
verdict and value of aggregateVerify (bls_sig_min_pubkey.nim:127-199 -> ContextCoreAggregateVerify, blst_min_pubkey_sig_core.nim:305-414) for
every group, from oracle/bls12381_py.py alone:
value = final_exp(miller_loop([(pk_j, H(m_j)) ...] + [(-G1, sig)])), verdict = value == 1 and no pk_j is infinity (and the group is not empty).

Kinds: valid groups of 1, 2, 3, 5 and 9 pairs; a wrong message at one member; a signature that aggregates one key more than the group lists;
two members' messages exchanged (both members wrong alone, and the product wrong); a cancelling pair (the members' own signatures are s1 + D
and s2 - D: neither verifies alone, their aggregate does - verdict 1); an infinity public key (verdict 0 whatever the value; the value recorded
is that of the pairs that are left); an infinity signature; a repeated pair (the same (pk, m) twice, signed twice: valid).

Run:  python tests/golden/gen_aggregate_verify_each.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402


def fp12_image(a):
    """blst_fp12 image (576 B) of an oracle Fp12 value"""
    return b"".join(o.fp_to_mont_bytes(c[0]) + o.fp_to_mont_bytes(c[1]) for c in o.f12_to_tower_ints(a))


def agg(sigs):
    s = None
    for x in sigs:
        s = o.g2_add(s, x)
    return s


def main():
    shapes = [("valid", 1), ("valid", 2), ("valid", 3), ("valid", 5), ("valid", 9), ("wrong_message", 3), ("missing_member", 2),
              ("swapped_messages", 3), ("cancelling_pair", 2), ("infinity_public_key", 3), ("infinity_signature", 2), ("repeated_pair", 2)]
    neg_g1 = o.g1_neg(o.G1_GEN)
    groups, seed = [], 2000
    for gi, (kind, t) in enumerate(shapes):
        keys = [o.keygen_seed(seed + j) for j in range(t + 1)]                 # (pk, sk); one spare
        seed += t + 1
        msgs = [hashlib.sha256(b"aggregate_verify_each fixture %d %d" % (gi, j)).digest() for j in range(t + 1)]
        pks = [k[0] for k in keys[:t]]
        if kind == "repeated_pair":
            keys[1], msgs[1], pks[1] = keys[0], msgs[0], pks[0]
        member_sigs = [o.sign(keys[j][1], msgs[j]) for j in range(t)]
        extra = {}
        if kind == "cancelling_pair":
            d = o.g2_mul(o.hash_to_g2(b"a point nobody signed"), 7)
            member_sigs = [o.g2_add(member_sigs[0], d), o.g2_add(member_sigs[1], o.g2_neg(d))]
            for j in range(2):
                assert not o.core_verify(pks[j], msgs[j], member_sigs[j])
            extra["member_signatures"] = b"".join(o.g2_to_blst_affine(s) for s in member_sigs).hex()
        sig = agg(member_sigs)
        msgs = msgs[:t]
        if kind == "wrong_message":
            msgs[1] = hashlib.sha256(b"another message").digest()
        elif kind == "missing_member":
            sig = o.g2_add(sig, o.sign(keys[t][1], hashlib.sha256(b"the member that is not listed").digest()))
        elif kind == "swapped_messages":
            msgs[0], msgs[2] = msgs[2], msgs[0]
            for j in (0, 2):
                assert not o.core_verify(pks[j], msgs[j], member_sigs[j])
        elif kind == "infinity_public_key":
            sig = agg([member_sigs[0], member_sigs[2]])
            pks[1] = None
        elif kind == "infinity_signature":
            sig = None
        v = o.final_exp(o.miller_loop([(pk, o.hash_to_g2(m)) for pk, m in zip(pks, msgs)] + [(neg_g1, sig)]))
        ok = v == o.F12_ONE and all(pk is not None for pk in pks)
        if all(pk is not None for pk in pks):
            assert ok == o.aggregate_verify(pks, msgs, sig)
        assert ok == (kind in ("valid", "cancelling_pair", "repeated_pair")), (gi, kind, ok)
        if kind == "infinity_public_key":
            assert v == o.F12_ONE                                              # the pairs that are left verify: only the key's rule fails the group
        groups.append(dict({"kind": kind, "pks": b"".join(o.g1_to_blst_affine(pk) for pk in pks).hex(), "msgs": b"".join(msgs).hex(),
                            "sig": o.g2_to_blst_affine(sig).hex(), "verdict": int(ok), "gt": fp12_image(v).hex()}, **extra))
        print("group", gi, kind, t, int(ok), flush=True)
    out = {"comment": "tests/golden/gen_aggregate_verify_each.py: per-group verdict and final_exp value (blst_fp12 image) from oracle/bls12381_py.py",
           "groups": groups}
    with open(os.path.join(HERE, "aggregate_verify_each.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", len(groups), "groups")


if __name__ == "__main__":
    main()
