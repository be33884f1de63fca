#!/usr/bin/env python3
"""Generates tests/golden/verify_each.json: twelve SignatureSet records with the per-set verdict and value of
verify = coreVerifyNoGroupCheck (bls_sig_min_pubkey.nim:108-125, blst_min_pubkey_sig_core.nim:269-297), from oracle/bls12381_py.py alone:
value = final_exp(miller_loop([(pk, H(msg)), (-G1, sig)])), verdict = value == 1 and pk is not infinity.

Kinds: valid sets; a wrong message; a signature made with another key; two sets with their signatures swapped - each bad on its own although
the product over both is one, which is what a batch check without blinding would pass; an infinity signature (the pair is skipped: the value is
e(pk, H), verdict 0); an infinity public key (verdict 0 whatever the value; the value recorded is e(-G1, sig), the pair that is left); a set
whose signature is [2] * (valid signature).

Run:  python tests/golden/gen_verify_each.py      (pure Python, about a minute).  Reproducible byte for byte: no clock, no `random`.
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


def main():
    keys = [o.keygen_seed(1000 + i) for i in range(12)]                    # (pk, sk)
    msgs = [hashlib.sha256(b"verify_each fixture %d" % i).digest() for i in range(12)]
    sigs = [o.sign(keys[i][1], msgs[i]) for i in range(12)]
    pks = [k[0] for k in keys]
    kinds = ["valid"] * 12
    msgs[2] = hashlib.sha256(b"another message").digest(); kinds[2] = "wrong_message"
    sigs[3] = o.sign(keys[4][1], msgs[3]); kinds[3] = "other_key"
    # same message, same key pair order swapped: sets 5 and 6 carry each other's signature
    sigs[5], sigs[6] = sigs[6], sigs[5]; kinds[5] = kinds[6] = "swapped_pair"
    sigs[7] = None; kinds[7] = "infinity_signature"
    pks[8] = None; kinds[8] = "infinity_public_key"
    sigs[9] = o.g2_mul(sigs[9], 2); kinds[9] = "doubled_signature"
    sets = []
    neg_g1 = o.g1_neg(o.G1_GEN)
    for i in range(12):
        f = o.miller_loop([(pks[i], o.hash_to_g2(msgs[i])), (neg_g1, sigs[i])])
        v = o.final_exp(f)
        ok = v == o.F12_ONE and pks[i] is not None
        assert ok == (o.core_verify(pks[i], msgs[i], sigs[i]) if pks[i] is not None else False)
        assert ok == (kinds[i] == "valid"), (i, kinds[i], ok)
        sets.append({"kind": kinds[i], "set": o.signature_set_bytes(pks[i], msgs[i], sigs[i]).hex(), "verdict": int(ok), "gt": fp12_image(v).hex()})
    # the swapped pair is good as a sum: the unblinded product over both sets is one
    both = o.miller_loop([(pks[5], o.hash_to_g2(msgs[5])), (neg_g1, sigs[5]), (pks[6], o.hash_to_g2(msgs[6])), (neg_g1, sigs[6])])
    assert o.final_exp(both) == o.F12_ONE
    out = {"comment": "tests/golden/gen_verify_each.py: per-set verdict and final_exp value (blst_fp12 image) from oracle/bls12381_py.py", "sets": sets}
    with open(os.path.join(HERE, "verify_each.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", len(sets), "sets")


if __name__ == "__main__":
    main()
