#!/usr/bin/env python3
"""Generates tests/golden/pop.json: twelve (public key, proof of possession) pairs with the verdict and value of
popVerify = coreVerifyNoGroupCheck(pk, compress(pk), proof, DST_POP) (bls_sig_min_pubkey.nim:60-74), from oracle/bls12381_py.py alone:
value = final_exp(miller_loop([(pk, H_pop(compress(pk))), (-G1, proof)])), verdict = value == 1 and pk is not infinity.

Keys: the reference's three (sk, pk, proof) vectors (tests/eth2_vectors.nim:33-47) and nine from keygen_seed.  Kinds: valid pairs; a proof made
by another key; [2] * (valid proof); an infinity proof (the pair is skipped: the value is e(pk, H), verdict 0); an infinity key (verdict 0
whatever the value; its message is the compression of infinity, 0xc0 00..00); two keys with their proofs swapped.

The valid pairs are also recorded as one batch under a fixed rnd: the blinding scalars (num_threads chains, as batchVerify draws them) and
final_exp(prod e([r_i]pk_i, H_i) * e(-G1, sum [r_i]proof_i)).

Run:  python tests/golden/gen_pop.py      (pure Python, about a minute).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

REFERENCE = [       # tests/eth2_vectors.nim:33-47: secret key, compressed public key, compressed proof
    ("263dbd792f5b1be47ed85f8938c0f29586af0d3ac7b977f21c278fe1462040e3",
     "a491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a",
     "b803eb0ed93ea10224a73b6b9c725796be9f5fefd215ef7a5b97234cc956cf6870db6127b7e4d824ec62276078e787db05584ce1adbf076bc0808ca0f15b73d59060254b25393d95dfc7abe3cda566842aaedf50bbb062aae1bbb6ef3b1f77e1"),
    ("47b8192d77bf871b62e87859d653922725724a5c031afeabc60bcef5ff665138",
     "b301803f8b5ac4a1133581fc676dfedc60d891dd5fa99028805e5ea5b08d3491af75d0707adab3b70c6a6a580217bf81",
     "88bb31b27eae23038e14f9d9d1b628a39f5881b5278c3c6f0249f81ba0deb1f68aa5f8847854d6554051aa810fdf1cdb02df4af7a5647b1aa4afb60ec6d446ee17af24a8a50876ffdaf9bf475038ec5f8ebeda1c1c6a3220293e23b13a9a5d26"),
    ("328388aff0d4a5b7dc9205abd374e7e98f3cd9f3418edb4eafda5fb16473d216",
     "b53d21a4cfd562c469cc81514d4ce5a6b577d8403d32a394dc265dd190b47fa9f829fdd7963afdf972e5e77854051f6f",
     "88873ea58f5017a33facc9bf04efaf5e2f34f7bc9ce564d0481dd469326c04ef43552f50e99de8a13315dcd37a4fb9ef036d1a54e5febf5d20b6aa488f3e3c917e6a96ce6461f609ec7e0a1fd8950380922e46c3654fa7542436603f833462da"),
]
NUM_THREADS = 4


def fp12_image(a):
    """blst_fp12 image (576 B) of an oracle Fp12 value"""
    return b"".join(o.fp_to_mont_bytes(c[0]) + o.fp_to_mont_bytes(c[1]) for c in o.f12_to_tower_ints(a))


def main():
    sks = [int(r[0], 16) for r in REFERENCE] + [o.keygen_seed(2000 + i)[1] for i in range(9)]
    pks = [o.sk_to_pk(sk) for sk in sks]
    proofs = [o.pop_prove(sk) for sk in sks]
    for i, (_, pk, proof) in enumerate(REFERENCE):
        assert o.g1_compress(pks[i]).hex() == pk and o.g2_compress(proofs[i]).hex() == proof
    # both signs of y among the keys: bit 5 of byte 0 of the compressed form
    signs = {o.g1_compress(pk)[0] >> 5 & 1 for pk in pks}
    assert signs == {0, 1}, signs
    kinds = ["valid"] * 12
    proofs[4] = o.pop_prove(sks[3]); kinds[4] = "other_key_proof"
    proofs[5] = o.g2_mul(proofs[5], 2); kinds[5] = "doubled_proof"
    proofs[6] = None; kinds[6] = "infinity_proof"
    pks[7] = None; kinds[7] = "infinity_key"
    proofs[8], proofs[9] = proofs[9], proofs[8]; kinds[8] = kinds[9] = "swapped_proofs"
    neg_g1 = o.g1_neg(o.G1_GEN)
    cases, hs = [], []
    for i in range(12):
        comp = o.g1_compress(pks[i])
        h = o.hash_to_g2(comp, o.DST_POP)
        hs.append(h)
        v = o.final_exp(o.miller_loop([(pks[i], h), (neg_g1, proofs[i])]))
        ok = v == o.F12_ONE and pks[i] is not None
        assert ok == (o.pop_verify(pks[i], proofs[i]) if pks[i] is not None else False)
        assert ok == (kinds[i] == "valid"), (i, kinds[i], ok)
        cases.append({"kind": kinds[i], "reference": i < 3, "sk": "%064x" % sks[i], "pk": o.g1_to_blst_affine(pks[i]).hex(), "proof": o.g2_to_blst_affine(proofs[i]).hex(),
                      "compressed": comp.hex(), "verdict": int(ok), "gt": fp12_image(v).hex()})
    # the swapped pair is good as a product: an unblinded batch check would pass it
    both = o.miller_loop([(pks[8], hs[8]), (neg_g1, proofs[8]), (pks[9], hs[9]), (neg_g1, proofs[9])])
    assert o.final_exp(both) == o.F12_ONE
    # the valid pairs as one blinded batch
    good = [i for i in range(12) if cases[i]["verdict"]]
    rnd = hashlib.sha256(b"pop fixture rnd").digest()
    rs = o.blinding_scalars(rnd, len(good), NUM_THREADS)
    agg = None
    pairs = []
    for i, r in zip(good, rs):
        agg = o.g2_add(agg, o.g2_mul(proofs[i], r))
        pairs.append((o.g1_mul(pks[i], r), hs[i]))
    pairs.append((neg_g1, agg))
    gt = o.final_exp(o.miller_loop(pairs))
    assert gt == o.F12_ONE
    out = {"comment": "tests/golden/gen_pop.py: popVerify verdict and final_exp value (blst_fp12 image) per pair, and the valid pairs as one blinded batch, "
                      "from oracle/bls12381_py.py",
           "cases": cases,
           "batch": {"indices": good, "rnd": rnd.hex(), "num_threads": NUM_THREADS, "scalars": rs, "gt": fp12_image(gt).hex()}}
    with open(os.path.join(HERE, "pop.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", len(cases), "cases")


if __name__ == "__main__":
    main()
