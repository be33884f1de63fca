#!/usr/bin/env python3
"""Generates tests/golden/key_table.json: (public key, proof of possession) rows in their WIRE forms with the status key admission must give
them (mi355_bls_admit_keys) and the 96-byte blst_p1_affine image an admitted key leaves in the table, from oracle/bls12381_py.py alone.

status = the first that applies of
    1  the key does not decode (flags, x >= p, not on the curve)           PublicKey.fromBytes (bls_sig_io.nim:81-99)
    3  the key is the point at infinity
    2  [r]key != infinity
    4  the proof does not decode                                           Signature.fromBytes (:42-58)
    5  the proof is not infinity and [r]proof != infinity
    8  both decode and popVerify(key, proof) is false (the infinity proof included)   popVerify (bls_sig_min_pubkey.nim:60-74)
    0  admitted
by the big-integer definitions only: decode by square root, membership by [r]P == infinity, o.pop_verify.

Rows:
  pop      the twelve pairs of tests/golden/pop.json in wire form, kinds kept (valid, other-key proof, doubled proof, infinity proof, infinity
           key, swapped proofs)
  key      every KEY encoding of tests/golden/deser_adversarial.json, each with a valid proof - of some other key
  proof    valid keys with adversarial SIGNATURE encodings of that fixture (bad flags, x >= p, on the curve outside G2) and two made here
           (x on no curve point, compressed and uncompressed)
  valid    two more valid pairs, one per sign of the key's y
An encoding has a compressed form ("c": 48 / 96 bytes), an uncompressed form ("u": 96 / 192 bytes) or both; both forms of one encoding hold
the same point and get the same status (asserted).  Where only the compressed form exists the uncompressed entry points are fed that form
followed by zeros (tests/deser_cases.py wire); a row with an encoding that has only the uncompressed form applies to that wire form alone.

Run:  python tests/golden/gen_key_table.py      (pure Python, about two minutes).  Reproducible byte for byte: no clock, no `random`.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

PROOF_ENCODINGS = ("g2_inf_signbit", "g2_inf_payload", "g2_unc_0x60", "g2_xc0_bit383", "g2_xc0_bit382", "g2_xc1_p", "g2_xc0_p", "g2_unc_yc0_p",
                   "g2_unc_y0", "g2_unc_negy", "g2_ord13_0_pos", "g2_ord13_0_neg", "g2_ord2713_0_pos", "g2_G_plus_ord13_pos", "g2_G_plus_ord2713_neg",
                   "g2_y_c1zero_0_pos", "g2_y_c0zero_0_neg")


def forms(enc, full):
    """[(uncompressed?, bytes)] of the wire forms an encoding applies to"""
    out = []
    if enc.get("c"):
        c = bytes.fromhex(enc["c"])
        out.append((False, c))
        if not enc.get("u"):
            out.append((True, c + bytes(full - len(c))))
    if enc.get("u"):
        out.append((True, bytes.fromhex(enc["u"])))
    return out


def decode(side, b, unc):
    try:
        if side == "pk":
            return True, (o.g1_deserialize(b) if unc else o.g1_decompress(b))
        return True, (o.g2_deserialize(b) if unc else o.g2_decompress(b))
    except ValueError:
        return False, None


_pop = {}


def pop_ok(pk, proof):
    if (pk, proof) not in _pop:
        _pop[(pk, proof)] = bool(o.pop_verify(pk, proof))
    return _pop[(pk, proof)]


def status_of(pkb, pku, prb, pru):
    """-> (status, key point)"""
    ok, pk = decode("pk", pkb, pku)
    if not ok:
        return 1, None
    if pk is None:
        return 3, None
    if o.g1_mul(pk, o.R) is not None:
        return 2, None
    ok, pr = decode("sig", prb, pru)
    if not ok:
        return 4, None
    if pr is not None and o.g2_mul(pr, o.R) is not None:
        return 5, None
    if pr is None or not pop_ok(pk, pr):
        return 8, None
    return 0, pk


def row(kind, pk_enc, proof_enc):
    """status and image of a row under every wire-form combination it applies to: they must agree"""
    got = set()
    for pku, pkb in forms(pk_enc, 96):
        for pru, prb in forms(proof_enc, 192):
            st, pk = status_of(pkb, pku, prb, pru)
            got.add((st, o.g1_to_blst_affine(pk).hex() if st == 0 else bytes(96).hex()))
    assert len(got) == 1, (kind, got)
    st, img = got.pop()
    return {"kind": kind, "pk": pk_enc, "proof": proof_enc, "status": st, "image": img}


def off_curve_proof(proof):
    """the compressed form of `proof` with x.c0 stepped until x is on no curve point, and that x with some y < p as an uncompressed form"""
    (x0, x1), _ = proof
    while True:
        x0 += 1
        b = (x1 | (1 << 383)).to_bytes(48, "big") + x0.to_bytes(48, "big")
        if not decode("sig", b, False)[0]:
            assert x0 < o.P
            return b, x1.to_bytes(48, "big") + x0.to_bytes(48, "big") + (5).to_bytes(48, "big") + (7).to_bytes(48, "big")


def main():
    pop = json.load(open(os.path.join(HERE, "pop.json")))
    adv = json.load(open(os.path.join(HERE, "deser_adversarial.json")))
    rows = []
    for c in pop["cases"]:
        pk, pr = o.g1_from_blst_affine(bytes.fromhex(c["pk"])), o.g2_from_blst_affine(bytes.fromhex(c["proof"]))
        rows.append(row("pop_" + c["kind"], {"c": o.g1_compress(pk).hex(), "u": o.g1_serialize(pk).hex()}, {"c": o.g2_compress(pr).hex(), "u": o.g2_serialize(pr).hex()}))
        assert (rows[-1]["status"] == 0) == bool(c["verdict"]), c["kind"]
        assert rows[-1]["status"] == {"valid": 0, "infinity_key": 3}.get(c["kind"], 8), c["kind"]
    # a valid proof of some OTHER key beside every adversarial key encoding
    other = o.pop_prove(o.keygen_seed(3000)[1])
    other_enc = {"c": o.g2_compress(other).hex(), "u": o.g2_serialize(other).hex()}
    names = []
    for r in adv["rows"]:
        if r["pk"] not in names:
            names.append(r["pk"])
    for nm in names:
        rows.append(row("key_" + nm, adv["enc"][nm], other_enc))
        assert rows[-1]["status"] in (1, 2, 3, 8), nm                 # a key that decodes into G1 is refused for its proof
    # valid keys beside adversarial proof encodings
    sks = [o.keygen_seed(3100 + i)[1] for i in range(len(PROOF_ENCODINGS) + 2)]
    pk_encs = [{"c": o.g1_compress(o.sk_to_pk(sk)).hex(), "u": o.g1_serialize(o.sk_to_pk(sk)).hex()} for sk in sks]
    for k, nm in enumerate(PROOF_ENCODINGS):
        rows.append(row("proof_" + nm, pk_encs[k], adv["enc"][nm]))
        assert rows[-1]["status"] in (4, 5, 8), nm                    # 8: an encoding that decodes into G2 (the negated y) is some signature, not this key's proof
    oc, ou = off_curve_proof(o.pop_prove(sks[-2]))
    rows.append(row("proof_off_curve_c", pk_encs[-2], {"c": oc.hex(), "u": None}))
    rows.append(row("proof_off_curve_u", pk_encs[-1], {"c": None, "u": ou.hex()}))
    assert rows[-1]["status"] == rows[-2]["status"] == 4
    # both signs of y among the admitted keys: the first seeded key of either sign, with its own proof
    want, seed = {0, 1}, 3200
    while want:
        sk = o.keygen_seed(seed)[1]
        seed += 1
        pk = o.sk_to_pk(sk)
        sign = o.g1_compress(pk)[0] >> 5 & 1
        if sign in want:
            want.discard(sign)
            pr = o.pop_prove(sk)
            rows.append(row("valid_y_sign%d" % sign, {"c": o.g1_compress(pk).hex(), "u": o.g1_serialize(pk).hex()}, {"c": o.g2_compress(pr).hex(), "u": o.g2_serialize(pr).hex()}))
            assert rows[-1]["status"] == 0
    have = {r["status"] for r in rows}
    assert have == {0, 1, 2, 3, 4, 5, 8}, have
    signs = {int(r["pk"]["c"][:2], 16) >> 5 & 1 for r in rows if r["status"] == 0}
    assert signs == {0, 1}, signs                                      # both signs of y among the admitted keys
    out = {"comment": "tests/golden/gen_key_table.py: (key, proof) rows in wire form (c = compressed, u = uncompressed), the status of key admission and the "
                      "admitted key's blst_p1_affine image (all zero when refused), from oracle/bls12381_py.py",
           "rows": rows}
    path = os.path.join(HERE, "key_table.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(HERE, n)) for n in os.listdir(HERE) if n != "key_table.json")
    print("wrote", len(rows), "rows; statuses", sorted(have))


if __name__ == "__main__":
    main()
