"""The inputs the CPU and GPU tests of the key table share: tests/golden/key_table.json (tests/golden/gen_key_table.py) laid out as
mi355_bls_admit_keys takes it, and the key encodings of tests/golden/deser_adversarial.json with the oracle's verdict on each."""
import bls12381_py as o
import deser_cases as dc
from util import golden

KEY_BAD_PROOF = 8


def fixture():
    return golden("key_table")


def admit_inputs(pku, sgu, fx=None):
    """the fixture's rows that apply to the wire-form combination -> (kinds, keys, proofs, expected status bytes, expected 96-byte table)"""
    fx = fx or fixture()
    kinds, pk, pr, st, img = [], [], [], [], []
    for r in fx["rows"]:
        kb, pb = dc.wire(r["pk"], "pk", pku), dc.wire(r["proof"], "sig", sgu)
        if kb is None or pb is None:
            continue
        kinds.append(r["kind"]); pk.append(kb); pr.append(pb); st.append(r["status"]); img.append(bytes.fromhex(r["image"]))
    return kinds, b"".join(pk), b"".join(pr), bytes(st), b"".join(img)


def adversarial_keys(unc):
    """[(name, wire bytes)] of every key encoding the adversarial rows use that has this wire form (deser_cases.wire), in fixture order"""
    fx = dc.fixture()
    names = []
    for r in fx["rows"]:
        if r["pk"] not in names:
            names.append(r["pk"])
    out = []
    for nm in names:
        b = dc.wire(fx["enc"][nm], "pk", unc)
        if b is not None:
            out.append((nm, b))
    return out


def oracle_key(b, unc, known):
    """PublicKey.fromBytes / fromBytesKnownOnCurve of one encoding by the big-integer definitions -> (status, 96-byte image, all zero unless 0)"""
    ok, pt = dc.decode("pk", b, unc)
    st = 1 if not ok else 3 if pt is None else 2 if (not known and not dc.in_subgroup("pk", pt)) else 0
    return st, (o.g1_to_blst_affine(pt) if st == 0 else bytes(96))


def key_layout(unc, valid):
    """The decoder's batch of one wire form: the adversarial key encodings with the valid keys (wire bytes in the same form) spread evenly
    between them, as deser_cases.layout spreads tuples, and a count that is no multiple of 64.  -> [(name or None, key bytes)]"""
    rows = adversarial_keys(unc)
    out, v = [], 0
    for j, (nm, b) in enumerate(rows):
        while v * len(rows) <= j * len(valid) and v < len(valid):
            out.append((None, valid[v]))
            v += 1
        out.append((nm, b))
    out += [(None, k) for k in valid[v:]]
    if len(out) % 64 == 0:
        out.append((None, valid[0]))
    return out
