"""The adversarial fromBytes rows of tests/golden/deser_adversarial.json (tests/golden/gen_deser_adversarial.py): loading, the status of a
tuple under the big-integer definitions (decode by square root, membership by [r]P == infinity; oracle/bls12381_py.py only), and the batch
layout the CPU and GPU tests share.

A row names one key encoding and one signature encoding.  An encoding has a compressed form (48 / 96 bytes), an uncompressed form (96 / 192
bytes) or both; both forms of one encoding hold the same point.  Where only the compressed form exists, the uncompressed entry points are fed
that form followed by zeros: blst_pN_deserialize reads a first half with the top bit set as a compressed point and nothing after it.  A row
whose encoding has only the uncompressed form applies to the uncompressed wire form alone."""
import hashlib

import bls12381_py as o
from util import golden

PK_UNCOMPRESSED, SIG_UNCOMPRESSED, KNOWN_ON_CURVE = 1, 2, 4
COMBOS = ((False, False), (True, False), (False, True), (True, True))        # (keys uncompressed, signatures uncompressed)


def fixture():
    return golden("deser_adversarial")


def wire(enc, side, unc):
    """the bytes of encoding `enc` ({"c": hex | None, "u": hex | None}) for the wire form, or None when the row does not apply to it"""
    full = (96 if side == "pk" else 192)
    if not unc:
        return bytes.fromhex(enc["c"]) if enc.get("c") else None
    if enc.get("u"):
        return bytes.fromhex(enc["u"])
    c = bytes.fromhex(enc["c"])
    return c + bytes(full - len(c))


def decode(side, b, unc):
    """-> (ok, point or None): the oracle's decode step of one side"""
    try:
        if side == "pk":
            return True, (o.g1_deserialize(b) if unc else o.g1_decompress(b))
        return True, (o.g2_deserialize(b) if unc else o.g2_decompress(b))
    except ValueError:
        return False, None


_member = {}


def in_subgroup(side, pt):
    """[r]P == infinity, remembered per point (the tests ask for the same points under every wire form)"""
    key = (side, pt)
    if key not in _member:
        _member[key] = (o.g1_mul(pt, o.R) is None) if side == "pk" else (o.g2_mul(pt, o.R) is None)
    return _member[key]


def oracle_status(pkb, pku, sgb, sgu, known):
    """fromBytes / fromBytesKnownOnCurve of one tuple (bls_sig_io.nim:42-121): the status byte of include/blscurve_mi355x.h"""
    ok, pk = decode("pk", pkb, pku)
    if not ok:
        return 1
    if pk is None:
        return 3
    if not known and not in_subgroup("pk", pk):
        return 2
    ok, sg = decode("sig", sgb, sgu)
    if not ok:
        return 4
    if not known and sg is not None and not in_subgroup("sig", sg):
        return 5
    return 0


def oracle_record(pkb, pku, msg, sgb, sgu):
    """the 320-byte SignatureSet image of a tuple that decodes"""
    return o.signature_set_bytes(decode("pk", pkb, pku)[1], msg, decode("sig", sgb, sgu)[1])


def message(i):
    return hashlib.sha256(b"deser adversarial %d" % i).digest()


def rows_for(fx, pku, sgu):
    """[(row index, key bytes, signature bytes)] of the rows that apply to the wire-form combination"""
    out = []
    for i, r in enumerate(fx["rows"]):
        pkb, sgb = wire(fx["enc"][r["pk"]], "pk", pku), wire(fx["enc"][r["sig"]], "sig", sgu)
        if pkb is not None and sgb is not None:
            out.append((i, pkb, sgb))
    return out


def layout(fx, pku, sgu, valid):
    """The batch of one wire-form combination: the fixture's rows with the valid tuples spread evenly between them, so that hostile and valid
    lanes sit side by side in every wave, and a count that is no multiple of 64.  valid: [(key bytes, signature bytes)] in the same wire forms.
    -> [(row index or None, key bytes, message, signature bytes)]"""
    rows = rows_for(fx, pku, sgu)
    out, v = [], 0
    for j, (i, pkb, sgb) in enumerate(rows):
        while v * len(rows) <= j * len(valid) and v < len(valid):              # valid tuple v goes in front of row v * len(rows) / len(valid)
            out.append((None,) + valid[v])
            v += 1
        out.append((i, pkb, sgb))
    out += [(None,) + t for t in valid[v:]]
    if len(out) % 64 == 0:                                                      # the tail wave must be partial
        out.append((None,) + valid[0])
    return [(i, pkb, message(k), sgb) for k, (i, pkb, sgb) in enumerate(out)]


def compress_boundary_images():
    """(x, y) images for g1_compress at the boundary of "y is the larger root": not curve points - the compress calls take images as they are"""
    xs = (0, 1, o.P - 1, o.G1_GEN[0], (o.P - 1) // 2)
    ys = (1, (o.P - 1) // 2, (o.P + 1) // 2, o.P - 1)
    return [(x, y) for x in xs for y in ys]


def compress_boundary_expect(x, y):
    """the integer rule, written out: canonical big-endian x, bit 383 set, bit 381 set iff y > p - y"""
    return (x | (1 << 383) | ((1 << 381) if y > o.P - y else 0)).to_bytes(48, "big")
