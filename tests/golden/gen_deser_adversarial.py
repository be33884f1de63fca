#!/usr/bin/env python3
"""Generates tests/golden/deser_adversarial.json: the encodings an attacker would hand to fromBytes (mi355_bls_deserialize_sets*,
mi355_bls_batch_verify_compressed*), with the status each tuple must get under the big-integer definitions - decode by square root,
membership by [r]P == infinity - from oracle/bls12381_py.py alone.

Families (the other side of the tuple is a valid point unless the row is a precedence row):
  g1_torsion   E(Fp) = Z_d x Z_{3 d r}, d = 11 * 10177 * 859267 * 52437899: the two points of order 3 (x = 0), two independent points of
               order l for every l | d (the whole l-torsion is rational, so phi acts on it as a 2 x 2 matrix), a point of order 33, and
               G1 points plus a point of order 3 / 11; every point with both signs
  g2_torsion   #E'(Fp2) = r * 13^2 * 23^2 * 2713 * 11953 * 262069 * c448 (found among the six CM candidates): two independent points of
               order 13 and of order 23, points of order 2713, 11953, 262069, 13 * 23 and c448, G2 points plus a torsion point
  fp2_sign     curve points of E' whose x^3 + 4(1 + u) lies in Fp: y = (a, 0) (the sign rule falls back to c0) or y = (0, b); both signs
  range        coordinates p - 1, p, p + 1, 2^381 - 1; the three top bits of x.c0 (no flags there); infinity encodings with the sign bit or
               a payload; 0x60...; uncompressed (x, 0), (x, p), (x, p - y) and (x, y + p)
  precedence   a bad key with a bad signature: the key's status wins

Every point's defining property is asserted here: on the curve, exact order (l prime, [l]P == infinity, P != infinity; independence of a
pair by baby-step giant-step), the zero component.  Per row the file holds the names of its two encodings and the status with
KNOWN_ON_CURVE off and on; each encoding is stored once, in the wire forms it has.  Records are not stored: the tests derive them
with the oracle's *_decompress / *_deserialize.

Run:  python tests/golden/gen_deser_adversarial.py      (pure Python, a few minutes).  Reproducible byte for byte from SEED.
"""
import json
import math
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import bls12381_py as o  # noqa: E402
import deser_cases as dc  # noqa: E402

SEED = 0x0BAD5EED
P = o.P
D_FACTORS = (11, 10177, 859267, 52437899)
D = math.prod(D_FACTORS)
N1 = o.H1 * o.R                                   # #E(Fp)
H2_SMALL = (13, 13, 23, 23, 2713, 11953, 262069)


def is_probable_prime(n, rng, rounds=40):
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(rounds):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def rand_g1(rng):
    while True:
        x = rng.randrange(P)
        y = o.fp_sqrt((x ** 3 + 4) % P)
        if y is not None:
            return (x, y if rng.getrandbits(1) else P - y)


def rand_g2(rng):
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = o.f2sqrt(o.f2add(o.f2mul(o.f2sqr(x), x), o.B2))
        if y is not None:
            return (x, y if rng.getrandbits(1) else o.f2neg(y))


def independent(add, mul, neg, p, q, l):
    """q is no multiple of p (both of prime order l): baby-step giant-step over k = i m + j"""
    m = math.isqrt(l) + 1
    baby, t = set(), None
    for _ in range(m):
        baby.add(t)
        t = add(t, p)
    step, s = neg(mul(p, m)), q
    for _ in range(m + 1):
        if s in baby:
            return False
        s = add(s, step)
    return True


def torsion(rng, rand, mul, cof, l, on_curve):
    """[cof] * random until it is not infinity; cof = #E / l^k kills everything but the l-part, which has exponent l"""
    while True:
        t = mul(rand(rng), cof)
        if t is not None:
            assert on_curve(t) and mul(t, l) is None
            return t


def twist_order(rng):
    """#E'(Fp2): the one of the six CM candidates that r divides and that annihilates a random point of E'"""
    t = P + 1 - N1
    t2 = t * t - 2 * P
    f = math.isqrt((4 * P * P - t2 * t2) // 3)
    assert 3 * f * f == 4 * P * P - t2 * t2
    assert (t2 + 3 * f) % 2 == 0
    traces = [t2, -t2, (t2 + 3 * f) // 2, -(t2 + 3 * f) // 2, (t2 - 3 * f) // 2, -(t2 - 3 * f) // 2]
    q = rand_g2(rng)
    good = [P * P + 1 - tr for tr in traces if (P * P + 1 - tr) % o.R == 0 and o.g2_mul(q, P * P + 1 - tr) is None]
    assert len(good) == 1, len(good)
    return good[0]


class Fixture:
    def __init__(self):
        self.enc, self.rows = {}, []

    def add(self, name, c=None, u=None):
        assert name not in self.enc, name
        self.enc[name] = {"c": c.hex() if c is not None else None, "u": u.hex() if u is not None else None}
        return name

    def g1(self, name, p):
        assert o.g1_on_curve(p) and p is not None
        return self.add(name, o.g1_compress(p), o.g1_serialize(p))

    def g2(self, name, q):
        assert o.g2_on_curve(q) and q is not None
        return self.add(name, o.g2_compress(q), o.g2_serialize(q))

    def row(self, family, pk, sig, expect=None):
        """status under every wire form the row applies to (they must agree), KNOWN_ON_CURVE off and on"""
        st, nonmember = None, False
        for pku, sgu in dc.COMBOS:
            pkb, sgb = dc.wire(self.enc[pk], "pk", pku), dc.wire(self.enc[sig], "sig", sgu)
            if pkb is None or sgb is None:
                continue
            got = [dc.oracle_status(pkb, pku, sgb, sgu, known) for known in (False, True)]
            assert st is None or st == got, (family, pk, sig, st, got)
            st = got
            for side, b, unc in (("pk", pkb, pku), ("sig", sgb, sgu)):
                ok, pt = dc.decode(side, b, unc)
                nonmember |= ok and pt is not None and not dc.in_subgroup(side, pt)
        assert st is not None and (expect is None or st == expect), (family, pk, sig, st, expect)
        self.rows.append({"family": family, "pk": pk, "sig": sig, "st": st, "nonmember": nonmember})


def g1_torsion_rows(fx, rng):
    fams = {}
    t3 = (0, 2)
    assert o.g1_on_curve(t3) and o.g1_mul(t3, 3) is None
    assert o.g1_compress(t3) == bytes([0x80]) + bytes(47) and o.g1_compress(o.g1_neg(t3)) == bytes([0xa0]) + bytes(47)
    fams[3] = [t3]
    for l in D_FACTORS:
        assert o.g1_mul(rand_g1(rng), N1 // l) is None                 # the l-part has exponent l although l^2 | #E: rank 2
        a = torsion(rng, rand_g1, o.g1_mul, N1 // (l * l), l, o.g1_on_curve)
        while True:
            b = torsion(rng, rand_g1, o.g1_mul, N1 // (l * l), l, o.g1_on_curve)
            if independent(o.g1_add, o.g1_mul, o.g1_neg, a, b, l):
                break
        fams[l] = [a, b]
    t33 = o.g1_add(t3, fams[11][0])
    assert o.g1_mul(t33, 33) is None and o.g1_mul(t33, 3) is not None and o.g1_mul(t33, 11) is not None
    fams[33] = [t33]
    g = o.g1_mul(o.G1_GEN, rng.randrange(1, o.R))
    assert o.g1_in_subgroup(g)
    named = [("g1_ord%d_%d" % (l, i), t) for l, ts in fams.items() for i, t in enumerate(ts)]
    named += [("g1_G_plus_ord3", o.g1_add(g, t3)), ("g1_G_plus_ord11", o.g1_add(g, fams[11][1]))]
    for name, t in named:
        for sign, pt in (("pos", t), ("neg", o.g1_neg(t))):
            assert not o.g1_in_subgroup(pt)
            fx.row("g1_torsion", fx.g1(name + "_" + sign, pt), "good_sig", expect=[2, 0])
    return fams


def g2_torsion_rows(fx, rng):
    n2 = twist_order(rng)
    h2 = n2 // o.R
    c448 = h2 // math.prod(H2_SMALL)
    assert c448 * math.prod(H2_SMALL) == h2 and c448.bit_length() == 448 and is_probable_prime(c448, rng)
    assert math.gcd(c448, math.prod(H2_SMALL) * o.R) == 1
    fams = {}
    for l in (13, 23):
        assert o.g2_mul(rand_g2(rng), n2 // l) is None                 # rank 2, as on E(Fp)
        a = torsion(rng, rand_g2, o.g2_mul, n2 // (l * l), l, o.g2_on_curve)
        while True:
            b = torsion(rng, rand_g2, o.g2_mul, n2 // (l * l), l, o.g2_on_curve)
            if independent(o.g2_add, o.g2_mul, o.g2_neg, a, b, l):
                break
        fams[l] = [a, b]
    for l in (2713, 11953, 262069, c448):
        fams[l] = [torsion(rng, rand_g2, o.g2_mul, n2 // l, l, o.g2_on_curve)]
    t299 = o.g2_add(fams[13][0], fams[23][1])
    assert o.g2_mul(t299, 299) is None and o.g2_mul(t299, 13) is not None and o.g2_mul(t299, 23) is not None
    g = o.g2_mul(o.G2_GEN, rng.randrange(1, o.R))
    assert o.g2_in_subgroup(g)
    named = [("g2_ord%s_%d" % ("c448" if l == c448 else l, i), t) for l, ts in fams.items() for i, t in enumerate(ts)]
    named += [("g2_ord299_0", t299), ("g2_G_plus_ord13", o.g2_add(g, fams[13][1])), ("g2_G_plus_ord2713", o.g2_add(g, fams[2713][0]))]
    for name, t in named:
        for sign, pt in (("pos", t), ("neg", o.g2_neg(t))):
            assert not o.g2_in_subgroup(pt)
            fx.row("g2_torsion", "good_pk", fx.g2(name + "_" + sign, pt), expect=[5, 0])
    return fams


def fp2_sign_rows(fx, rng):
    """x = (x0, x1) with x0^2 = (x1^3 - 4) / (3 x1): the imaginary part of x^3 + 4(1 + u) vanishes, the real part is s + 4 with
    s = x0^3 - 3 x0 x1^2.  p = 3 mod 4, so exactly one of s + 4, -(s + 4) is a square: y = (a, 0) or y = (0, b)."""
    found = {"c1zero": [], "c0zero": []}
    while min(len(v) for v in found.values()) < 3:
        x1 = rng.randrange(1, P)
        x0 = o.fp_sqrt((x1 ** 3 - 4) * o.fp_inv(3 * x1) % P)
        if x0 is None:
            continue
        if rng.getrandbits(1):
            x0 = P - x0
        c = (x0 ** 3 - 3 * x0 * x1 * x1 + 4) % P
        assert o.f2add(o.f2mul(o.f2sqr((x0, x1)), (x0, x1)), o.B2) == (c, 0) and c != 0
        a = o.fp_sqrt(c)
        if a is not None:
            kind, y = "c1zero", (a, 0)
        else:
            kind, y = "c0zero", (0, o.fp_sqrt(-c % P))
        if len(found[kind]) < 3:
            found[kind].append(((x0, x1), y))
    for kind, pts in found.items():
        for i, q in enumerate(pts):
            for sign, pt in (("pos", q), ("neg", o.g2_neg(q))):
                assert o.g2_on_curve(pt) and pt[1][0 if kind == "c0zero" else 1] == 0 and pt[1][1 if kind == "c0zero" else 0] != 0
                assert o.g2_decompress(o.g2_compress(pt)) == pt and o.g2_deserialize(o.g2_serialize(pt)) == pt
                fx.row("fp2_sign", "good_pk", fx.g2("g2_y_%s_%d_%s" % (kind, i, sign), pt), expect=[0 if o.g2_in_subgroup(pt) else 5, 0])
    # the two signs of one point differ in the sign bit alone
    for kind in found:
        a, b = (bytes.fromhex(fx.enc["g2_y_%s_0_%s" % (kind, s)]["c"]) for s in ("pos", "neg"))
        assert a[0] ^ b[0] == 0x20 and a[1:] == b[1:]


def be(v):
    return v.to_bytes(48, "big")


def range_rows(fx, rng, good_pk, good_sig):
    top = 1 << 383
    # G1 x at and around p
    for name, xv in (("pm1", P - 1), ("p", P), ("pp1", P + 1), ("2e381m1", (1 << 381) - 1)):
        fx.row("range", fx.add("g1_x_" + name, c=be(xv | top)), "good_sig", expect=None if xv < P else [1, 1])
    fx.row("range", fx.add("g1_x_pm1_signbit", c=be((P - 1) | top | (1 << 381))), "good_sig")
    # G2: one component p - 1 (the other searched so that the point exists: the decode must get as far as the square root), then p
    def companion(fixed_c1, v):
        k = 0
        while True:
            x = (k, v) if fixed_c1 else (v, k)
            if o.f2sqrt(o.f2add(o.f2mul(o.f2sqr(x), x), o.B2)) is not None:
                return k
            k += 1
    k0 = companion(True, P - 1)
    fx.row("range", "good_pk", fx.add("g2_xc1_pm1", c=be((P - 1) | top) + be(k0)), expect=[5, 0])
    fx.row("range", "good_pk", fx.add("g2_xc1_p", c=be(P | top) + be(k0)), expect=[4, 4])
    k1 = companion(False, P - 1)
    fx.row("range", "good_pk", fx.add("g2_xc0_pm1", c=be(k1 | top) + be(P - 1)), expect=[5, 0])
    fx.row("range", "good_pk", fx.add("g2_xc0_p", c=be(k1 | top) + be(P)), expect=[4, 4])
    # the three top bits of x.c0 are not flags: rejected, not masked
    sc, su = o.g2_compress(good_sig), o.g2_serialize(good_sig)
    for bit in (0x80, 0x40, 0x20):
        c, u = bytearray(sc), bytearray(su)
        assert not c[48] & 0xe0 and c[48:96] == u[48:96]
        c[48] |= bit
        u[48] |= bit
        fx.row("range", "good_pk", fx.add("g2_xc0_bit%d" % {0x80: 383, 0x40: 382, 0x20: 381}[bit], c=bytes(c), u=bytes(u)), expect=[4, 4])
    # infinity encodings
    fx.row("range", fx.add("g1_inf", c=bytes([0xc0]) + bytes(47), u=bytes([0x40]) + bytes(95)), "good_sig", expect=[3, 3])
    fx.row("range", "good_pk", fx.add("g2_inf", c=bytes([0xc0]) + bytes(95), u=bytes([0x40]) + bytes(191)), expect=[0, 0])
    fx.row("range", fx.add("g1_inf_signbit", c=bytes([0xe0]) + bytes(47)), "good_sig", expect=[1, 1])
    fx.row("range", fx.add("g1_inf_payload", c=bytes([0xc0]) + bytes(46) + b"\x01"), "good_sig", expect=[1, 1])
    fx.row("range", "good_pk", fx.add("g2_inf_signbit", c=bytes([0xe0]) + bytes(95)), expect=[4, 4])
    fx.row("range", "good_pk", fx.add("g2_inf_payload", c=bytes([0xc0]) + bytes(94) + b"\x01"), expect=[4, 4])
    fx.row("range", fx.add("g1_unc_0x60", u=bytes([0x60]) + bytes(95)), "good_sig", expect=[1, 1])
    fx.row("range", "good_pk", fx.add("g2_unc_0x60", u=bytes([0x60]) + bytes(191)), expect=[4, 4])
    # uncompressed y = 0 and y = p under an x of the curve
    gx, gy = good_pk
    (sx0, sx1), (sy0, sy1) = good_sig
    fx.row("range", fx.add("g1_unc_y0", u=be(gx) + be(0)), "good_sig", expect=[1, 1])
    fx.row("range", fx.add("g1_unc_yp", u=be(gx) + be(P)), "good_sig", expect=[1, 1])
    fx.row("range", "good_pk", fx.add("g2_unc_y0", u=be(sx1) + be(sx0) + be(0) + be(0)), expect=[4, 4])
    fx.row("range", "good_pk", fx.add("g2_unc_yp", u=be(sx1) + be(sx0) + be(P) + be(P)), expect=[4, 4])
    fx.row("range", "good_pk", fx.add("g2_unc_yc0_p", u=be(sx1) + be(sx0) + be(sy1) + be(P)), expect=[4, 4])
    # y replaced by p - y (the negated point: valid) and by y + p (the same residue, not canonical: >= p).  y + p < 2^381 keeps the three
    # top bits clear, so the range check and not the flag handling must reject it; y + p < 2 p < 2^382 always fits the 48 bytes.
    lim = (1 << 381) - P
    fx.row("range", fx.add("g1_unc_negy", u=be(gx) + be(P - gy)), "good_sig", expect=[0, 0])
    k = 2
    while True:
        x, y = o.g1_mul(o.G1_GEN, k)
        y = min(y, P - y)
        if y < lim:
            break
        k += 1
    fx.row("range", fx.add("g1_unc_y_canonical", u=be(x) + be(y)), "good_sig", expect=[0, 0])
    fx.row("range", fx.add("g1_unc_y_plus_p", u=be(x) + be(y + P)), "good_sig", expect=[1, 1])
    fx.row("range", "good_pk", fx.add("g2_unc_negy", u=be(sx1) + be(sx0) + be(-sy1 % P) + be(-sy0 % P)), expect=[0, 0])
    k = 2
    while True:
        (x0, x1), (y0, y1) = o.g2_mul(o.G2_GEN, k)
        if y0 >= lim and y1 >= lim:
            y0, y1 = P - y0, P - y1
        if y0 < lim and y1 < lim:
            break
        k += 1
    fx.row("range", "good_pk", fx.add("g2_unc_y_canonical", u=be(x1) + be(x0) + be(y1) + be(y0)), expect=[0, 0])
    fx.row("range", "good_pk", fx.add("g2_unc_yc1_plus_p", u=be(x1) + be(x0) + be(y1 + P) + be(y0)), expect=[4, 4])
    fx.row("range", "good_pk", fx.add("g2_unc_yc0_plus_p", u=be(x1) + be(x0) + be(y1) + be(y0 + P)), expect=[4, 4])


def precedence_rows(fx):
    keys = {1: "g1_inf_signbit", 2: "g1_ord11_0_pos", 3: "g1_inf"}
    sigs = {4: "g2_inf_signbit", 5: "g2_ord13_0_pos"}
    for ks, kn in keys.items():
        for ss, sn in sigs.items():
            on = ks if ks != 2 else (4 if ss == 4 else 0)           # KNOWN_ON_CURVE: the torsion key passes, the torsion signature too
            fx.row("precedence", kn, sn, expect=[ks, on])


def main():
    rng = random.Random(SEED)
    assert o.H1 == 3 * D * D and N1 % (3 * D * D * o.R) == 0
    fx = Fixture()
    good_pk = o.g1_mul(o.G1_GEN, rng.randrange(1, o.R))
    good_sig = o.g2_mul(o.G2_GEN, rng.randrange(1, o.R))
    fx.g1("good_pk", good_pk)
    fx.g2("good_sig", good_sig)
    fx.row("valid", "good_pk", "good_sig", expect=[0, 0])
    g1_torsion_rows(fx, rng)
    g2_torsion_rows(fx, rng)
    fp2_sign_rows(fx, rng)
    range_rows(fx, rng, good_pk, good_sig)
    precedence_rows(fx)
    assert len(fx.rows) < 200
    out = {"comment": "tests/golden/gen_deser_adversarial.py: adversarial fromBytes encodings; st = status with KNOWN_ON_CURVE off, on under "
                      "the big-integer definitions (oracle/bls12381_py.py); enc: c = compressed, u = uncompressed wire form",
           "seed": SEED, "enc": fx.enc, "rows": fx.rows}
    with open(os.path.join(HERE, "deser_adversarial.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    fams = {}
    for r in fx.rows:
        fams[r["family"]] = fams.get(r["family"], 0) + 1
    print("wrote", len(fx.rows), "rows,", len(fx.enc), "encodings:", fams)


if __name__ == "__main__":
    main()
