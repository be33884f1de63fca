#!/usr/bin/env python3
"""Generates tests/golden/lincomb.json: groups of (point, scalar) terms on G1 and on G2 with the affine image of sum_p [s_p mod 2^nbits] P_p
and the status byte mi355_bls_p1s_lincomb_many / mi355_bls_p2s_lincomb_many give for each.  Only oracle/bls12381_py.py is used: g1_mul /
g2_mul / g1_add / g2_add over Python integers (the scalar is NEVER reduced mod r here: it acts as an integer), g2_psi for the check of the
base-X identity, the *_to_blst_affine images, and sswu_g2 / iso3_g2 for one G2 curve point outside the subgroup.

Per curve: `table` (entry 0 is the all-zero infinity image; G2's last entry is the point outside G2) and `groups`, each
  kind      a name
  terms     [[table index, scalar as 64 hex digits little-endian], ...]
  nbits     the nbits of the call this group belongs to (groups are called together per nbits value)
  psi       G2 only: the group may also run under LINCOMB_SUBGROUP (every point in G2); the expected image is the same
  out       the affine image, hex (all zero: infinity)      status   0 ok | 1 empty | 2 the sum is infinity
and `bad_index`: a value past the table; the tests put it in place of one index of the indexed form, whose group then has status 3.

Groups
  len_N        N = 0, 1, 2, 3, 8, 9, 64, 65 terms (the edges of AGG_C = 8 and of a second sum level), 255-bit scalars
  edge_*       s and -s mod r on one point; P and -P with scalar 1; the same term twice (a doubling in the sum); an all-zero point among
               good ones; zero scalars only; G2: the point outside the subgroup with scalars above r (plain route only: psi false)
  k_*          chosen scalars, a group of one each: 0, 1, 8, 9, 15, 16, every nibble 8, every nibble f, 16^j 8 + 8, r - 1, r, r + 1, 2^255,
               2^256 - 1; G2 also X - 1, X, X + 1, X^2, X^3, X^3 + X^2 + X + 1, every base-X digit X - 1, base-X digits 16^j 8 + 8, and a
               scalar with d0 = d2, d1 = d3 (the Straus accumulator meets psi-images of itself)
  nbits_N      N = 1, 4, 5, 64, 255, 256 over scalars with every high bit set
The file holds about 40 groups per curve; the eight lengths alone are 152 terms per curve, so it has about 400 terms, 70 KB.

Run:  python tests/golden/gen_lincomb.py      (pure Python, about a minute).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls12381_py as o  # noqa: E402

R, X = o.R, o.X_ABS
LENGTHS = (0, 1, 2, 3, 8, 9, 64, 65)
NBITS = (1, 4, 5, 64, 255, 256)
ALL = (1 << 256) - 1


def h(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "little")


def chosen(g2):
    cs = [("0", 0), ("1", 1), ("8", 8), ("9", 9), ("15", 15), ("16", 16), ("nibbles_8", int("8" * 64, 16)), ("nibbles_f", ALL)]
    cs += [("8_at_%d_plus_8" % j, 16 ** j * 8 + 8) for j in (1, 15, 16, 62)]
    cs += [("r_minus_1", R - 1), ("r", R), ("r_plus_1", R + 1), ("2_255", 1 << 255), ("2_256_minus_1", ALL)]
    if g2:
        cs += [("x_minus_1", X - 1), ("x", X), ("x_plus_1", X + 1), ("x2", X ** 2), ("x3", X ** 3), ("x3_x2_x_1", X ** 3 + X ** 2 + X + 1)]
        top = (R - 1) // X ** 3                                          # the largest d3 a canonical scalar has
        # X^4 - 1 has four digits X - 1 but is not below r (it is X^2 - 2 mod r); the largest canonical scalar of that kind caps the top digit
        cs += [("digits_x_minus_1", X ** 4 - 1), ("digits_x_minus_1_below_r", (X - 1) * (1 + X + X ** 2) + (top - 1) * X ** 3)]
        cs += [("digits_8_at_%d_plus_8" % j, sum((16 ** j * 8 + 8) * X ** i for i in range(4))) for j in (1, 15)]
        assert R <= cs[-4][1] <= ALL and all(k < R and base_x(k)[0] == base_x(k)[3] for _, k in cs[-2:]) and cs[-3][1] < R
        d0, d1 = h(b"lincomb d0") % X, h(b"lincomb d1") % (top - 1)
        cs += [("d0_eq_d2_d1_eq_d3", d0 + d1 * X + d0 * X ** 2 + d1 * X ** 3)]
    names = [n for n, _ in cs]
    assert len(set(names)) == len(names)
    return cs


def base_x(k):
    d = []
    for _ in range(4):
        d.append(k % X)
        k //= X
    assert k == 0
    return d


def curve(g2):
    mul, add, neg, gen = (o.g2_mul, o.g2_add, o.g2_neg, o.G2_GEN) if g2 else (o.g1_mul, o.g1_add, o.g1_neg, o.G1_GEN)
    img = o.g2_to_blst_affine if g2 else o.g1_to_blst_affine
    nb = 192 if g2 else 96
    tag = b"g2" if g2 else b"g1"
    pts = [None] + [mul(gen, h(b"lincomb point %s %d" % (tag, i)) % R) for i in range(1, 12)]
    pts.append(neg(pts[1]))                                              # entry 12 = -entry 1
    if g2:
        u = o.hash_to_field_fp2(b"lincomb: a curve point outside G2", o.DST_SIG, 2)[0]
        outside = o.iso3_g2(o.sswu_g2(u))                                # SSWU + isogeny output, before cofactor clearing
        assert o.g2_on_curve(outside) and not o.g2_in_subgroup(outside)
        pts.append(outside)
        # the identity the psi route rests on: [X]Q = -psi(Q) on G2, and not for the point outside
        q = pts[3]
        assert mul(q, X) == neg(o.g2_psi(q)) and mul(outside, X) != neg(o.g2_psi(outside))
        k = h(b"lincomb identity") % R
        d = base_x(k)
        acc, e = None, q
        for i in range(4):
            t = mul(e, d[i])
            acc = add(acc, neg(t) if i & 1 else t)
            e = o.g2_psi(e)
        assert acc == mul(q, k)
    table = [bytes(nb) if p is None else img(p) for p in pts]
    groups = []

    def group(kind, terms, nbits=255, psi=None):
        acc = None
        for t, s in terms:
            assert 0 <= s <= ALL
            acc = add(acc, mul(pts[t], s & ((1 << nbits) - 1)) if pts[t] is not None else None)
        status = 1 if not terms else 2 if acc is None else 0
        g = {"kind": kind, "terms": [[t, s.to_bytes(32, "little").hex()] for t, s in terms], "nbits": nbits,
             "out": (img(acc) if status == 0 else bytes(nb)).hex(), "status": status}
        if g2:
            g["psi"] = all(t < 13 for t, _ in terms) if psi is None else psi
        groups.append(g)
        return g

    for n in LENGTHS:
        group("len_%d" % n, [(1 + (i * 7 + n) % 11, h(b"lincomb scalar %s %d %d" % (tag, n, i)) >> 1) for i in range(n)])
    s = h(b"lincomb cancel " + tag) % R
    assert group("edge_s_and_minus_s", [(2, s), (2, R - s)])["status"] == 2
    assert group("edge_p_and_minus_p", [(1, 1), (12, 1)])["status"] == 2
    group("edge_same_term_twice", [(4, s), (4, s), (5, 3)])
    group("edge_zero_point", [(3, s), (0, s >> 3), (6, 77)])
    assert group("edge_zero_scalars", [(3, 0), (4, 0)])["status"] == 2
    assert group("edge_zero_point_only", [(0, s)])["status"] == 2
    if g2:
        group("edge_outside_g2", [(13, R + 5)], nbits=256)
        group("edge_outside_g2_two", [(13, ALL), (13, (1 << 255) | 9)], nbits=256)
        assert groups[-2]["out"] != img(mul(pts[13], 5)).hex() and not groups[-1]["psi"]
    for name, k in chosen(g2):
        group("k_" + name, [(3, k)], nbits=256)
    for nbits in NBITS:
        group("nbits_%d" % nbits, [(5, ALL), (6, ALL ^ (1 << (nbits - 1))), (7, h(b"lincomb nbits %d" % nbits) | (ALL << nbits) & ALL)], nbits=nbits)
    return {"table": [t.hex() for t in table], "groups": groups, "bad_index": len(table) + 5}


def main():
    fx = {"r": hex(R), "x_abs": hex(X), "g1": curve(False), "g2": curve(True)}
    path = os.path.join(HERE, "lincomb.json")
    with open(path, "w") as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write("\n")
    terms = sum(len(g["terms"]) for c in ("g1", "g2") for g in fx[c]["groups"])
    print("wrote %s: %d + %d groups, %d terms, %d bytes" % (path, len(fx["g1"]["groups"]), len(fx["g2"]["groups"]), terms, os.path.getsize(path)))


if __name__ == "__main__":
    main()
