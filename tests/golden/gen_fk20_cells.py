#!/usr/bin/env python3
"""Generates tests/golden/fk20_cells.json: setups, polynomials and the images mi355_bls_fk20_open_cells_many must give for them.  The call
is defined for ANY n = 2^m G1 points S_0 .. S_(n-1), coefficients c_0 .. c_(n-1), a cell size l = 2^c <= n, q = n / l and N = q 2^ext:

    h_s  = sum_{i=0}^{n-1-l(s+1)} [c_(i + l(s+1))] S_i     s = 0 .. q-2,   h_(q-1) = infinity
    pi_j = sum_{s=0}^{q-1} [omega_N^(j s)] h_s              j = 0 .. N-1

For S_i = [tau^i]G, pi_j = [Q_j(tau)]G with Q_j = p(X) div (X^l - omega_N^j), the KZG multi-proof of the coset {x : x^l = omega_N^j}: the
fixture's expected images come from that long division, and the generator asserts that the two sums as written give the same scalars.  The
one case whose setup is no SRS comes from the sums as written.  Only oracle/bls12381_py.py (g1_mul, g1_to_blst_affine) and Python integers
mod r are used; nothing comes from the code under test.  tau and the polynomials of n16 are gen_fk20.py's, so that cell 1, ext 0 repeats
fk20.json's n16_k3.

`points`: every DISTINCT 96-byte blst_p1_affine image the cases speak of, hex, once (entry 0 is the all-zero image: infinity); the cases
name images by their number in it (tests/fk20_cells_cases.py puts the bytes back).
`cases`, each
  name      a name
  n, k      k polynomials of n coefficients
  cell, ext the cell size l and ext_log2
  setup     the n images of S_i, as numbers in `points`
  polys     the k x n 32-byte little-endian coefficient images, hex; an image may be >= r and acts as its value mod r.  Cases that share
            their polynomials hold the NAME of the first case that has them instead (wide_n16: its first k)
  status    the k status bytes: 2 where a polynomial has an image >= r
  out       {flags as a decimal string: the expected images, as numbers in `points`}; flags 0: k x N, pi_j at slot j; 2 (BITREV):
            pi_rev(j) at slot j; 4 (H): k x q, h_s at slot s

Cases
  n16_l<l>_x<x>     n = 16, k = 3 random polynomials, l in 1, 2, 4, 8, 16 and ext in 0, 1; flags 0, BITREV and H
  wide_n16          n = 16, l = 4, ext = 2: N = 16 > 2q = 8; the first two of those polynomials; flags 0 and BITREV
  n64_l8_x1         n = 64, l = 8, ext = 1, k = 2; flags BITREV and H
  special_n16       l = 4, ext = 1, flags 0 and H: 0 the zero polynomial | 1 degree < l | 2 X^(n-1) alone | 3 divisible by X^l - omega_N^3 |
                    4 h_1 is infinity | 5 every image is c + r | 6 c_2 is the image 2^256 - 1
  sums_n16          l = 4, ext = 1, S_i = [s_i]G with S_(4u+1) = S_(4u), S_(4u+3) = -S_(4u+2) and S_8 = S_9 = infinity (the pair that keeps
                    the first relation); flags 0, BITREV and H: 0 c_(4u) = c_(4u+1) and c_(4u+2) = c_(4u+3): in every slot of the l-fold
                    sum two equal terms and two opposite ones | 1 the same with c_(4u+2) = c_(4u+3) = 0: two equal terms and two infinities
                    | 2 c_(4u) = c_(4u+1) = 0: two infinities and an opposite pair, every slot sum and every output is infinity

Run:  python tests/golden/gen_fk20_cells.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import bls12381_py as o  # noqa: E402
import frntt_cases as fc  # noqa: E402

R = o.R
assert R == fc.R
BITREV, H = 2, 4
_images = {0: bytes(96)}
_numbers = {0: 0}                                            # scalar -> its image's number in `points`


def h(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "little") % R


TAU = h(b"fk20 tau")


def image(a):
    a %= R
    if a not in _images:
        _images[a] = o.g1_to_blst_affine(o.g1_mul(o.G1_GEN, a))
    return _images[a]


def number(a):
    image(a)
    return _numbers.setdefault(a % R, len(_numbers))


def h_scalars(s, c, l):
    """the defining sum over the setup's scalars s_i: h_t = sum_{i <= n-1-l(t+1)} c_(i + l(t+1)) s_i, t < q"""
    n = len(c)
    return [sum(c[i + l * (t + 1)] * s[i] for i in range(n - l * (t + 1))) % R for t in range(n // l)]


def pi_scalars(hs, ext):
    """the defining sum: pi_j = sum_t omega_N^(j t) h_t, N = q 2^ext"""
    big = len(hs) << ext
    w = fc.omega(big)
    return [sum(pow(w, j * t, R) * x for t, x in enumerate(hs)) % R for j in range(big)]


def quotient_at(c, l, a, x):
    """(p(X) div (X^l - a))(x), by long division from the top coefficient down"""
    rem, quo = list(c), [0] * len(c)
    for d in range(len(c) - 1, l - 1, -1):
        quo[d - l] = rem[d]
        rem[d - l] = (rem[d - l] + a * rem[d]) % R
        rem[d] = 0
    return sum(b * pow(x, j, R) for j, b in enumerate(quo)) % R


def case(name, s, polys, l, ext, flags, srs):
    """s: the setup's scalars; polys: rows of coefficient IMAGES (integers below 2^256)"""
    n = len(s)
    assert all(len(p) == n for p in polys) and n % l == 0
    q = n // l
    big = q << ext
    mb = big.bit_length() - 1
    out = {str(f): [] for f in flags}
    for p in polys:
        c = [a % R for a in p]
        hs = h_scalars(s, c, l)
        pis = pi_scalars(hs, ext)
        assert hs[q - 1] == 0 and len(pis) == big
        if srs:                                              # the closed form is what the fixture holds; the sums must agree with it
            assert s == [pow(TAU, j, R) for j in range(n)]
            closed = [quotient_at(c, l, pow(fc.omega(big), j, R), TAU) for j in range(big)]
            assert closed == pis
            pis = closed
        for f in flags:
            if f & H:
                row = hs
            elif f & BITREV:
                row = [pis[fc.rev(j, mb)] for j in range(big)]
            else:
                row = pis
            out[str(f)] += [number(x) for x in row]
    return {"name": name, "n": n, "k": len(polys), "cell": l, "ext": ext, "setup": [number(a) for a in s],
            "polys": b"".join(a.to_bytes(32, "little") for p in polys for a in p).hex(),
            "status": [2 if any(a >= R for a in p) else 0 for p in polys], "out": out}


def srs(n):
    return [pow(TAU, j, R) for j in range(n)]


def specials(n, l, ext):
    rnd = [[h(b"fk20 cells special %d %d %d" % (n, g, j)) for j in range(n)] for g in range(7)]
    q = n // l
    zero = [0] * n
    low = rnd[1][:l] + [0] * (n - l)
    top = [0] * (n - 1) + [rnd[2][0]]
    a = pow(fc.omega(q << ext), 3, R)                        # (X^l - a) d(X), d of degree n - l - 1
    d = rnd[3][:n - l]
    div = [((d[j - l] if j >= l else 0) - a * (d[j] if j < n - l else 0)) % R for j in range(n)]
    assert quotient_at(div, l, a, TAU) == sum(b * pow(TAU, j, R) for j, b in enumerate(d)) % R
    hole = list(rnd[4])                                      # h_1 = sum_i c_(i + 2l) tau^i = 0
    hole[2 * l] = -sum(hole[i + 2 * l] * pow(TAU, i, R) for i in range(1, n - 2 * l)) % R
    assert h_scalars(srs(n), hole, l)[1] == 0 and h_scalars(srs(n), hole, l)[0] != 0 and all(hole)
    over = [b % ((1 << 256) - R) + R for b in rnd[5]]        # every image in [r, 2^256)
    ones = list(rnd[6])
    ones[2] = (1 << 256) - 1
    return [zero, low, top, div, hole, over, ones]


def sums_case():
    n, l = 16, 4
    s = [0] * n
    for u in range(n // l):
        a, b = h(b"fk20 cells sums setup a %d" % u), h(b"fk20 cells sums setup b %d" % u)
        if u == 2:
            a = 0                                            # S_8 = S_9 = infinity
        s[l * u:l * u + l] = [a, a, b, -b % R]
    polys = []
    for g in range(3):
        p = [0] * n
        for u in range(n // l):
            a, b = h(b"fk20 cells sums poly a %d %d" % (g, u)), h(b"fk20 cells sums poly b %d %d" % (g, u))
            if g == 1:
                b = 0
            if g == 2:
                a = 0
            p[l * u:l * u + l] = [a, a, b, b]
        polys.append(p)
    return case("sums_n16", s, polys, l, 1, (0, BITREV, H), False)


def main():
    cases = []
    p16 = [[h(b"fk20 %d %d %d" % (16, g, j)) for j in range(16)] for g in range(3)]          # gen_fk20.py's n16_k3
    for l in (1, 2, 4, 8, 16):
        for ext in (0, 1):
            cases.append(case("n16_l%d_x%d" % (l, ext), srs(16), p16, l, ext, (0, BITREV, H), True))
    cases.append(case("wide_n16", srs(16), p16[:2], 4, 2, (0, BITREV), True))
    cases.append(case("n64_l8_x1", srs(64), [[h(b"fk20 cells 64 %d %d" % (g, j)) for j in range(64)] for g in range(2)], 8, 1, (BITREV, H), True))
    cases.append(case("special_n16", srs(16), specials(16, 4, 1), 4, 1, (0, H), True))
    cases.append(sums_case())
    path = os.path.join(HERE, "fk20_cells.json")
    points = [_images[a].hex() for a in sorted(_numbers, key=_numbers.get)]
    first = {}
    for c in cases:                                          # polynomials that an earlier case holds: its name
        held = [name for hexes, name in first.items() if hexes.startswith(c["polys"])]
        if held:
            c["polys"] = held[0]
        else:
            first[c["polys"]] = c["name"]
    with open(path, "w") as f:                                # a case a line, four points a line
        f.write('{"r": "%s", "tau": "%s",\n"cases": [\n%s],\n' % (hex(R), hex(TAU), ",\n".join(json.dumps(c, sort_keys=True) for c in cases)))
        f.write('"points": [\n%s]}\n' % ",\n".join(", ".join('"%s"' % x for x in points[i:i + 4]) for i in range(0, len(points), 4)))
    print("wrote %s: %d cases, %d distinct points, %d bytes" % (path, len(cases), len(_images), os.path.getsize(path)))


if __name__ == "__main__":
    main()
