#!/usr/bin/env python3
"""Generates tests/golden/fk20.json: setups, polynomials and the images mi355_bls_fk20_open_all_many must give for them.  The call is
defined for ANY n = 2^m G1 points S_0 .. S_(n-1) and coefficients c_0 .. c_(n-1):

    h_t  = sum_{i=0}^{n-2-t} [c_(i+t+1)] S_i      t = 0 .. n-2,   h_(n-1) = infinity
    pi_l = sum_{t=0}^{n-1} [omega_n^(l t)] h_t    l = 0 .. n-1

For S_j = [tau^j]G these are h_t = [sum_i c_(i+t+1) tau^i]G and pi_l = [(p(tau) - p(omega^l)) / (tau - omega^l)]G, the KZG proof at
omega^l, and the fixture's expected images come from those closed forms; the one case whose setup is no SRS (arbitrary multiples of G, one
of them infinity) comes from the two sums as written.  Only oracle/bls12381_py.py (g1_mul, g1_to_blst_affine) and Python integers mod r are
used; nothing comes from the code under test.

`cases`, each
  name      a name
  n, k      k polynomials of n coefficients
  setup     the n 96-byte blst_p1_affine images of S_j, hex (all zero: infinity)
  polys     the k x n 32-byte little-endian coefficient images, hex; an image may be >= r and acts as its value mod r
  status    the k status bytes: 2 where a polynomial has an image >= r
  out       {flags as a decimal string: the k x n expected images, hex}; flags 0: pi_l at slot l; 2 (BITREV): pi_rev(l) at slot l;
            4 (H): h_t at slot t

Cases
  n1_k3 .. n16_k3   n = 1, 2, 4, 8, 16 with k = 3 random polynomials, flags 0, BITREV and H
  n64_k1            one polynomial of 64 coefficients, flags 0 and H
  special_n8        flags 0 and H: 0 the zero polynomial | 1 a constant | 2 X^(n-1) alone | 3 c_(n-1) = 0 | 4 a root inside the domain
                    (omega^3) | 5 h_2 is infinity | 6 every image is c + r | 7 c_2 is the image 2^256 - 1
  linear_n8         S_j = [s_j]G for arbitrary s_j with s_5 = 0 (infinity), flags 0, BITREV and H

Run:  python tests/golden/gen_fk20.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
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


def h(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "little") % R


TAU = h(b"fk20 tau")


def image(a):
    a %= R
    if a not in _images:
        _images[a] = o.g1_to_blst_affine(o.g1_mul(o.G1_GEN, a))
    return _images[a]


def h_scalars(s, c):
    """the defining sum over the setup's scalars s_j: h_t = sum_{i <= n-2-t} c_(i+t+1) s_i"""
    n = len(c)
    return [sum(c[i + t + 1] * s[i] for i in range(n - 1 - t)) % R for t in range(n)]


def pi_scalars(hs):
    """the defining sum: pi_l = sum_t omega^(l t) h_t"""
    n = len(hs)
    w = fc.omega(n)
    return [sum(pow(w, l * t, R) * x for t, x in enumerate(hs)) % R for l in range(n)]


def pi_closed(c, tau):
    """(p(tau) - p(omega^l)) / (tau - omega^l)"""
    n = len(c)
    w = fc.omega(n)

    def p(x):
        return sum(a * pow(x, j, R) for j, a in enumerate(c)) % R
    return [(p(tau) - p(pow(w, l, R))) * pow(tau - pow(w, l, R), -1, R) % R for l in range(n)]


def case(name, s, polys, flags, srs):
    """s: the setup's scalars; polys: rows of coefficient IMAGES (integers below 2^256)"""
    n = len(s)
    m = n.bit_length() - 1
    assert all(len(p) == n for p in polys)
    out = {str(f): b"" for f in flags}
    for p in polys:
        c = [a % R for a in p]
        hs = h_scalars(s, c)
        pis = pi_scalars(hs)
        assert hs[n - 1] == 0
        if srs:                                              # the closed forms are what the fixture holds; the sums must agree with them
            assert s == [pow(TAU, j, R) for j in range(n)] and pow(TAU, n, R) != 1
            assert hs == [sum(c[i + t + 1] * pow(TAU, i, R) for i in range(n - 1 - t)) % R for t in range(n)]
            assert pis == pi_closed(c, TAU)
        for f in flags:
            if f & H:
                row = hs
            elif f & BITREV:
                row = [pis[fc.rev(l, m)] for l in range(n)]
            else:
                row = pis
            out[str(f)] += b"".join(image(x) for x in row)
    return {"name": name, "n": n, "k": len(polys), "setup": b"".join(image(a) for a in s).hex(),
            "polys": b"".join(a.to_bytes(32, "little") for p in polys for a in p).hex(),
            "status": [2 if any(a >= R for a in p) else 0 for p in polys], "out": {f: b.hex() for f, b in out.items()}}


def srs(n):
    return [pow(TAU, j, R) for j in range(n)]


def specials(n):
    rnd = [[h(b"fk20 special %d %d %d" % (n, g, j)) for j in range(n)] for g in range(8)]
    w = fc.omega(n)
    zero = [0] * n
    const = [rnd[1][0]] + [0] * (n - 1)
    top = [0] * (n - 1) + [rnd[2][0]]
    no_top = rnd[3][:n - 1] + [0]
    q = rnd[4][:n - 1]                                       # (X - omega^3) q(X)
    z = pow(w, 3, R)
    root = [((q[j - 1] if j else 0) - z * (q[j] if j < n - 1 else 0)) % R for j in range(n)]
    assert sum(a * pow(z, j, R) for j, a in enumerate(root)) % R == 0
    hole = list(rnd[5])                                      # sum_i c_(i+3) tau^i = 0
    hole[3] = -sum(hole[i + 3] * pow(TAU, i, R) for i in range(1, n - 3)) % R
    assert h_scalars(srs(n), hole)[2] == 0 and all(hole)
    over = [a % ((1 << 256) - R) + R for a in rnd[6]]        # every image in [r, 2^256)
    ones = list(rnd[7])
    ones[2] = (1 << 256) - 1
    return [zero, const, top, no_top, root, hole, over, ones]


def main():
    cases = []
    for n in (1, 2, 4, 8, 16):
        cases.append(case("n%d_k3" % n, srs(n), [[h(b"fk20 %d %d %d" % (n, g, j)) for j in range(n)] for g in range(3)], (0, BITREV, H), True))
    cases.append(case("n64_k1", srs(64), [[h(b"fk20 64 0 %d" % j) for j in range(64)]], (0, H), True))
    cases.append(case("special_n8", srs(8), specials(8), (0, H), True))
    s = [h(b"fk20 linear setup %d" % j) for j in range(8)]
    s[5] = 0
    cases.append(case("linear_n8", s, [[h(b"fk20 linear %d %d" % (g, j)) for j in range(8)] for g in range(2)], (0, BITREV, H), False))
    path = os.path.join(HERE, "fk20.json")
    with open(path, "w") as f:
        json.dump({"r": hex(R), "tau": hex(TAU), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d distinct points, %d bytes" % (path, len(cases), len(_images), os.path.getsize(path)))


if __name__ == "__main__":
    main()
