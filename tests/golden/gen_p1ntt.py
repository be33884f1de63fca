#!/usr/bin/env python3
"""Generates tests/golden/p1ntt.json: vectors of G1 points [a_j]G with the images mi355_bls_p1s_ntt_many must give for them, through the
defining property of the call: the transform of [a_j]G is [fr_ntt(a)_i]G under the same flags.  Only oracle/bls12381_py.py (g1_mul,
g1_to_blst_affine) and tests/frntt_cases.py (ntt, in Python integers mod r) are used; nothing comes from the code under test.

`cases`, each
  name      a name
  n, k      k vectors of n points
  scalars   k x n scalars a_j as hex integers; 0 is the point at infinity (the all-zero image)
  in        the k x n 96-byte blst_p1_affine images of [a_j]G, hex
  out       {flags as a decimal string: the k x n expected images, hex} for the flag values the case is run under

Cases
  n1_k3 .. n16_k3   n = 1, 2, 4, 8, 16 with k = 3 random vectors, all four flag combinations
  n64_k1            one vector of 64, forward and INVERSE | BITREV
  special_n4, special_n8   seven vectors each, forward and INVERSE | BITREV (the DIF and the DIT walk, the latter with 1 / n folded in):
      0 all infinity | 1 constant (P, ..., P): a doubling in a + t, infinity from a - t | 2 (P, 0, ..., 0) | 3 (0, ..., 0, P)
      4 (P, -P, P, -P, ...) | 5 random with two infinity entries | 6 a vector whose forward transform has an infinity at slot 3

Run:  python tests/golden/gen_p1ntt.py      (pure Python, a few minutes).  Reproducible byte for byte: no clock, no `random`.
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
ALL_FLAGS = (0, 1, 2, 3)
BOTH_WALKS = (0, 3)
_images = {0: bytes(96)}


def h(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "little") % R


def image(a):
    a %= R
    if a not in _images:
        _images[a] = o.g1_to_blst_affine(o.g1_mul(o.G1_GEN, a))
    return _images[a]


def case(name, vectors, flags):
    n = len(vectors[0])
    assert all(len(v) == n for v in vectors)
    out = {}
    for f in flags:
        rows = [fc.ntt(list(v), bool(f & fc.INVERSE), bool(f & fc.BITREV)) for v in vectors]
        out[str(f)] = b"".join(image(x) for row in rows for x in row).hex()
    return {"name": name, "n": n, "k": len(vectors), "scalars": [[hex(a) for a in v] for v in vectors],
            "in": b"".join(image(a) for v in vectors for a in v).hex(), "out": out}


def specials(n):
    p = h(b"p1ntt special point %d" % n)
    rnd = [h(b"p1ntt special random %d %d" % (n, j)) for j in range(n)]
    rnd[1] = rnd[n - 2] = 0
    vals = [h(b"p1ntt special values %d %d" % (n, j)) for j in range(n)]
    vals[3] = 0
    hole = fc.ntt(vals, True, False)                       # its forward transform is vals: infinity at slot 3
    assert fc.ntt(hole)[3] == 0 and all(hole)
    return [[0] * n, [p] * n, [p] + [0] * (n - 1), [0] * (n - 1) + [p], [p if j % 2 == 0 else R - p for j in range(n)], rnd, hole]


def main():
    cases = []
    for n in (1, 2, 4, 8, 16):
        cases.append(case("n%d_k3" % n, [[h(b"p1ntt %d %d %d" % (n, g, j)) for j in range(n)] for g in range(3)], ALL_FLAGS))
    cases.append(case("n64_k1", [[h(b"p1ntt 64 0 %d" % j) for j in range(64)]], BOTH_WALKS))
    for n in (4, 8):
        cases.append(case("special_n%d" % n, specials(n), BOTH_WALKS))
    path = os.path.join(HERE, "p1ntt.json")
    with open(path, "w") as f:
        json.dump({"r": hex(R), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d distinct points, %d bytes" % (path, len(cases), len(_images), os.path.getsize(path)))


if __name__ == "__main__":
    main()
