"""Inputs the pairing-product tests share (tests/test_gpu_pairing_check.py, tests/test_pairprod_emu.py): pairs built from bilinearity, so
that a verdict needs no oracle pairing, and the adversarial points of tests/golden/deser_adversarial.json as blst affine images.

A valid group of m pairs is (a_j G1, b_j G2) for j < m - 1 followed by (-(sum a_j b_j mod r) G1, G2): its product is
e(G1, G2)^(sum a_j b_j - sum a_j b_j) = 1.  An invalid group is the same with the closing scalar off by one."""
import random

import bls12381_py as o
import deser_cases as dc

OK, P_OFF_CURVE, P_NOT_IN_G1, Q_OFF_CURVE, Q_NOT_IN_G2 = range(5)
VALIDATE = 1
INF1, INF2 = bytes(96), bytes(192)

_g1, _g2 = {}, {}


def g1(a):
    """[a]G1 as a point of the oracle, remembered"""
    a %= o.R
    if a not in _g1:
        _g1[a] = o.g1_mul(o.G1_GEN, a) if a else None
    return _g1[a]


def g2(b):
    b %= o.R
    if b not in _g2:
        _g2[b] = o.g2_mul(o.G2_GEN, b) if b else None
    return _g2[b]


def p1b(p):
    return o.g1_to_blst_affine(p) if p is not None else INF1


def q2b(q):
    return o.g2_to_blst_affine(q) if q is not None else INF2


class Pool:
    """a few dozen small scalars whose multiples are made once; groups draw from them"""

    def __init__(self, seed, size=24):
        rng = random.Random(seed)
        self.a = [rng.randrange(2, 1 << 20) for _ in range(size)]
        self.b = [rng.randrange(2, 1 << 20) for _ in range(size)]

    def group(self, rng, m, valid=True):
        """-> [(P point, Q point)] of m >= 1 pairs"""
        js = [(rng.randrange(len(self.a)), rng.randrange(len(self.b))) for _ in range(m - 1)]
        s = sum(self.a[i] * self.b[j] for i, j in js) % o.R
        return [(g1(self.a[i]), g2(self.b[j])) for i, j in js] + [(g1(-s if valid else -s - 1), g2(1))]


def images(group):
    return [(p1b(p), q2b(q)) for p, q in group]


def adversarial():
    """-> {name: (96- or 192-byte affine image, expected status)}: points on a curve outside the subgroup (the fixture's torsion points and
    generator-plus-torsion sums) and points off the curve (a subgroup point with y + 1)"""
    fx = dc.fixture()
    out = {}
    for name in ("g1_ord3_0_pos", "g1_ord11_1_neg", "g1_ord10177_0_pos", "g1_G_plus_ord3_pos", "g1_G_plus_ord11_neg"):
        pt = o.g1_deserialize(bytes.fromhex(fx["enc"][name]["u"]))
        assert o.g1_on_curve(pt) and not o.g1_in_subgroup(pt)
        out[name] = (o.g1_to_blst_affine(pt), P_NOT_IN_G1)
    for name in ("g2_ord13_0_pos", "g2_ord23_1_neg", "g2_ord2713_0_pos", "g2_G_plus_ord13_pos", "g2_G_plus_ord2713_neg"):
        pt = o.g2_deserialize(bytes.fromhex(fx["enc"][name]["u"]))
        assert o.g2_on_curve(pt) and not o.g2_in_subgroup(pt)
        out[name] = (o.g2_to_blst_affine(pt), Q_NOT_IN_G2)
    x, y = g1(7)
    assert not o.g1_on_curve((x, (y + 1) % o.P))
    out["g1_off_curve"] = (o.g1_to_blst_affine((x, (y + 1) % o.P)), P_OFF_CURVE)
    x, y = g2(7)
    bad = (x, ((y[0] + 1) % o.P, y[1]))
    assert not o.g2_on_curve(bad)
    out["g2_off_curve"] = (o.g2_to_blst_affine(bad), Q_OFF_CURVE)
    return out
