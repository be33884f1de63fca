"""k_hash_clear (round 5: one hand-allocated assembly statement, tools/gen_clear_asm.py) and the lane-team engine's cofactor clearing (round 6:
k_team_clear + k_clear_fix, csrc/teamvm.hpp; a latency-mode context takes it) on the device, through the test hook
mi355_bls_debug_g2_clear_cofactor: H = clear_cofactor(q0 + q1) for pairs of arbitrary points of E2 against the oracle - including the inputs
no hash produces and the loop does NOT handle itself (it flags them and the kernel recomputes the lane with the complete formulas): points at
infinity, q0 == q1, q0 == -q1.  Reference: the cofactor clearing of hash-to-G2 (blst_abi.nim:383, RFC 9380 G.3)."""
import ctypes
import random

import pytest

import bls12381_py as o
from util import g2_jac_to_affine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def _jac_bytes(p, z):
    """affine p -> blst_p2 image with the Jacobian coordinate Z = z (an Fp2 element): (x z^2, y z^3, z)"""
    if p is None:
        return bytes(288)
    z2 = o.f2sqr(z)
    x, y = o.f2mul(p[0], z2), o.f2mul(p[1], o.f2mul(z2, z))
    return b"".join(o.fp_to_mont_bytes(c) for c in (x[0], x[1], y[0], y[1], z[0], z[1]))


def _patterns(rng):
    """76 pairs (q0, q1): 70 of arbitrary points of E2, then the exceptional ones at 70 .. 74 (q / infinity, infinity / q, infinity /
    infinity, q / q, q / -q) and two multiples of the generator"""
    def e2_point():          # a point of E2(Fp2), generally outside G2: what the SSWU map + isogeny produce
        return o.iso3_g2(o.sswu_g2((rng.randrange(o.P), rng.randrange(o.P))))

    pairs = [(e2_point(), e2_point()) for _ in range(70)]
    a, b = e2_point(), e2_point()
    return pairs + [(a, None), (None, b), (None, None), (a, a), (a, o.g2_neg(a)), (o.G2_GEN, o.g2_mul(o.G2_GEN, 2))]


EXCEPTIONAL = (72, 70, 71, 73, 74)       # _patterns' infinity / infinity, q / infinity, infinity / q, q / q, q / -q


@pytest.mark.parametrize("mode", ["throughput", "latency", "latency_rows2", "latency_team"])
def test_clear_cofactor_of_arbitrary_pairs(m, mode):
    rng = random.Random(3)

    def z():
        return (rng.randrange(1, o.P), rng.randrange(o.P))

    pairs = _patterns(rng)
    if mode == "latency_rows2":                     # 304 pairs: the row executor at two workgroups per CU
        pairs = pairs * 4
    if mode == "latency_team":                      # 456 pairs, beyond what the row executor takes (four waves per message): the lane-team engine, a message per 16 lanes
        pairs = pairs * 6
    blob = b"".join(_jac_bytes(p, z()) + _jac_bytes(q, z()) for p, q in pairs)
    out = ctypes.create_string_buffer(288 * len(pairs))
    cache = m.BatchedBLSVerifierCache.init(max_sets=1024)
    cache.set_cooperative(mode != "throughput")     # latency: the engine's programs on rows (k_team_clear_rows) or lane teams (k_team_clear); throughput: k_hash_clear
    assert m._check(m.lib().mi355_bls_debug_g2_clear_cofactor(cache._h, blob, len(pairs), out)) == 0
    for i, (p, q) in enumerate(pairs):
        got = g2_jac_to_affine(out.raw[288 * i:288 * i + 288])
        s = o.g2_add(p, q)
        want = None if s is None else o.clear_cofactor_g2(s)
        assert got == want, i
        assert got is None or o.g2_in_subgroup(got)


_RINV = pow(o.MONT_R, -1, o.P)


def _fp2_at(b, k):
    """Fp2 coordinate k (0 X, 1 Y, 2 Z) of a 288-byte Jacobian image, Montgomery limbs in any partially reduced form"""
    return tuple(int.from_bytes(b[96 * k + 48 * j:96 * k + 48 * j + 48], "little") * _RINV % o.P for j in (0, 1))


def _same_point(jac, want):
    """the Jacobian image `jac` is the affine point `want` (None: infinity): X = x Z^2, Y = y Z^3 - no inversion"""
    Z = _fp2_at(jac, 2)
    if want is None:
        return Z == (0, 0)
    Z2 = o.f2sqr(Z)
    return Z != (0, 0) and _fp2_at(jac, 0) == o.f2mul(want[0], Z2) and _fp2_at(jac, 1) == o.f2mul(want[1], o.f2mul(Z2, Z))


@pytest.fixture(scope="module")
def patterns():
    """(_patterns, the oracle's clear_cofactor(q0 + q1) of each): computed once, ~57 ms per pattern"""
    pats = _patterns(random.Random(3))
    return pats, [None if o.g2_add(p, q) is None else o.clear_cofactor_g2(o.g2_add(p, q)) for p, q in pats]


@pytest.mark.parametrize("slots_x", ["4S+1", "11S"])
def test_clear_cofactor_wide_form_with_exceptional_pairs(m, patterns, slots_x):
    """The plain (WIDE) grid of the lane-team engine, k_team_clear + k_clear_fix, which a latency-mode context takes from 4 S + 1 to 11 S
    messages (S = 4 x CU count; tests/util.py latency_plan): the 76 patterns tiled, every point with a fresh random Jacobian Z, and the
    exceptional pairs placed at index 0, on all four teams of one wave, on both sides of index 4 S and at n - 1 (at 4 S + 1 the lone live
    team of the last wave).  Every output equal to the oracle's projectively; the exceptional ones in G2."""
    import torch
    from util import TEAM_CLEAR_ITEMS_PER_SLOT, latency_plan
    S = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * S + 1 if slots_x == "4S+1" else 11 * S
    assert n <= TEAM_CLEAR_ITEMS_PER_SLOT * S and latency_plan(n, S)["clear"] == "team_wide", (n, S)
    pats, want = patterns
    which = [i % len(pats) for i in range(n)]
    special = [0] + [4 * (S // 2) + t for t in range(4)] + [4 * S - 1, 4 * S] + ([4 * S + 1] if 4 * S + 1 < n else []) + [n - 1]
    for j, i in enumerate(special):
        which[i] = EXCEPTIONAL[j % len(EXCEPTIONAL)]
    rng = random.Random(n)

    def z():
        return (rng.randrange(1, o.P), rng.randrange(o.P))

    blob = b"".join(_jac_bytes(pats[k][0], z()) + _jac_bytes(pats[k][1], z()) for k in which)
    out = ctypes.create_string_buffer(288 * n)
    cache = m.BatchedBLSVerifierCache.init(max_sets=n)                 # latency mode: the default
    assert m._check(m.lib().mi355_bls_debug_g2_clear_cofactor(cache._h, blob, n, out)) == 0
    cache.close()
    res = out.raw
    for i, k in enumerate(which):
        assert _same_point(res[288 * i:288 * i + 288], want[k]), (i, k)
    for i in special:
        got = g2_jac_to_affine(res[288 * i:288 * i + 288])
        assert got == want[which[i]] and (got is None or o.g2_in_subgroup(got)), i
