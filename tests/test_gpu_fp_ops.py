"""The device's field arithmetic bodies, its SSWU map and its final exponentiation on CHOSEN inputs.

On the batch path these bodies only ever see what SHA-256, a Miller loop or a bucket sum produces: uniformly random field elements in canonical
form.  Here they get the operand families of tests/fp_operands.py - carry-stressing limb patterns, non-canonical representatives of 0, 1 and -1,
uncarried sums and differences, the corners of the exponentiation's input contract - through mi355_bls_debug_fp_op (raw limbs in, raw limbs out),
the u values that take the SSWU map's rare arms through mi355_bls_debug_map_to_g2 in every form the batch path launches the map in, and chosen
Fp12 states through finalverify_shards.  The reference is big-integer arithmetic; tests/test_fp_operands_emu.py runs the same check functions on
the bounds-tracked CPU build, which proves that every operand is inside the contract of the body it meets.  A mismatch names the operation, the
family member and both values."""
import ctypes
import random

import pytest

import bls12381_py as o
import fp_operands as F
from util import fp12_from_bytes, fp12_to_bytes, slice_plan

pytestmark = pytest.mark.gpu

CAP = 8192


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


@pytest.fixture(scope="module")
def cache(m):
    c = m.BatchedBLSVerifierCache.init(max_sets=CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def run(m, cache):
    def run(op, a, b, fam_a, fam_b):
        return F.unwords(m.debugFpOp(cache, op, F.words(a), F.words(b)))
    return run


@pytest.mark.parametrize("pairing", F.PAIRINGS, ids=lambda p: "%s-%s" % p)
def test_multipliers(run, pairing):
    """fp_mul, fp_sqr, fp_sqr_n (1 and 4 squarings), fp_dot2, row_mul, row_sqr over the full cross product of a pairing"""
    F.check_multipliers(run, pairing)


def test_reduce_inverse_predicates(run):
    F.check_reduce(run)
    F.check_inv(run)
    F.check_predicates(run)


def test_exponentiation_in_its_three_forms(run):
    """fp_recip_sqrt_pow (the generated assembly body, in a 256-register kernel), pow_per_row and pow_two_rows: the same residues, the same verdicts"""
    F.check_pow(run)


def test_hooks_reject_bad_arguments(m, cache):
    """n == 0, n > max_sets, null pointers, an unknown operation: MI355_BLS_ERR_ARG (-3), as the other hooks answer"""
    L, img, us = m.lib(), bytes(56), bytes(224)
    buf, pts = ctypes.create_string_buffer(56), ctypes.create_string_buffer(576)
    for args in ((cache._h, 0, img, img, 0, buf), (cache._h, 0, img, img, CAP + 1, buf), (cache._h, 0, None, img, 1, buf), (cache._h, 0, img, None, 1, buf),
                 (cache._h, 0, img, img, 1, None), (None, 0, img, img, 1, buf), (cache._h, 9, img, img, 1, buf), (cache._h, 20, img, img, 1, buf),
                 (cache._h, -1, img, img, 1, buf)):
        assert L.mi355_bls_debug_fp_op(*args) == -3, args[1:2] + args[4:5]
    for args in ((cache._h, us, 0, pts), (cache._h, us, CAP + 1, pts), (cache._h, None, 1, pts), (cache._h, us, 1, None), (None, us, 1, pts)):
        assert L.mi355_bls_debug_map_to_g2(*args) == -3, args[2]


def _smallest(n0, S, coop, form):
    """the smallest n >= n0 whose map the plan gives `form` (0 rows, 1 spread, 2 plain) on a context of S wave slots"""
    n = n0
    while slice_plan(n, S, coop)["hash_map"] != form:
        n += 1
        assert n <= CAP, (form, S)
    return n


def test_sswu_map_through_every_batch_form(m, cache):
    """One list of u values (fp_operands.sswu_cases: u = 0, a zero real or imaginary part under both sgn0 values, u and -u, the same residues given
    non-canonically, 200 random u and the real-ratio family, for which N / D is real and the `fp_is_zero(d)` arm of the Fp2 square root is reachable;
    its branch tallies are asserted on the CPU before anything is sent) through k_hash_map_rows', k_hash_map_spread's and k_hash_map's bodies, at
    sizes the plan names those forms for.  The list is padded to each size with its own random u in a shuffled order, so every point has a
    reference computed once.  Every point equals the oracle's iso3(sswu(u)); the three forms' outputs are bit-exact equal.
    The mirror family, for which Z g(x1) is real, needs a cubic root in Fp and is left out."""
    import torch
    S = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows, _, want = F.sswu_cases()
    canon = [k for k, r in enumerate(rows) if r[3] == "canon"]
    random_rows = [k for k in canon if rows[k][0].startswith("rnd")]
    assert len(random_rows) == 200
    base = list(range(len(rows)))
    n0 = (len(base) + 1) // 2
    n_rows, n_spread = _smallest(n0, S, True, 0), _smallest(n0, S, True, 1)
    n_plain = _smallest(n_spread, S, False, 2)
    assert n_plain == n_spread and n_rows < n_spread
    rng = random.Random(20261022)

    def send(n, coop, form):
        assert slice_plan(n, S, coop)["hash_map"] == form                # the plan names the intended form
        which = base + [rng.choice(random_rows) for _ in range(2 * n - len(base))]
        cache.set_cooperative(coop)
        try:
            out = m.debugMapToG2(cache, F.words([c for k in which for c in rows[k][1]]))
        finally:
            cache.set_cooperative(True)
        pts = [out[288 * t:288 * t + 288] for t in range(2 * n)]
        for t, k in enumerate(which):
            assert F.same_point(pts[t], want[k]), "form %d, point %d: sswu + iso3 of %s (%s) = %s" % (form, t, rows[k][0], rows[k][3], pts[t].hex())
        return which, pts

    w0, p0 = send(n_rows, True, 0)
    rng = random.Random(20261023)
    w1, p1 = send(n_spread, True, 1)
    rng = random.Random(20261023)
    w2, p2 = send(n_plain, False, 2)
    assert w1 == w2 and p1 == p2                                         # spread and plain: the same 2 n points, bit for bit
    assert p0[:len(base)] == p1[:len(base)]                              # rows: the list itself
    seen = {}
    for w, p in ((w0, p0), (w1, p1)):                                    # and a u maps to the same bytes wherever it sits
        for k, pt in zip(w, p):
            assert seen.setdefault(k, pt) == pt, rows[k][0]
    by_name = {r[0]: k for k, r in enumerate(rows)}
    for i in range(4):                                                   # the map of -u is the negation
        assert want[by_name["pm%d-" % i]] == o.g2_neg(want[by_name["pm%d" % i]])


def _rnd12(rng):
    return tuple((rng.randrange(o.P), rng.randrange(o.P)) for _ in range(6))


def _prod(states):
    f = states[0]
    for s in states[1:]:
        f = o.f12mul(f, s)
    return f


F12_ZERO = (o.F2_ZERO,) * 6


@pytest.fixture(scope="module")
def final_cases():
    """(name, states, the oracle's final_exp of their product): computed once, shared by the two contexts.  The power is the oracle's own
    (f^(3 (p^12 - 1) / r), which the GT parity tests pin); the all-zero state is the one value-in, value-out case the oracle has no inverse for:
    fp6_inv(0) = 0, so GT = 0."""
    rng = random.Random(20261024)
    z, one = o.F2_ZERO, o.F2_ONE
    f, g = _rnd12(rng), _rnd12(rng)
    many = [_rnd12(rng) for _ in range(64)]
    to_one = [_rnd12(rng) for _ in range(63)]
    to_one.append(o.f12inv(_prod(to_one)))
    a, b = rng.randrange(1, o.P), rng.randrange(1, o.P)
    cases = [("one", [o.F12_ONE]), ("random", [f]), ("f, 1/f", [f, o.f12inv(f)]), ("g^r", [o.f12pow(g, o.R)]), ("64 random", many),
             ("64 with product 1", to_one), ("in Fp", [((a, 0), z, z, z, z, z)]), ("in Fp2", [((a, b), z, z, z, z, z)]),
             ("in Fp6", [(_rnd12(rng)[0], z, _rnd12(rng)[1], z, _rnd12(rng)[2], z)]), ("w", [(z, one, z, z, z, z)]),
             ("-1", [((o.P - 1, 0), z, z, z, z, z)]), ("p-1 in every slot", [((o.P - 1, o.P - 1),) * 6]),
             ("the Montgomery image of 1 in every slot", [((o.MONT_R, o.MONT_R),) * 6]), ("1 in every slot", [((1, 1),) * 6]),
             ("zero", [F12_ZERO])]
    out = []
    for name, states in cases:
        p = _prod(states)
        out.append((name, states, F12_ZERO if p == F12_ZERO else o.final_exp(p)))
    want = dict((n, w) for n, _, w in out)
    for name in ("one", "f, 1/f", "g^r", "64 with product 1", "in Fp", "in Fp2", "in Fp6"):
        assert want[name] == o.F12_ONE, name                            # verdict true: the easy part (or the order) gives 1
    assert want["random"] != o.F12_ONE and want["64 random"] != o.F12_ONE
    return out


def test_final_exponentiation_on_chosen_states(m, final_cases):
    """finalverify_shards on a latency-mode context (k_tail_rows: the cyclotomic squarings on DPP rows) and on a throughput-mode one (k_tail): the
    product of k states at k = 1, 2 and 64, states that multiply to 1, subfield elements (the easy part collapses to 1), w, -1, extreme coefficients
    and 0.  GT equals the oracle's final exponentiation of the product, the two contexts agree bit for bit, the verdict is GT == 1."""
    gts = {}
    for coop in (True, False):
        c = m.BatchedBLSVerifierCache.init(max_sets=64)
        c.set_cooperative(coop)
        for name, states, want in final_cases:
            ok = c.finalverify_shards([fp12_to_bytes(s) for s in states])
            gt = c.fetch(4, 576)
            assert fp12_from_bytes(gt) == want, (coop, name, gt.hex())
            assert ok is (want == o.F12_ONE), (coop, name)
            gts[coop, name] = gt
        for k in (0, 65):
            with pytest.raises(m.BlsGpuError):
                c.finalverify_shards([fp12_to_bytes(o.F12_ONE)] * k)
        c.close()
    for name, _, _ in final_cases:
        assert gts[True, name] == gts[False, name], name
