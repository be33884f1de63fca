"""The small-multiples family: inputs for point sums whose partial sums coincide, cancel and vanish on the way.

A base point P and the table T[k] = [k]P, k = -8 .. 8 (T[0] = infinity), made once with the big-int oracle.  A list of indices k_i sums to
[sum k_i]P in whatever order a reduction combines it, so the expected value of any sum is one table lookup or one oracle multiplication -
and with only seventeen distinct points, partial sums meet as equal points, as opposite points and as infinity all the time, in Jacobian
representations that differ (different Z) because they were reached by different additions.  That is the case the complete addition
formulas of csrc/curve.hpp decide by f_is_zero(H) on a value that is a non-zero multiple of p, and the one no random or hashed input makes.

The drawn inputs of tests/test_gpu_point_sums.py live here so that tests/test_point_sum_census.py (no GPU) can replay them through
tests/reduction_model.py and hold the seeds to what they are for."""
import functools
import random

import bls12381_py as o
from util import LAMBDAS_FP, LAMBDAS_FP2, g1_jac_image, g2_jac_image

KMAX = 8
KS = tuple(range(-KMAX, KMAX + 1))


class Family:
    """base, table and images of one curve: `g2` False = E(Fp) (G1 or, for the third family, a point of E(Fp) outside G1), True = G2"""

    def __init__(self, name, g2, base):
        self.name, self.g2, self.base = name, g2, base
        self._mul, self._neg = (o.g2_mul, o.g2_neg) if g2 else (o.g1_mul, o.g1_neg)
        self.lambdas = LAMBDAS_FP2 if g2 else LAMBDAS_FP
        self.aff_bytes, self.jac_bytes = (192, 288) if g2 else (96, 144)
        self.T = {0: None}
        for k in range(1, KMAX + 1):
            self.T[k] = self._mul(base, k)
            self.T[-k] = self._neg(self.T[k])
        self._aff = {k: self._to_aff(self.T[k]) for k in KS}

    def _to_aff(self, p):
        if p is None:
            return bytes(self.aff_bytes)                  # the all-zero image: infinity in an affine list
        return o.g2_to_blst_affine(p) if self.g2 else o.g1_to_blst_affine(p)

    def mul(self, k):
        """[k]P for any integer k"""
        return self.T[k] if -KMAX <= k <= KMAX else self._mul(self.base, k)

    def aff(self, k):
        return self._aff[k]

    def jac(self, k, lam):
        """the Jacobian image of T[k] with Z = lam (an index into the family's lambda set, or a field element)"""
        if isinstance(lam, int) and 0 <= lam < len(self.lambdas):
            lam = self.lambdas[lam]
        return (g2_jac_image if self.g2 else g1_jac_image)(self.T[k], lam)

    def affine_list(self, ks):
        return b"".join(self._aff[k] for k in ks)

    def jac_list(self, ks, lams):
        return b"".join(self.jac(k, l) for k, l in zip(ks, lams))

    def to_affine_bytes(self, p):
        return self._to_aff(p)


def _outside_g1(rng):
    """a point of E(Fp) whose order is not r"""
    while True:
        x = rng.randrange(o.P)
        y = o.fp_sqrt((x * x * x + 4) % o.P)
        if y is not None and o.g1_mul((x, y), o.R) is not None:
            return (x, y)


@functools.lru_cache(maxsize=None)
def family(name):
    """"g1", "g2" or "outside" (on E(Fp), outside G1); built on first use, then shared"""
    rng = random.Random("small multiples " + name)
    if name == "g1":
        return Family(name, False, o.g1_mul(o.G1_GEN, rng.randrange(1, o.R)))
    if name == "g2":
        return Family(name, True, o.g2_mul(o.G2_GEN, rng.randrange(1, o.R)))
    if name == "outside":
        return Family(name, False, _outside_g1(rng))
    raise ValueError(name)


# ---- drawn index lists
def draw(n, seed):
    rng = random.Random(seed)
    return [rng.randint(-KMAX, KMAX) for _ in range(n)]


def draw_zero(n, seed):
    """a drawn list bent from its end until it sums to zero"""
    ks = draw(n, seed)
    s = sum(ks)
    for i in reversed(range(n)):
        if s == 0:
            break
        new = max(-KMAX, min(KMAX, ks[i] - s))
        s -= ks[i] - new
        ks[i] = new
    assert sum(ks) == 0 or n == 1
    return ks


def draw_lams(n, seed, count):
    rng = random.Random(seed * 7919 + 1)
    return [rng.randrange(count) for _ in range(n)]


# (b) k_jac_sum_blst: Jacobian small multiples, every element with a lambda of its own
JAC_SIZES = (3, 33, 64, 65, 129, 300)
JAC_SEEDS = (1, 2, 3)


def _nonzero(ks):
    return [k if k else 1 for k in ks]


def jac_cases(nlam):
    """-> [(label, ks, lambda indices)].  The four lists of 64 after the drawn ones: `halves` - the second half repeats (negates) the first, so
    the tree's first step adds 32 equal (opposite) pairs and the halves have equal (opposite) sums; `lanes` - odd places repeat (negate) the even
    ones, so everything is generic until the tree's last step adds two sums of 32 elements that are equal (opposite)."""
    out = [("n%d/s%d" % (n, s), draw(n, 100 * n + s), draw_lams(n, 100 * n + s, nlam)) for n in JAC_SIZES for s in JAC_SEEDS]
    h = _nonzero(draw(32, 6401))
    pair = [k for k in _nonzero(draw(32, 6402)) for _ in (0, 1)]
    alt = list(range(nlam)) * 10
    out.append(("halves_equal", h + h, alt[:64]))
    out.append(("halves_opposite", h + [-k for k in h], alt[3:67]))
    out.append(("lanes_equal", pair, alt[1:65]))
    out.append(("lanes_opposite", [k if i % 2 == 0 else -k for i, k in enumerate(pair)], alt[2:66]))
    return out


# (c) aggregateAll / aggregateAllSignatures: affine small multiples, T[0] (the all-zero image) among them.  The seeds of the two sizes that
# have more than one block (513: two, 1025: three) are chosen so that k_*_sum2 meets block sums that are equal, opposite and zero - see the
# census in tests/test_point_sum_census.py.
AGG_SIZES = (2, 3, 4, 63, 64, 65, 128, 513, 1025)
AGG_SEEDS = {n: (1, 2, 3) for n in AGG_SIZES}
AGG_SEEDS[513] = (55, 129, 464)          # block 0 sums to zero | the two blocks have equal sums | block 1 sums to zero
AGG_SEEDS[1025] = (1, 8, 114)           # blocks 0 + 2 equal block 1 | a block sums to zero, on the left | on the right


def agg_cases():
    """-> [(label, ks)]: three drawn lists and one that sums to zero per size"""
    out = []
    for n in AGG_SIZES:
        out += [("n%d/s%d" % (n, s), draw(n, 1000 * n + s)) for s in AGG_SEEDS[n]]
        out.append(("n%d/zero" % n, draw_zero(n, 1000 * n) if n > 2 else [5, -5]))
    return out


# (d) aggregate_sets: index sequences into the 17-entry table
def aggsets_lists(C):
    """-> [(label, ks)].  Lengths 1, 2, C - 1, C, C + 1, C^2 + 1 and 600 drawn; then lists laid out against the plan's items (C consecutive keys
    each at level 0): `pairwise_*` - item 2j + 1 holds item 2j's keys (negated for `opposite`) in reverse order, so level 1 adds equal (opposite)
    sums that were reached by different additions; `items_zero` - every level-0 item sums to zero, so level 1 adds infinities only;
    `zero_*` - a drawn list bent to sum to zero (status 2)."""
    out = []
    for n in (1, 2, C - 1, C, C + 1, C * C + 1, 600):
        for s in (1, 2):
            out.append(("n%d/s%d" % (n, s), draw(n, 77 * n + s)))
    for n in (2, C + 1, C * C + 1, 600):
        out.append(("zero_n%d" % n, draw_zero(n, 78 * n) if n > 2 else [-3, 3]))
    items = [_nonzero(draw(C, 900 + j)) for j in range(C)]
    for j in range(C):
        if sum(items[j]) == 0:
            items[j][0] = items[j][0] % KMAX + 1
    out.append(("pairwise_equal", [k for it in items for k in it + it[::-1]]))
    out.append(("pairwise_opposite", [k for it in items for k in it + [-x for x in it[::-1]]] + [4]))
    half = [_nonzero(draw(C // 2, 950 + j)) for j in range(2 * C)]
    out.append(("items_zero", [k for h in half for k in h + [-x for x in h[::-1]]] + [7, 0, 7]))
    return out


# (e) Pippenger scalars
def pippenger_scalars():
    s = {0, 1, 2, o.R - 1, (1 << 255) - 1}
    for c in range(3, 18):
        s |= {(1 << c) - 1, 1 << c, (1 << c) + 1}
    return sorted(s)


# (a) one addition, every class, for every ordered pair of lambdas
def pair_table(fam, classes=None):
    """-> [(class, (ia, ib), A image, B image, expected affine point or None)] for every ordered pair of the family's lambdas.  `garbage_*`: the
    infinite operand is Z = 0 under non-zero X, Y."""
    from util import g1_inf_image, g2_inf_image
    inf_image = g2_inf_image if fam.g2 else g1_inf_image
    zero = bytes(fam.jac_bytes)
    out = []
    for ia, la in enumerate(fam.lambdas):
        for ib, lb in enumerate(fam.lambdas):
            k = 1 + (3 * ia + ib) % 4                      # 1 .. 4: k and 2 k stay in the table
            g = 1 + (ia + 2 * ib) % 3                      # the generic partner: k + g + 1 <= 8, and k + 1 + g != +-k
            trash_a = inf_image(la, fam.T[k][0]) if fam.g2 else inf_image(la, fam.T[k][0] + 1)
            trash_b = inf_image(fam.T[g][1], lb) if fam.g2 else inf_image(fam.T[g][1], lb + 1)
            rows = (("equal", fam.jac(k, la), fam.jac(k, lb), fam.T[2 * k]),
                    ("opposite", fam.jac(k, la), fam.jac(-k, lb), None),
                    ("a_inf", zero, fam.jac(-k, lb), fam.T[-k]),
                    ("b_inf", fam.jac(k, la), zero, fam.T[k]),
                    ("both_inf", zero, zero, None),
                    ("garbage_a", trash_a, fam.jac(k, lb), fam.T[k]),
                    ("garbage_b", fam.jac(-k, la), trash_b, fam.T[-k]),
                    ("garbage_both", trash_a, trash_b, None),
                    ("generic", fam.jac(k, la), fam.jac(k + g + 1, lb), fam.T[2 * k + g + 1] if 2 * k + g + 1 <= KMAX else fam.mul(2 * k + g + 1)))
            out += [(cl, (ia, ib), a, b, want) for cl, a, b, want in rows if classes is None or cl in classes]
    return out


# ---- the hard case itself.  The device's multiplier leaves values so close to canonical that two products with the same residue almost always
# have the same limbs: for equal or opposite operands with random Z, H = U2 - U1 is LITERALLY zero all but about once in 10 000 additions, and
# a branch test that looked at the limbs alone would pass everything above.  The pairs below were searched (search_hard_pairs, through
# emu_g1_add_probe / emu_g2_add_probe of tests/host_emu) for the other case: H, or r, is zero mod p and its limbs are not.
# tests/test_host_emu.py holds them to that; if the field arithmetic changes, search again.
HARD_SEED = 20261017


def search_hard_pairs(emu, fam, want=2, limit=400000):
    """-> {"equal_H" | "equal_r" | "opposite_H": [(k, iteration)]}: draws of hard_lambdas(fam, iteration) for which the probe reports a zero value
    with non-zero limbs"""
    probe = emu.emu_g2_add_probe if fam.g2 else emu.emu_g1_add_probe
    found = {"equal_H": [], "equal_r": [], "opposite_H": []}
    for it in range(limit):
        la, lb = hard_lambdas(fam, it)
        k = 1 + it % 4
        for cl, kb in (("equal", k), ("opposite", -k)):
            v = probe(fam.jac(k, la), fam.jac(kb, lb))
            key = cl + "_H" if (v & 3) == 1 else "equal_r" if cl == "equal" and (v & 12) == 4 else None
            if key and len(found[key]) < want:
                found[key].append((k, it))
        if all(len(x) >= want for x in found.values()):
            break
    return found


def hard_lambdas(fam, it):
    """the pair of Z values of iteration `it` of the search: a pure function of (family, it), so a found pair is stored as its iteration"""
    rng = random.Random("hard %s %d %d" % (fam.name, HARD_SEED, it))
    if fam.g2:
        return (rng.randrange(1, o.P), rng.randrange(o.P)), (rng.randrange(1, o.P), rng.randrange(o.P))
    return rng.randrange(1, o.P), rng.randrange(1, o.P)


HARD_PAIRS = {"g1": ((4, 3311), (4, 8327), (3, 12346), (2, 14121)), "g2": ((1, 2408), (2, 5465), (3, 3202), (4, 4699))}      # (k, iteration)


def hard_pair_table(fam):
    """-> [(class, (k, iteration), A image, B image, expected)]: equal and opposite operands with the searched Z pairs, in both orders"""
    out = []
    for k, it in HARD_PAIRS[fam.name]:
        la, lb = hard_lambdas(fam, it)
        a, b, nb = fam.jac(k, la), fam.jac(k, lb), fam.jac(-k, lb)
        out += [("equal", (k, it), a, b, fam.T[2 * k]), ("equal", (k, it), b, a, fam.T[2 * k]), ("opposite", (k, it), a, nb, None),
                ("opposite", (k, it), nb, a, None)]
    return out
