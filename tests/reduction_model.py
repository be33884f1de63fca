"""The order in which the device's point sums combine their inputs, replayed on integers.

An input element is the small multiple [k]P of tests/small_multiples.py, so a partial sum is an integer and what kind of addition two partial
sums make - generic, equal points, opposite points, infinity on either side - is arithmetic on integers.  Each model below restates one
kernel's loop and fold in a few lines (csrc/kernels.hip, csrc/aggsets.hpp; the layout of the segmented sum comes from the product's own
plan.hpp through tests/host_emu).  The models check nothing on the device: tests/test_point_sum_census.py uses them to make sure the drawn
inputs of the GPU tests do reach the exceptional branches at every level, with operands whose Z differ.

A value carries (v, n, worked): the integer, the number of input elements summed into it, and whether its representation has been through a
genuine addition or came with a Z of its own (Z != 1).  Two equal values of which at least one is `worked` have different Z almost surely."""
from collections import Counter, namedtuple

V = namedtuple("V", "v n worked")
INF0 = V(0, 0, False)             # an accumulator nothing has been added to yet
WAVE = 64
CLASSES = ("equal", "opposite", "inf_left", "inf_right")


class Census:
    def __init__(self):
        self.counts = {}

    def add(self, level, a, b, single_right=False):
        """a + b as the complete formulas see it.  equal / opposite are counted for partial sums of at least two elements each that have been worked
        on; at a level whose right operand is one input element by construction (`single_right`) that is asked of the left operand alone.  An
        infinity is counted when it holds at least one element (an all-zero image, or a sum that cancelled) and so does the other operand: an empty
        accumulator on either side is not an event."""
        c = self.counts.setdefault(level, Counter())
        c["all"] += 1
        if a.v == 0 or b.v == 0:
            if a.v == 0 and a.n >= 1 and b.n >= 1:
                c["inf_left"] += 1
            if b.v == 0 and b.n >= 1 and a.n >= 1:
                c["inf_right"] += 1
            r = b if a.v == 0 else a
            return V(r.v, a.n + b.n, r.worked)
        deep = a.worked and a.n >= 2 and (single_right or (b.worked and b.n >= 2))
        if deep and a.v == b.v:
            c["equal"] += 1
        if deep and a.v == -b.v:
            c["opposite"] += 1
        return V(a.v + b.v, a.n + b.n, True)

    def fold(self, level, lanes, top=32):
        """for d = top .. 1: lane l += lane l + d (the shuffle fold; only the lanes that reach lane 0 are followed)"""
        lanes = list(lanes)
        d = top
        while d >= 1:
            for l in range(d):
                lanes[l] = self.add(level, lanes[l], lanes[l + d])
            d >>= 1
        return lanes[0]

    def missing(self, levels):
        return [(lv, cl) for lv in levels for cl in CLASSES if self.counts.get(lv, Counter())[cl] < 1]

    def table(self, levels):
        return "\n".join("    %-10s " % lv + "  ".join("%s %d" % (cl, self.counts.get(lv, Counter())[cl]) for cl in CLASSES + ("all",)) for lv in levels)


def aff(k):
    return V(k, 1, False)


def sum_grid(n, slots=1024, g2=False):
    """nblk, m of g1_sum_enqueue / mi355_bls_g2_aggregate_device (about 8 points per lane; slots = the context's wave slots)"""
    nblk = (n + WAVE * 8 - 1) // (WAVE * 8)
    nblk = min(nblk, slots if g2 else slots * 2)
    if g2:
        nblk = min(nblk, 2048)
    nblk = max(nblk, 1)
    return nblk, (n + nblk * WAVE - 1) // (nblk * WAVE)


def affine_sum(c, ks, slots=1024, g2=False):
    """k_g1_sum / k_g2_sum, then k_g1_sum2 / k_g2_sum2 -> the value"""
    n = len(ks)
    nblk, m = sum_grid(n, slots, g2)
    parts = []
    for b in range(nblk):
        lanes = []
        for l in range(WAVE):
            acc = INF0
            for j in range(m):
                i = l + WAVE * b + j * WAVE * nblk
                if i < n:
                    acc = c.add("sum.lane", acc, aff(ks[i]), single_right=True)
            lanes.append(acc)
        parts.append(c.fold("sum.fold", lanes))
    lanes = []
    for l in range(WAVE):
        acc = INF0
        for j in range(l, nblk, WAVE):
            acc = c.add("sum2", acc, parts[j])
        lanes.append(acc)
    return c.fold("sum2", lanes)


def jac_sum(c, ks, worked):
    """k_jac_sum_blst: lane l takes l, l + 64, ...; the fold starts at the largest power of two below k"""
    k = len(ks)
    lanes = []
    for l in range(WAVE):
        acc = INF0
        for j in range(l, k, WAVE):
            acc = c.add("jac.lane", acc, V(ks[j], 1, worked[j]), single_right=True)
        lanes.append(acc)
    top = 32
    while top >= 1 and top >= k:
        top >>= 1
    return c.fold("jac.fold", lanes, top)


def aggsets_sum(c, lists):
    """the segmented sum of mi355_bls_aggregate_sets over these index lists (plan.hpp aggsets_fill, aggsets.hpp) -> the value of every list"""
    from test_aggsets_plan import aggsets_plan, plan_aggsets_lib
    L = plan_aggsets_lib()
    keys = [k for ks in lists for k in ks]
    levels, lf, items, final_of = aggsets_plan(L, [len(ks) for ks in lists])
    part = {}
    for lv in range(levels):
        for src, cnt, dst, _ in items[lf[lv]:lf[lv + 1]].tolist():
            if lv == 0:
                acc = INF0
                for j in range(cnt):
                    acc = c.add("agg.l0", acc, aff(keys[src + j]), single_right=True)
            else:
                acc = part[src]
                for j in range(1, cnt):
                    acc = c.add("agg.ln", acc, part[src + j])
            part[dst] = acc
    return [part[f].v if f != L.aggsets_plan_none() else None for f in final_of.tolist()]
