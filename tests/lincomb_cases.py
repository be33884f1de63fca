"""The inputs the CPU and GPU tests of the short linear combinations share: tests/golden/lincomb.json (tests/golden/gen_lincomb.py) laid out
as the calls take it.  A call has ONE nbits, so the fixture's groups are called together per nbits value."""
from util import golden

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
X = 0xd201000000010000
ROW = {"g1": 96, "g2": 192}


def fixture():
    return golden("lincomb")


def table_of(fx, curve):
    return [bytes.fromhex(t) for t in fx[curve]["table"]]


def nbits_values(fx, curve):
    return sorted({g["nbits"] for g in fx[curve]["groups"]})


def groups_of(fx, curve, nbits, psi=False):
    """the groups of one call: those of this nbits; psi: only the ones whose points are all in G2"""
    return [g for g in fx[curve]["groups"] if g["nbits"] == nbits and (not psi or g["psi"])]


def expected(groups):
    return b"".join(bytes.fromhex(g["out"]) for g in groups), bytes(g["status"] for g in groups)


def contiguous_inputs(fx, curve, groups):
    """-> (points laid end to end, scalars by position, offsets, expected images, status bytes)"""
    tab = table_of(fx, curve)
    pts = b"".join(tab[t] for g in groups for t, _ in g["terms"])
    sc = b"".join(bytes.fromhex(s) for g in groups for _, s in g["terms"])
    offsets = [0]
    for g in groups:
        offsets.append(offsets[-1] + len(g["terms"]))
    return (pts, sc, offsets) + expected(groups)


def indexed_inputs(fx, curve, groups, bad=False):
    """-> (table, idx, scalars by position, offsets, expected images, status bytes); bad: the first index of the first group of two or more
    terms that has good groups on both sides is replaced by the fixture's out-of-range value: status 3, the all-zero image"""
    _, sc, offsets, want, status = contiguous_inputs(fx, curve, groups)
    idx = [t for g in groups for t, _ in g["terms"]]
    if bad:
        row = ROW[curve]
        g = next(i for i in range(1, len(groups) - 1) if len(groups[i]["terms"]) >= 2 and groups[i - 1]["status"] == 0 and groups[i + 1]["status"] == 0)
        idx[offsets[g]] = fx[curve]["bad_index"]
        want = want[:row * g] + bytes(row) + want[row * g + row:]
        status = status[:g] + bytes([3]) + status[g + 1:]
    return b"".join(table_of(fx, curve)), idx, sc, offsets, want, status


def base_x(k):
    """the four base-X digits of k mod r"""
    k %= R
    d = []
    for _ in range(4):
        d.append(k % X)
        k //= X
    assert k == 0
    return d
