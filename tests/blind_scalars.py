"""Blinding scalars of the tests' choice (shared by the CPU and the GPU tests of mi355_bls_debug_batch_verify_scalars).

On the batch path the 64-bit blinding scalars come out of a SHA-256 chain, so the code that depends on their value - the signed 4-bit digits of
k_pkmul (tools/gen_pkmul_asm.py: k' = r + 0x8888888888888888, digit j = nibble j of k' minus 8, digit 16 = the carry), its "not started"
accumulator, its branches on an empty execution mask, the digit sort and the buckets of the signature side - sees only what uniform random
values produce.  The families below are the values it does not: every scalar is a non-zero u64 with a name, and the module asserts on import
(on the CPU, without a device) that the list holds every class the tests claim to run."""
import random

MASK64 = (1 << 64) - 1
BIAS = 0x8888888888888888


def digits(r):
    """the generator's digit rule: seventeen signed digits, d_0 .. d_15 in [-8, 7] and the carry d_16 in {0, 1}; sum d_j 16^j == r"""
    kp = r + BIAS
    return [((kp >> (4 * j)) & 15) - 8 for j in range(16)] + [kp >> 64]


def unsigned_digits(r, c):
    """the signature side's digits: window w = bits [c w, c w + c) of r"""
    return [(r >> (c * w)) & ((1 << c) - 1) for w in range(64 // c)]


def _families():
    fam = {}
    fam["single_digit"] = [("%d*16^%d" % (d, j), d << (4 * j)) for j in range(16) for d in range(1, 16)]
    fam["equal_nibbles"] = [("0x%X repeated" % d, d * 0x1111111111111111) for d in range(1, 16)]
    fam["all_minus_8"] = [("0x7777777777777778", 0x7777777777777778)]
    fam["edges"] = [("1", 1), ("2", 2), ("7", 7), ("8", 8), ("9", 9), ("15", 15), ("16", 16), ("17", 17), ("2^32-1", (1 << 32) - 1), ("2^32", 1 << 32),
                    ("2^32+1", (1 << 32) + 1), ("2^63-1", (1 << 63) - 1), ("2^63", 1 << 63), ("2^64-8", (1 << 64) - 8)]
    rng = random.Random(20261019)
    rnd = []
    while len(rnd) < 32:
        v = rng.getrandbits(64)
        if v:
            rnd.append(("random[%d]=0x%016x" % (len(rnd), v), v))
    fam["random"] = rnd
    return fam


FAMILIES = _families()
ALL = [("%s: %s" % (f, nm), v) for f, members in FAMILIES.items() for nm, v in members]          # (name, scalar); some values occur under two names
NAMES = [nm for nm, _ in ALL]
SCALARS = [v for _, v in ALL]
BY_NAME = dict(ALL)

# the scalars all 64 lanes of a wave share in the uniform-wave tests: a branch on an empty execution mask is taken only there
UNIFORM = [("1", 1), ("16^8", 1 << 32), ("8*16^15", 8 << 60), ("2^64-1", MASK64), ("0x7777777777777778", 0x7777777777777778),
           ("0x7777777777777777", 0x7777777777777777)]
# what tools/gen_pkmul_asm.py --selftest --scalars runs through the generated blocks (tests/test_asm_loops.py): at most 16
SELFTEST = [("1", 1), ("16^8", 1 << 32), ("8*16^15", 8 << 60), ("2^64-1", MASK64), ("0x7777777777777778", 0x7777777777777778),
            ("0x8888888888888888", BIAS), ("2^32-1", (1 << 32) - 1)] + [(nm, v) for nm, v in FAMILIES["random"][:4]]


def rotated(k):
    """the list rotated by k: scalar i + k (mod N) on set i, so every scalar meets another lane and another key"""
    k %= len(ALL)
    return ALL[k:] + ALL[:k]


def _census():
    assert len(NAMES) == len(set(NAMES)) and all(0 < v <= MASK64 for v in SCALARS)
    assert len(ALL) % 64 != 0 and len(ALL) > 4 * 64                                   # several waves, the last one partial
    assert len(SELFTEST) <= 16
    every = set(SCALARS)
    assert all(v in every for _, v in UNIFORM) and all(v in every for _, v in SELFTEST)      # subsets of the families
    D = {v: digits(v) for v in every}
    for v, dg in D.items():
        assert sum(d << (4 * j) for j, d in enumerate(dg)) == v and all(-8 <= d <= 7 for d in dg[:16]) and dg[16] in (0, 1), hex(v)
    for j in range(16):                                                               # every digit value at every position
        seen = {dg[j] for dg in D.values()}
        assert seen == set(range(-8, 8)), (j, sorted(set(range(-8, 8)) - seen))
    assert {dg[16] for dg in D.values()} == {0, 1}                                    # the carry digit takes both values
    first = {max(j for j in range(17) if dg[j]) for dg in D.values()}                 # where the accumulator starts (the loop walks j = 16 .. 0)
    assert first == set(range(17)), sorted(set(range(17)) - first)

    def zero_run_behind_start(dg):
        top = max(j for j in range(17) if dg[j])
        best = run = 0
        for j in range(top - 1, -1, -1):
            run = run + 1 if dg[j] == 0 else 0
            best = max(best, run)
        return best
    runs = {v: zero_run_behind_start(dg) for v, dg in D.items()}
    assert any(0 < x for x in runs.values()) and max(runs.values()) >= 15             # a zero digit, and fifteen in a row, behind a started accumulator
    assert runs[MASK64] == 15 and D[MASK64] == [-1] + [0] * 15 + [1]
    assert D[0x7777777777777778] == [-8] * 16 + [1] and D[0x7777777777777777] == [7] * 16 + [0] and D[BIAS] == [-8] + [-7] * 15 + [1]
    assert D[8 << 60] == [0] * 15 + [-8, 1]                                           # the carry digit 16 out of one negative digit
    assert any(v < 1 << 32 for v in every) and D[1] == [1] + [0] * 16                 # eight and more windows of doublings on a not-started accumulator
    for c in (4, 8):                                                                  # the signature side: empty, lowest and highest bucket of every window
        for w in range(64 // c):
            seen = {unsigned_digits(v, c)[w] for v in every}
            assert {0, 1, (1 << c) - 1} <= seen, (c, w)


_census()
