"""Chosen operands for the device field arithmetic (a sibling of small_multiples.py): seeded, deterministic families of RAW fp images - 14 signed
28-bit limbs in 14 uint32 words, the in-register form of csrc/fp.hpp, not blst bytes - and their big-integer model.

    val(img) = sum of sign-extended l[i] * 2^(28 i)           (every limb is a two's complement 32-bit word; the top one carries the sign)

The images are Montgomery images only in the sense that the multipliers divide by R = 2^392: the model of a product is
val(a) val(b) 2^-392 mod p whatever a and b "mean".  tests/test_fp_operands_emu.py runs every (operation, family) pairing of
tests/test_gpu_fp_ops.py through the bounds-tracked CPU build (tests/host_emu) with each operand tagged by its family's BOUNDS - that is the proof
that a chosen operand is inside the contract of the operation it meets; the GPU test then holds the device bodies against the same model.

Families (each a list of (name, image)); BOUNDS[family] = the (BLS_VB, BLS_LB) tag of its images:
    canon       values in [0, p), fully carried
    noncanon    x + p, x - p, x - 2p + 1 and 2p - 1 - x for a subset x of canon, fully carried: other representatives of residues, |value| < 2p
    lazy        limb-wise sums and differences of two canon images, NOT carried: limbs reach +-(2^29 - 2), mixed signs across limbs
    pow_corner  values in (-8p, 8p) with at most two limb units: the input contract of fp_recip_sqrt_pow's assembly body
REGRESSIONS: operands at which the device once disagreed with the model, kept by name (none so far)."""
import random

import bls12381_py as o

P = o.P
N = 14
MASK = (1 << 28) - 1
R392 = 1 << 392
RINV = pow(R392, -1, P)
ONE_M = R392 % P                       # the Montgomery image of 1
POW_E = (P - 3) // 4

BOUNDS = {"canon": (1, 0), "noncanon": (2, 0), "lazy": (2, 2), "pow_corner": (8, 2)}


def _s32(w):
    return w - (1 << 32) if w & (1 << 31) else w


def val(img):
    """the integer an image stands for"""
    return sum(_s32(w) << (28 * i) for i, w in enumerate(img))


def limbs(img):
    """the signed limbs"""
    return [_s32(w) for w in img]


def carried(v):
    """the fully carried image of the integer v: limbs 0..12 in [0, 2^28), the top limb signed"""
    top = v >> (28 * (N - 1))
    assert -(1 << 31) <= top < (1 << 31)
    img = tuple((v >> (28 * i)) & MASK for i in range(N - 1)) + (top & 0xffffffff,)
    assert val(img) == v
    return img


def limbwise(a, b, sign_a=1, sign_b=1):
    """sign_a a + sign_b b limb by limb, no carry"""
    out = []
    for x, y in zip(limbs(a), limbs(b)):
        s = sign_a * x + sign_b * y
        assert -(1 << 31) <= s < (1 << 31)
        out.append(s & 0xffffffff)
    return tuple(out)


def words(imgs):
    """images -> the bytes of their uint32 words, one after another"""
    return b"".join(int(w).to_bytes(4, "little") for img in imgs for w in img)


def unwords(b):
    """bytes -> list of 14-word images"""
    assert len(b) % (4 * N) == 0
    w = [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(len(b) // 4)]
    return [tuple(w[N * i:N * i + N]) for i in range(len(w) // N)]


_TOP = P >> (28 * (N - 1))              # p's top limb
ALL_HIGH = ((_TOP - 1) << 364) | ((1 << 364) - 1)


def _canon_values():
    rng = random.Random(20261018)
    named = [("0", 0), ("1", 1), ("2", 2), ("p-1", P - 1), ("p-2", P - 2), ("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2), ("R", ONE_M),
             ("RR", R392 * R392 % P), ("-R", P - ONE_M),
             ("low0_top", _TOP << 364), ("low0_1", 1 << 364), ("lowF_top", ALL_HIGH), ("lowF_0", (1 << 364) - 1)]
    named += [("2^%d" % (28 * i), 1 << (28 * i)) for i in range(1, N)] + [("2^%d-1" % (28 * i), (1 << (28 * i)) - 1) for i in range(1, N)]
    named += [("rnd%d" % i, rng.randrange(P)) for i in range(32)]
    seen, out = set(), []
    for name, v in named:
        assert 0 <= v < P, name
        if v not in seen:
            seen.add(v)
            out.append((name, v))
    return out


CANON_VALUES = _canon_values()
_NONCANON_OF = ("0", "1", "2", "p-1", "p-2", "(p-1)/2", "R", "-R", "low0_top", "lowF_top", "lowF_0", "low0_1", "rnd0", "rnd1", "rnd2")


def _families():
    canon = [(name, carried(v)) for name, v in CANON_VALUES]
    by_name = dict(CANON_VALUES)
    noncanon = []
    for name in _NONCANON_OF:
        x = by_name[name]
        noncanon += [(name + "+p", carried(x + P)), (name + "-p", carried(x - P)), (name + "-2p+1", carried(x - 2 * P + 1)), ("2p-1-" + name, carried(2 * P - 1 - x))]
    img = dict(canon)
    rng = random.Random(20261019)
    names = [n for n, _ in canon]
    pairs = [("lowF_top", "lowF_top"), ("lowF_top", "lowF_0"), ("lowF_0", "low0_top"), ("p-1", "p-1"), ("p-1", "lowF_top"), ("0", "lowF_top"), ("R", "-R"),
             ("2^196-1", "2^196"), ("lowF_0", "2^196-1")]
    pairs += [(rng.choice(names), rng.choice(names)) for _ in range(11)]
    lazy = []
    for a, b in pairs:
        lazy += [("%s + %s" % (a, b), limbwise(img[a], img[b])), ("%s - %s" % (a, b), limbwise(img[a], img[b], 1, -1)),
                 ("-%s - %s" % (a, b), limbwise(img[a], img[b], -1, -1))]
    corner = []
    for name, v in (("8p-1", 8 * P - 1), ("7p+1", 7 * P + 1), ("4p", 4 * P), ("2p-1", 2 * P - 1), ("p", P), ("1", 1), ("0", 0), ("R+7p", ONE_M + 7 * P),
                    ("-R+8p", 8 * P - ONE_M)):
        corner += [(name, carried(v)), ("-(%s)" % name, carried(-v))]
    h = carried(4 * P - 1)
    corner += [("(4p-1) + (4p-1) nc", limbwise(h, h)), ("-(4p-1) - (4p-1) nc", limbwise(h, h, -1, -1)),
               ("lowF_top + (7p-1) nc", limbwise(img["lowF_top"], carried(7 * P - 1))), ("(4p-1) - lowF_top nc", limbwise(h, img["lowF_top"], 1, -1))]
    for i in range(12):
        kq, x = rng.randrange(-8, 8), rng.randrange(P)
        corner.append(("rnd%d%+dp" % (i, kq), carried(x + kq * P)))
    fams = {"canon": canon, "noncanon": noncanon, "lazy": lazy, "pow_corner": corner}
    # what the docstring promises
    assert all(0 <= val(i) < P and all(0 <= x <= MASK for x in limbs(i)[:13]) for _, i in canon)
    assert all(abs(val(i)) < 2 * P and all(0 <= x <= MASK for x in limbs(i)[:13]) for _, i in noncanon)
    lz = [x for _, i in lazy for x in limbs(i)[:13]]
    assert max(lz) == (1 << 29) - 2 and min(lz) == -((1 << 29) - 2) and all(abs(val(i)) < 2 * P for _, i in lazy)
    assert any(min(limbs(i)[:13]) < 0 < max(limbs(i)[:13]) for _, i in lazy)
    assert all(abs(val(i)) < 8 * P and all(abs(x) < (1 << 29) for x in limbs(i)[:13]) for _, i in corner)
    assert {8 * P - 1, 1 - 8 * P} <= {val(i) for _, i in corner}
    return fams


FAMILIES = _families()
REGRESSIONS = []                       # (operation, family, name, image): none so far


def family(name):
    return FAMILIES[name]


# ---- the model: residues mod p
def m_mul(a, b):
    return val(a) * val(b) * RINV % P


def m_sqr_n(a, n):
    v = val(a) % P
    for _ in range(n):
        v = v * v * RINV % P
    return v


def m_dot2(a0, b0, a1, b1):
    return (val(a0) * val(b0) + val(a1) * val(b1)) * RINV % P


def m_inv(a):
    """R^2 / val(a): the Montgomery image of the inverse; 0 for a = 0 mod p"""
    v = val(a) % P
    return pow(v, -1, P) * R392 * R392 % P if v else 0


def m_pow(a):
    """the Montgomery image of x^((p-3)/4) for val(a) = x R"""
    x = val(a) * RINV % P
    return pow(x, POW_E, P) * R392 % P


def is_residue(a):
    """val(a) / R is a square mod p (0 counts)"""
    x = val(a) * RINV % P
    return x == 0 or pow(x, (P - 1) // 2, P) == 1


def m_sgn0(a, b):
    """RFC 9380 sgn0 of the Fp2 element whose Montgomery images are (a, b)"""
    return o.f2sgn0((val(a) * RINV % P, val(b) * RINV % P))


def mont(x):
    """integer -> the canonical Montgomery image"""
    return carried(x % P * R392 % P)


# ---- output shapes
def shape_mul(img):
    """what a lane multiplier (and the exponentiation) returns: limbs 0..12 in [0, 2^28), |value| < 2p"""
    return all(0 <= x <= MASK for x in limbs(img)[:13]) and abs(val(img)) < 2 * P


def shape_reduce(img):
    """fp_reduce: fully carried, |value| < 0.51 p"""
    return all(0 <= x <= MASK for x in limbs(img)[:13]) and 100 * abs(val(img)) < 51 * P


def shape_row(img):
    """row_mul: limbs 0..12 in [0, 2^28) plus a carry of at most 16 in size, |value| < 2p (a b / R + (0..1) p)"""
    return all(-16 <= x < (1 << 28) + 16 for x in limbs(img)[:13]) and abs(val(img)) < 2 * P


# ---- the SSWU map's chosen inputs (tests/test_gpu_fp_ops.py and the CPU build see the same list)
def sqrt_ratio_replay(N, D):
    """sqrt_ratio_fp2_with's own formulas on integers (h2c.hpp), pow(M, (p-3)/4, p) where the device exponentiates -> the branch record
    {is_sq, qr, d_zero, g_c1_zero} and y"""
    nN, nD = (N[0] * N[0] + N[1] * N[1]) % P, (D[0] * D[0] + D[1] * D[1]) % P
    M = nN * nD % P
    t = pow(M, POW_E, P)
    s = M * t % P
    is_sq = s * s % P == M
    t2 = t * t % P
    invM = t2 if is_sq else -t2 % P
    invnD = nN * invM % P
    g = o.f2muls(o.f2mul(N, o.f2conj(D)), invnD)
    n = s * invnD % P
    c5 = pow(P - 5, (P + 1) // 4, P)
    if not is_sq:
        g, n = o.f2mul(g, o.SSWU_Z), n * c5 % P
    half = pow(2, -1, P)
    d = (g[0] + n) * half % P
    d_zero = d == 0
    if d_zero:
        d = g[0]
    t3 = pow(d, POW_E, P)
    x0 = d * t3 % P
    qr = x0 * x0 % P == d
    bh = g[1] * half % P * t3 % P
    y = (x0, bh) if qr else (bh, -x0 % P)
    return {"is_sq": is_sq, "qr": qr, "d_zero": d_zero, "g_c1_zero": g[1] == 0}, y


def sswu_replay(u):
    """sswu_g2_with on integers -> (branch record, affine point of E2')"""
    A, B, Z = o.SSWU_A, o.SSWU_B, o.SSWU_Z
    tv1 = o.f2mul(Z, o.f2sqr(u))
    tv2 = o.f2add(o.f2sqr(tv1), tv1)
    xn = o.f2mul(B, o.f2add(tv2, o.F2_ONE))
    tv2_zero = o.f2_is_zero(tv2)
    xd = o.f2mul(Z, A) if tv2_zero else o.f2mul(A, o.f2neg(tv2))
    xd2 = o.f2sqr(xd)
    D = o.f2mul(xd2, xd)
    Nn = o.f2add(o.f2mul(o.f2add(o.f2sqr(xn), o.f2mul(A, xd2)), xn), o.f2mul(B, D))
    rec, y1 = sqrt_ratio_replay(Nn, D)
    rec["tv2_zero"] = tv2_zero
    if rec["is_sq"]:
        x, y = xn, y1
    else:
        x, y = o.f2mul(tv1, xn), o.f2mul(o.f2mul(tv1, u), y1)
    if o.f2sgn0(u) != o.f2sgn0(y):
        y = o.f2neg(y)
    return rec, (o.f2mul(x, o.f2inv(xd)), y)        # the device returns (x xd, y xd^3, xd): this point in Jacobian coordinates


def real_ratio_us(want=8, seed=20261020):
    """u for which N / D = g(x1(u)) is REAL, so that sqrt_ratio_fp2_with's g has c1 = 0 and its `fp_is_zero(d)` arm is reachable: x = a + b i on
    E2' with Im(x^3 + A x + B) = 0 - with A = 240 i, B = 1012 (1 + i): 3 b a^2 + 240 a + (1012 - b^3) = 0, a quadratic in a for a chosen b - pulled
    back through x1(u) = (-B / A)(1 + 1 / tv2), tv2 = t^2 + t, t = Z u^2: two Fp2 square roots, each there about half the time."""
    A, B, Z = o.SSWU_A, o.SSWU_B, o.SSWU_Z
    rng = random.Random(seed)
    mBA = o.f2mul(o.f2neg(B), o.f2inv(A))
    out = []
    while len(out) < want:
        b = rng.randrange(1, P)
        disc = (240 * 240 - 12 * b * (1012 - pow(b, 3, P))) % P
        r = o.fp_sqrt(disc)
        if r is None:
            continue
        for sgn in (1, -1):
            a = (-240 + sgn * r) * pow(6 * b, -1, P) % P
            x = (a, b)
            gx = o.f2add(o.f2add(o.f2mul(o.f2sqr(x), x), o.f2mul(A, x)), B)
            assert gx[1] == 0
            # x = mBA (1 + 1 / tv2)  =>  tv2 = 1 / (x / mBA - 1)
            q = o.f2sub(o.f2mul(x, o.f2inv(mBA)), o.F2_ONE)
            if o.f2_is_zero(q):
                continue
            tv2 = o.f2inv(q)
            # t^2 + t - tv2 = 0  =>  t = (-1 + sqrt(1 + 4 tv2)) / 2
            sq = o.f2sqrt(o.f2add(o.F2_ONE, o.f2muls(tv2, 4)))
            if sq is None:
                continue
            for s2 in (sq, o.f2neg(sq)):
                t = o.f2muls(o.f2sub(s2, o.F2_ONE), pow(2, -1, P))
                u = o.f2sqrt(o.f2mul(t, o.f2inv(Z)))
                if u is not None and not o.f2_is_zero(u) and len(out) < want:
                    out.append(u)
    return out


def sswu_inputs():
    """-> [(name, (c0, c1) as raw images, u as integers)]: the list the issue of this test names - u = 0; a zero real / imaginary part under both
    sgn0 values; u and -u; the same residues given non-canonically; 200 random u; the real-ratio family (extended until the d = 0 arm of the
    square root is taken at least twice and left at least twice)."""
    rng = random.Random(20261021)
    out = [("zero", (0, 0))]
    for c in (1, 2, P - 1, P - 2):
        out += [("(0,%d)" % c, (0, c)), ("(%d,0)" % c, (c, 0))]
    assert {o.f2sgn0(u) for _, u in out if u[0] == 0 and u[1]} == {0, 1} and {o.f2sgn0(u) for _, u in out if u[1] == 0 and u[0]} == {0, 1}
    for i in range(4):
        u = (rng.randrange(P), rng.randrange(P))
        out += [("pm%d" % i, u), ("pm%d-" % i, o.f2neg(u))]
    out += [("rnd%d" % i, (rng.randrange(P), rng.randrange(P))) for i in range(200)]
    want = 8
    while True:
        rr = real_ratio_us(want)
        recs = [sswu_replay(u)[0] for u in rr]
        if sum(r["d_zero"] for r in recs) >= 2 and sum(not r["d_zero"] for r in recs) >= 2:
            break
        want += 4
    out += [("real%d" % i, u) for i, u in enumerate(rr)]
    rows = [(name, (mont(u[0]), mont(u[1])), u, "canon") for name, u in out]
    # the same residues in other representations: u + p in either coordinate (and the zero input as (p, -p))
    for name in ("zero", "(0,1)", "(%d,0)" % (P - 1), "pm0", "rnd0", "rnd1", "real0"):
        u = dict((n, v) for n, v in out)[name]
        c0, c1 = val(mont(u[0])), val(mont(u[1]))
        rows += [(name + " c0+p", (carried(c0 + P), mont(u[1])), u, "noncanon"), (name + " c1+p", (mont(u[0]), carried(c1 + P)), u, "noncanon"),
                 (name + " c0-p c1+p", (carried(c0 - P), carried(c1 + P)), u, "noncanon")]
    return rows


_SSWU = None


def sswu_cases():
    """(rows of sswu_inputs, the replay's branch record of each, the oracle's iso3(sswu(u)) of each): computed once per process.  The conditions the
    list has to meet are asserted here, on the CPU, before anything is handed to a device or to the CPU build; the tallies count the canonical rows
    (one per distinct u) - the non-canonical rows repeat seven of them in other representations, the zero input among them."""
    global _SSWU
    if _SSWU is None:
        rows = sswu_inputs()
        recs, want = [], []
        for name, _, u, _ in rows:
            rec, pt = sswu_replay(u)
            assert pt == o.sswu_g2(u), name                      # the replay is the map
            recs.append(rec)
            want.append(o.iso3_g2(pt))
        base = [r for r, row in zip(recs, rows) if row[3] == "canon"]
        for key in ("is_sq", "qr"):
            assert sum(r[key] for r in base) >= 50 and sum(not r[key] for r in base) >= 50, key
        assert sum(r["tv2_zero"] for r in base) == 1
        real = [r for r, row in zip(recs, rows) if row[0].startswith("real") and row[3] == "canon"]
        assert len(real) >= 8 and all(r["g_c1_zero"] for r in real)
        assert sum(r["d_zero"] for r in real) >= 2 and sum(not r["d_zero"] for r in real) >= 2
        _SSWU = (rows, recs, want)
    return _SSWU


def same_point(jac288, want):
    """the 288-byte Jacobian blst_p2 image (Montgomery R = 2^384, any partially reduced form) is the affine point `want`: X = x Z^2, Y = y Z^3"""
    r384 = pow(1 << 384, -1, P)
    c = [int.from_bytes(jac288[48 * j:48 * j + 48], "little") * r384 % P for j in range(6)]
    X, Y, Z = (c[0], c[1]), (c[2], c[3]), (c[4], c[5])
    Z2 = o.f2sqr(Z)
    return Z != (0, 0) and X == o.f2mul(want[0], Z2) and Y == o.f2mul(want[1], o.f2mul(Z2, Z))


# ---- the checks, shared by the CPU build (tests/test_fp_operands_emu.py) and the device (tests/test_gpu_fp_ops.py): `run(op, a, b, fam_a, fam_b)`
# takes the operation's name (the FPOP keys of the package), two lists of images and the names of their families, and returns the list of raw results
def _fail(op, fa, na, fb, nb, got, want, what):
    return "%s(%s:%s, %s:%s): %s - got limbs %s = %#x mod p, model %#x" % (op, fa, na, fb, nb, what, limbs(got), val(got) % P, want)


PAIRINGS = (("canon", "canon"), ("noncanon", "canon"), ("lazy", "lazy"))      # the multipliers' cross products
LANE_MULS = ("fp_mul", "fp_sqr", "fp_sqr_n1", "fp_sqr_n4", "fp_dot2")
ROW_MULS = ("row_mul", "row_sqr")


def check_multipliers(run, pairing):
    """every multiplier over the full cross product of a pairing: congruent to the model, documented output shape, lane and row forms agree"""
    fa, fb = pairing
    A, B = FAMILIES[fa], FAMILIES[fb]
    pairs = [(x, y) for x in A for y in B]
    a, b = [x[1] for x, _ in pairs], [y[1] for _, y in pairs]
    lane = run("fp_mul", a, b, fa, fb)
    row = run("row_mul", a, b, fa, fb)
    assert len(lane) == len(row) == len(pairs)
    for (x, y), gl, gr in zip(pairs, lane, row):
        want = m_mul(x[1], y[1])
        assert val(gl) % P == want, _fail("fp_mul", fa, x[0], fb, y[0], gl, want, "residue")
        assert shape_mul(gl), _fail("fp_mul", fa, x[0], fb, y[0], gl, want, "output bounds")
        assert val(gr) % P == want, _fail("row_mul", fa, x[0], fb, y[0], gr, want, "residue")
        assert shape_row(gr), _fail("row_mul", fa, x[0], fb, y[0], gr, want, "output bounds")
        assert (val(gl) - val(gr)) % P == 0
    # the dot product: pair k with pair 7 k + 3 of the same cross product
    other = [pairs[(7 * k + 3) % len(pairs)] for k in range(len(pairs))]
    a2 = [i for (x, _), (x2, _) in zip(pairs, other) for i in (x[1], x2[1])]
    b2 = [i for (_, y), (_, y2) in zip(pairs, other) for i in (y[1], y2[1])]
    for ((x, y), (x2, y2)), g in zip(zip(pairs, other), run("fp_dot2", a2, b2, fa, fb)):
        want = m_dot2(x[1], y[1], x2[1], y2[1])
        assert val(g) % P == want, _fail("fp_dot2", fa, x[0] + "|" + x2[0], fb, y[0] + "|" + y2[0], g, want, "residue")
        assert shape_mul(g), _fail("fp_dot2", fa, x[0] + "|" + x2[0], fb, y[0] + "|" + y2[0], g, want, "output bounds")
    # the squarings: every member of both families
    for f in dict.fromkeys((fa, fb)):
        imgs = [i for _, i in FAMILIES[f]]
        res = {op: run(op, imgs, imgs, f, f) for op in ("fp_sqr", "fp_sqr_n1", "fp_sqr_n4", "row_sqr")}
        for k, (name, img) in enumerate(FAMILIES[f]):
            for op, nsq in (("fp_sqr", 1), ("fp_sqr_n1", 1), ("fp_sqr_n4", 4), ("row_sqr", 1)):
                g, want = res[op][k], m_sqr_n(img, nsq)
                assert val(g) % P == want, _fail(op, f, name, f, name, g, want, "residue")
                assert (shape_row if op == "row_sqr" else shape_mul)(g), _fail(op, f, name, f, name, g, want, "output bounds")
            assert (val(res["fp_sqr"][k]) - val(res["row_sqr"][k])) % P == 0


def check_reduce(run):
    """fp_reduce over every family: residue unchanged, |r| < 0.51 p, limbs carried"""
    for f, members in FAMILIES.items():
        imgs = [i for _, i in members]
        for (name, img), g in zip(members, run("fp_reduce", imgs, imgs, f, f)):
            assert val(g) % P == val(img) % P, _fail("fp_reduce", f, name, f, name, g, val(img) % P, "residue")
            assert shape_reduce(g), _fail("fp_reduce", f, name, f, name, g, val(img) % P, "output bounds")


def check_inv(run):
    """fp_inv over canon and noncanon: a inv(a) = 1, and every representation of 0 maps to 0"""
    zeros = 0
    for f in ("canon", "noncanon"):
        imgs = [i for _, i in FAMILIES[f]]
        for (name, img), g in zip(FAMILIES[f], run("fp_inv", imgs, imgs, f, f)):
            want = m_inv(img)
            assert val(g) % P == want, _fail("fp_inv", f, name, f, name, g, want, "residue")
            assert shape_mul(g), _fail("fp_inv", f, name, f, name, g, want, "output bounds")
            if val(img) % P:
                assert m_mul(img, g) == ONE_M, (f, name)
            else:
                zeros += 1
                assert val(g) % P == 0, (f, name)
    assert zeros >= 3                                      # 0, +p, -p


def check_predicates(run):
    """fp_is_zero, fp_eq and fp2_sgn0 on (a, b) for a in noncanon and in canon, b in noncanon and in canon: every representation of a residue
    compares equal, different residues unequal; sgn0 as the oracle's, the real part = 0 given as 0, p and -p"""
    seen_eq = seen_zero_real = 0
    for fa in ("noncanon", "canon"):
        for fb in ("noncanon", "canon"):
            A = FAMILIES[fa] if fa == "noncanon" else [m for m in FAMILIES[fa] if m[0] in _NONCANON_OF]
            pairs = [(x, y) for x in A for y in FAMILIES[fb]]
            res = run("pred", [x[1] for x, _ in pairs], [y[1] for _, y in pairs], fa, fb)
            for (x, y), g in zip(pairs, res):
                w = g[0]
                assert all(v == 0 for v in g[1:]) and w < 8
                za, eq = val(x[1]) % P == 0, (val(x[1]) - val(y[1])) % P == 0
                assert bool(w & 1) == za, "fp_is_zero(%s:%s) = %d" % (fa, x[0], w & 1)
                assert bool(w & 2) == eq, "fp_eq(%s:%s, %s:%s) = %d" % (fa, x[0], fb, y[0], (w >> 1) & 1)
                assert w >> 2 == m_sgn0(x[1], y[1]), "fp2_sgn0(%s:%s, %s:%s) = %d" % (fa, x[0], fb, y[0], w >> 2)
                seen_eq += eq and x[1] != y[1]
                seen_zero_real += za and val(x[1]) != 0
    assert seen_eq >= 60 and seen_zero_real >= 100


POW_FORMS = ("fp_pow", "pow_per_row", "pow_two_rows")


def check_pow(run):
    """a^((p-3)/4) in its three device forms over canon + noncanon + pow_corner: congruent to the model, the forms agree, and the verdict derived
    from it - (a t)^2 = a exactly when a is a residue - holds for every representation of a (0, +-1 and non-residues among them)"""
    classes = set()
    for f in ("canon", "noncanon", "pow_corner"):
        imgs = [i for _, i in FAMILIES[f]]
        res = {op: run(op, imgs, imgs, f, f) for op in POW_FORMS}
        for k, (name, img) in enumerate(FAMILIES[f]):
            want = m_pow(img)
            for op in POW_FORMS:
                g = res[op][k]
                assert val(g) % P == want, _fail(op, f, name, f, name, g, want, "residue")
                assert (shape_mul if op == "fp_pow" else shape_reduce)(g), _fail(op, f, name, f, name, g, want, "output bounds")
                s = m_mul(img, g)
                assert (s * s * RINV % P == val(img) % P) == is_residue(img), (op, f, name)
            x = val(img) * RINV % P
            classes.add("0" if x == 0 else "1" if x == 1 else "-1" if x == P - 1 else "qr" if is_residue(img) else "nqr")
    assert classes == {"0", "1", "-1", "qr", "nqr"}


def check_sswu(map_fn):
    """map_fn(list of (c0, c1) image pairs, family) -> list of 288-byte Jacobian images: every point of sswu_cases() equals the oracle's
    iso3(sswu(u)) projectively; the map of -u is the negation of the map of u"""
    rows, _, want = sswu_cases()
    got = {}
    for fam in ("canon", "noncanon"):
        idx = [k for k, r in enumerate(rows) if r[3] == fam]
        for k, pt in zip(idx, map_fn([rows[k][1] for k in idx], fam)):
            got[k] = pt
    for k, row in enumerate(rows):
        assert same_point(got[k], want[k]), "sswu + iso3 of %s (%s): %s" % (row[0], row[3], got[k].hex())
    by_name = {r[0]: k for k, r in enumerate(rows)}
    for i in range(4):
        a, b = want[by_name["pm%d" % i]], want[by_name["pm%d-" % i]]
        assert b == o.g2_neg(a) and same_point(got[by_name["pm%d-" % i]], o.g2_neg(a))
    return [got[k] for k in range(len(rows))]
