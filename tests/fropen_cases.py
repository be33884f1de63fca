"""What mi355_bls_fr_open_many must give, in Python integers mod r, and the inputs the fr_open tests share (tests/test_fropen_emu.py on the
CPU, tests/test_gpu_fr_open.py and tests/test_gpu_fr_open_flow.py on the device).  Nothing here comes from the code under test."""
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_BOTH = (1, 2, 3, 255, 256, 257, 512, 4096)          # the sizes of the coefficient form ...
N_EVAL = (1, 2, 256, 512, 4096)                       # ... and those of them the evaluation form takes (powers of two)
IN_DOMAIN, REDUCED = 1, 2                             # the status byte's bits


def le(v):
    """the 32-byte little-endian image of an integer below 2^256, as it stands (not reduced)"""
    return int(v).to_bytes(32, "little")


def images(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def domain(n, bit_reversed=False):
    """the n distinct n-th roots of unity of Fr (7 generates Fr*), in natural or bit-reversed order"""
    w = pow(7, (R - 1) // n, R)
    assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
    xs = [1] * n
    for i in range(1, n):
        xs[i] = xs[i - 1] * w % R
    if bit_reversed:
        bits = n.bit_length() - 1
        xs = [xs[int(format(i, "0%db" % bits)[::-1], 2)] if bits else xs[i] for i in range(n)]
    return xs


def coef_open(c, z):
    """p = sum c_i X^i -> (p(z), the n slots of the quotient: q_(i-1) = c_i + z q_i, slot n - 1 = 0)"""
    n = len(c)
    q = [0] * n
    carry = 0
    for i in range(n - 1, 0, -1):
        carry = (c[i] + carry * z) % R
        q[i - 1] = carry
    return (c[0] + carry * z) % R, q


def eval_weights(xs, z):
    """per z: (j or None, x_i / (z - x_i) with slot j zero, 1 / (x_i - z) with slot j zero)"""
    z %= R
    j = xs.index(z) if z in set(xs) else None
    inv = [0 if i == j else pow((z - x) % R, -1, R) for i, x in enumerate(xs)]
    return j, [x * v % R for x, v in zip(xs, inv)], [(R - v) % R for v in inv]


def eval_open(f, xs, z, weights=None):
    """f_i = p(x_i) over the n-th roots of unity xs -> (p(z), the n slots (f_i - y) / (x_i - z); slot j for z = x_j by the issue's sum)"""
    n = len(xs)
    z %= R
    j, w, neg_inv = weights or eval_weights(xs, z)
    if j is None:
        y = (pow(z, n, R) - 1) * pow(n, -1, R) % R * (sum(a * b for a, b in zip(f, w)) % R) % R
    else:
        y = f[j] % R
    q = [(a - y) * v % R for a, v in zip(f, neg_inv)]
    if j is not None:
        q[j] = sum((a - y) * b for i, (a, b) in enumerate(zip(f, w)) if i != j) % R * pow(z, -1, R) % R
    return y, q


def interpolate(f, xs):
    """the coefficients of the polynomial of degree < n with p(x_i) = f_i, by the inverse DFT written out (n <= 256: n^2 products)"""
    n = len(xs)
    ninv = pow(n, -1, R)
    return [ninv * sum(fi * pow(x, (n - m) % n, R) for fi, x in zip(f, xs)) % R for m in range(n)]


def evaluate(c, x):
    y = 0
    for a in reversed(c):
        y = (y * x + a) % R
    return y


def random_call(seed, n, k, z_pool):
    """k polynomials of n random images below r, their z drawn in turn from z_pool -> (polys as lists, zs)"""
    rng = random.Random(seed)
    return [[rng.randrange(R) for _ in range(n)] for _ in range(k)], [z_pool[g % len(z_pool)] for g in range(k)]


def pack(rows):
    return b"".join(le(v) for row in rows for v in row)


def expected(polys, zs, xs=None):
    """-> (ys bytes, quotients bytes, status bytes, the count the call returns) for images that may be >= r"""
    ys, qs, st = [], [], []
    cache = {}
    for p, z in zip(polys, zs):
        red = [v % R for v in p]
        bits = REDUCED if (z >= R or any(v >= R for v in p)) else 0
        if xs is None:
            y, q = coef_open(red, z % R)
        else:
            if z % R not in cache:
                cache[z % R] = eval_weights(xs, z)
            y, q = eval_open(red, xs, z, cache[z % R])
            bits |= IN_DOMAIN if cache[z % R][0] is not None else 0
        ys.append(y), qs.append(q), st.append(bits)
    return pack([ys]), pack(qs), bytes(st), sum(1 for b in st if b & REDUCED)
