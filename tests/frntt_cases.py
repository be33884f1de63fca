"""What mi355_bls_fr_ntt_many and mi355_bls_fr_domain must give, in Python integers mod r, and the inputs the fr_ntt tests share
(tests/test_frntt_emu.py on the CPU, tests/test_gpu_fr_ntt.py and tests/test_gpu_fr_ntt_flow.py on the device).  Nothing here comes from the
code under test."""
import functools
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
INVERSE, BITREV = 1, 2                                # the flags
REDUCED = 2                                           # the status byte's bit
FLAGS = (0, INVERSE, BITREV, INVERSE | BITREV)
SHIFTS = (1, 7, R + 7)                                # an explicit 1, a coset, and the same coset by an image that is not canonical
NON_CANONICAL = (R, R + 1, (1 << 256) - 1)


def le(v):
    return int(v).to_bytes(32, "little")


def images(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def pack(rows):
    return b"".join(le(v) for row in rows for v in row)


def omega(n):
    """omega_n = 7^((r - 1) / n) for n = 2^m"""
    assert n & (n - 1) == 0 and 1 <= n <= 1 << 32
    return pow(7, (R - 1) // n, R)


def rev(i, m):
    """i with its m low bits reversed"""
    return int(format(i, "0%db" % m)[::-1], 2) if m else 0


def domain(n, bitrev=False):
    m = n.bit_length() - 1
    w = omega(n)
    return [pow(w, rev(i, m) if bitrev else i, R) for i in range(n)]


def ntt_definition(v, inverse=False, bitrev=False, shift=1):
    """the definition written out, n^2 products: forward out[i] = sum_j v[j] (g w^i)^j; the inverse is the exact inverse map (1 / n and
    g^-j included); with bitrev evaluation slot i holds the value at w^rev(i) (the forward output, the inverse input)"""
    n = len(v)
    m = n.bit_length() - 1
    w, g = omega(n), shift % R
    v = [x % R for x in v]
    if not inverse:
        out = [sum(c * pow(g * pow(w, i, R), j, R) for j, c in enumerate(v)) % R for i in range(n)]
        return [out[rev(i, m)] for i in range(n)] if bitrev else out
    vals = [v[rev(i, m)] for i in range(n)] if bitrev else v           # the value at w^i sits at slot rev(i): rev is its own inverse
    ninv, ginv, winv = pow(n, -1, R), pow(g, -1, R), pow(w, -1, R)
    return [ninv * pow(ginv, j, R) * sum(f * pow(winv, i * j, R) for i, f in enumerate(vals)) % R for j in range(n)]


def _dft(v, w):
    """sum_j v[j] w^(i j), radix 2, natural order in and out"""
    n = len(v)
    if n == 1:
        return list(v)
    even, odd = _dft(v[0::2], w * w % R), _dft(v[1::2], w * w % R)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * odd[i] % R
        out[i], out[i + n // 2] = (even[i] + x) % R, (even[i] - x) % R
        t = t * w % R
    return out


def ntt(v, inverse=False, bitrev=False, shift=1):
    """the same map: the definition up to n = 64, a recursive radix-2 transform beyond"""
    n = len(v)
    if n <= 64:
        return ntt_definition(v, inverse, bitrev, shift)
    return ntt_fast(v, inverse, bitrev, shift)


def ntt_fast(v, inverse=False, bitrev=False, shift=1):
    n = len(v)
    m = n.bit_length() - 1
    w, g = omega(n), shift % R
    v = [x % R for x in v]
    if not inverse:
        c, p = [], 1
        for x in v:
            c.append(x * p % R)
            p = p * g % R
        out = _dft(c, w)
        return [out[rev(i, m)] for i in range(n)] if bitrev else out
    vals = [v[rev(i, m)] for i in range(n)] if bitrev else v
    c = _dft(vals, pow(w, -1, R))
    out, p, ginv = [], pow(n, -1, R), pow(g, -1, R)
    for x in c:
        out.append(x * p % R)
        p = p * ginv % R
    return out


@functools.lru_cache(maxsize=None)
def random_vectors(seed, k, n):
    """k vectors of n random images below r (a tuple of tuples: shared between tests, never changed)"""
    rng = random.Random(seed)
    return tuple(tuple(rng.randrange(R) for _ in range(n)) for _ in range(k))


@functools.lru_cache(maxsize=None)
def _expected(vectors, flags, shift):
    out = [ntt(list(v), bool(flags & INVERSE), bool(flags & BITREV), 1 if shift is None else shift) for v in vectors]
    st = bytes(REDUCED if any(x >= R for x in v) else 0 for v in vectors)
    return pack(out), st, sum(1 for b in st if b)


def expected(vectors, flags=0, shift=None):
    """-> (k x n output images, status bytes, the count the call returns) for vectors whose images may be >= r; the shift sets no bit"""
    return _expected(tuple(tuple(v) for v in vectors), flags, shift)
