"""What mi355_bls_fk20_open_all_many and mi355_bls_fk20_open_cells_many must give, as SCALARS: Python integers mod r with [a]G the expected
image.  csrc/fk20cells.hpp defines the call for any setup points S_i = [s_i]G, coefficients c_0 .. c_(n-1), a cell of l = 2^c points,
q = n / l and N = q 2^ext:

    h_t  = sum_{i <= n-1-l(t+1)} c_(i + l(t+1)) s_i        t = 0 .. q-1  (h_(q-1) = 0)
    pi_j = sum_t omega_N^(j t) h_t                          j = 0 .. N-1

h_scalars and pi_scalars are those two sums as written.  For an SRS s_i = tau^i the same scalars come in O(n) and O(N log N): split
i = l u + v, then h_s = block_s(tau) + tau^l h_(s+1) with block_s(tau) = sum_{v<l} c_(v + l(s+1)) tau^v, and pi is the transform of h
zero-extended to N (srs_h, srs_pi).  quotient_at is the third statement of the same number: pi_j = (p(X) div (X^l - omega_N^j))(tau).
tests/test_fk20_scalars.py holds the three against each other and against the images of tests/golden/fk20.json and fk20_cells.json.
l = 1, ext = 0 is the all-openings call.  Nothing here comes from the code under test."""
import frntt_cases as fc

R = fc.R
BITREV, H = 2, 4                                      # the flags


def h_scalars(s, c, l):
    """the defining sum over the setup's scalars s_i -> h_0 .. h_(q-1)"""
    n = len(c)
    return [sum(c[i + l * (t + 1)] * s[i] for i in range(n - l * (t + 1))) % R for t in range(n // l)]


def pi_scalars(hs, ext):
    """the defining sum -> pi_0 .. pi_(N-1), N = q 2^ext"""
    big = len(hs) << ext
    w = fc.omega(big)
    return [sum(pow(w, j * t, R) * x for t, x in enumerate(hs)) % R for j in range(big)]


def srs(tau, n):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * tau % R
    return out


def srs_h(tau, c, l):
    """h_0 .. h_(q-1) for s_i = tau^i, from the top block down"""
    n = len(c)
    q = n // l
    tl = pow(tau, l, R)
    hs = [0] * q
    for s in range(q - 2, -1, -1):
        block = 0
        for v in range(l - 1, -1, -1):                               # Horner
            block = (block * tau + c[v + l * (s + 1)]) % R
        hs[s] = (block + tl * hs[s + 1]) % R
    return hs


def srs_pi(tau, c, l, ext):
    """pi_0 .. pi_(N-1) for s_i = tau^i"""
    hs = srs_h(tau, c, l)
    return fc.ntt_fast(hs + [0] * ((len(hs) << ext) - len(hs)))


def quotient_at(c, l, a, x):
    """(p(X) div (X^l - a))(x), by long division from the top coefficient down"""
    rem, quo = [b % R for b in c], [0] * len(c)
    for d in range(len(c) - 1, l - 1, -1):
        quo[d - l] = rem[d]
        rem[d - l] = (rem[d - l] + a * rem[d]) % R
        rem[d] = 0
    return sum(b * pow(x, j, R) for j, b in enumerate(quo)) % R


def ordered(hs, pis, flags):
    """the scalars of one polynomial's output row under flags: h with H, pi_rev(j) at slot j with BITREV, pi_j otherwise"""
    if flags & H:
        return list(hs)
    if flags & BITREV:
        mb = len(pis).bit_length() - 1
        return [pis[fc.rev(j, mb)] for j in range(len(pis))]
    return list(pis)


def expected_srs(tau, polys, l, ext, flags):
    """-> per polynomial the scalars of its output images, for s_i = tau^i; polys: rows of coefficient IMAGES (an image >= r acts mod r)"""
    out = []
    for p in polys:
        c = [a % R for a in p]
        out.append(ordered(srs_h(tau, c, l), [] if flags & H else srs_pi(tau, c, l, ext), flags))
    return out


def expected_any(s, polys, l, ext, flags):
    """the same from the defining sums, for any setup scalars s"""
    out = []
    for p in polys:
        hs = h_scalars(s, [a % R for a in p], l)
        out.append(ordered(hs, [] if flags & H else pi_scalars(hs, ext), flags))
    return out
