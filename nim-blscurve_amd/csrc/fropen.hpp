// Openings of MANY polynomials over Fr at once (mi355_bls_fr_open_many): for polynomial g of n scalars and its point z_g, the value
// y_g = p_g(z_g) and the quotient q_g(X) = (p_g(X) - y_g) / (X - z_g) as n canonical 32-byte images in the layout the MSM calls read - the
// bodies one lane carries between two barriers, written like recover.hpp and lincomb.hpp so that the host can run them (tests/host_emu/
// fropen.cpp walks them with 256 emulated lanes; csrc/kernels.hip k_fropen_coef / k_fropen_eval with a workgroup).
//   One workgroup of FROPEN_LANES = 256 lanes owns one polynomial; lane t owns the contiguous chunk [t L, (t + 1) L) cut to n,
//   L = ceil(n / 256).  A SINGLE very long polynomial (k = 1, n = 2^20) therefore runs on one workgroup: correct, slow; a form that spreads
//   one polynomial over several workgroups is out of scope here.
//   Forms of a value: PLAIN (the integer in [0, r)) or MONTGOMERY (fr.hpp: times 2^256).  fr_mont_mul(plain, Montgomery) is plain, so the
//   caller's images are only brought below r (fr_canon_words, no product) and every multiplier - z, its powers, the domain, the inverted
//   differences - is kept in Montgomery form: the outputs come out plain and canonical with no conversion per element.
//   coefficient form   lane: Horner over its chunk, h_t = sum c_i z^(i - t L)  |  workgroup: the suffix scan S_t = h_t + z^L S_(t+1), 8
//                      Kogge-Stone steps with z^(L 2^s)  |  lane: its chunk again from the top with the carry-in S_(t+1), emitting
//                      q_i = (the Horner value of everything above i); y = S_0.  Slot n - 1 is 0.  Two products per element.
//   evaluation form    over a domain x_i the host call has brought to Montgomery form once (k_fropen_domain).  lane: d_i = z - x_i, a zero
//                      difference (z = x_j) replaced by 1 and j remembered, the running products of its chunk stored  |  workgroup: the
//                      inclusive product scans from both ends, ONE fr_inv of the product of all n differences by lane 0, and from it
//                      1 / (lane t's product) = inv * (product of the lanes before) * (product of the lanes behind)  |  lane: its chunk
//                      from the top, 1 / d_i = run * (the stored product up to i - 1), run *= d_i - stored over the running product - and
//                      its part of sum f_i x_i / d_i  |  workgroup: the sum; y = (z^n - 1) / n * sum, or f_j  |  lane:
//                      q_i = (y - f_i) / d_i, and for z = x_j its part of sum q_i x_i, i != j  |  workgroup: q_j = -(1 / z) * that sum,
//                      1 / z = z^(n - 1).  Six products per element, seven with z in the domain.
// Variable time throughout: public polynomials only.
#pragma once
#include "fr.hpp"

namespace bls {

constexpr uint32_t FROPEN_LANES = 256, FROPEN_SCAN_STEPS = 8;
constexpr uint32_t FROPEN_ST_IN_DOMAIN = 1, FROPEN_ST_REDUCED = 2;        // the status byte's bits
constexpr uint64_t FROPEN_NO_J = ~(uint64_t)0;

// a 32-byte image at p (4-byte aligned; two 16-byte accesses where it is 16-byte aligned)
BLS_HD void fropen_ld(uint32_t (&w)[8], const uint32_t* p) {
    if (((uintptr_t)p & 15) == 0) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = p[i];
    }
}
BLS_HD void fropen_st(uint32_t* p, const fr& a) {
    if (((uintptr_t)p & 15) == 0) {
        reinterpret_cast<uint4*>(p)[0] = make_uint4(a.l[0], a.l[1], a.l[2], a.l[3]);
        reinterpret_cast<uint4*>(p)[1] = make_uint4(a.l[4], a.l[5], a.l[6], a.l[7]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = a.l[i];
    }
}
// element i of an array of images: a caller's image, brought below r (flags: FROPEN_ST_REDUCED when it was not) ...
BLS_HD fr fropen_image(const uint32_t* base, size_t i, uint32_t& flags) {
    uint32_t w[8];
    fropen_ld(w, base + i * 8);
    bool reduced;
    const fr a = fr_canon_words(w, reduced);
    if (reduced) flags |= FROPEN_ST_REDUCED;
    return a;
}
// ... or a value of the library's own workspace, as it was stored
BLS_HD fr fropen_own(const uint32_t* base, size_t i) {
    fr a;
    fropen_ld(a.l, base + i * 8);
    return a;
}

// elements per lane, and lane t's chunk [lo, hi) of [0, n)
BLS_HD size_t fropen_chunk_len(size_t n) { return (n + FROPEN_LANES - 1) / FROPEN_LANES; }
struct fropen_span {
    size_t lo, hi;
};
BLS_HD fropen_span fropen_chunk(uint32_t t, size_t n) {
    const size_t L = fropen_chunk_len(n), lo = (size_t)t * L < n ? (size_t)t * L : n;      // t L < n + 256 L: no overflow below 2^63
    return {lo, n - lo < L ? n : lo + L};
}

// One Kogge-Stone step of an inclusive scan over the workgroup's 256 values `sh`, lane t's new value: op(sh[t], sh[partner]) where the
// partner dist lanes away (behind: t + dist, a suffix scan; else t - dist) exists.  All lanes read, a barrier, all lanes write, a barrier.
template <class Op>
BLS_HD fr fropen_scan_step(const fr* sh, uint32_t t, uint32_t dist, bool behind, Op&& op) {
    if (behind) return t + dist < FROPEN_LANES ? op(sh[t], sh[t + dist]) : sh[t];
    return t >= dist ? op(sh[t], sh[t - dist]) : sh[t];
}
// one step of the tree sum that leaves the workgroup's total in sh[0]: dist = 128, 64 .. 1, a barrier behind each
BLS_HD void fropen_sum_step(fr* sh, uint32_t t, uint32_t dist) {
    if (t < dist) sh[t] = fr_add(sh[t], sh[t + dist]);
}

// ---- coefficient form
// lane t's Horner value h_t = sum over its chunk of c_i z^(i - lo), plain; zm: z in Montgomery form
BLS_HD fr fropen_coef_horner(const uint32_t* poly, fropen_span c, const fr& zm, uint32_t& flags) {
    fr h{};
#pragma clang loop unroll(disable)
    for (size_t i = c.hi; i > c.lo; i--) h = fr_add(fr_mont_mul(h, zm), fropen_image(poly, i - 1, flags));
    return h;
}
// The suffix scan's step s over sh (h_t at first): S_t += z^(L 2^s) S_(t + 2^s).  pw: z^(L 2^s) in Montgomery form; the lane squares it
// for the next step.
BLS_HD fr fropen_coef_scan_step(const fr* sh, uint32_t t, uint32_t s, const fr& pw) {
    return fropen_scan_step(sh, t, 1u << s, true, [&](const fr& mine, const fr& far) { return fr_add(mine, fr_mont_mul(far, pw)); });
}
// lane t's slots of the quotient: carry = S_(t+1), the Horner value of every coefficient above the chunk (0 for the last lane);
// q_i = the value above i, then the value takes c_i in.  Slot n - 1 gets 0, as every slot does that has nothing above it.
BLS_HD void fropen_coef_emit(const uint32_t* poly, fropen_span c, const fr& zm, fr carry, uint32_t* quot) {
    uint32_t fl = 0;
#pragma clang loop unroll(disable)
    for (size_t i = c.hi; i > c.lo; i--) {
        fropen_st(quot + (i - 1) * 8, carry);
        carry = fr_add(fr_mont_mul(carry, zm), fropen_image(poly, i - 1, fl));
    }
}

// ---- evaluation form
// a domain image to the workspace: below r, Montgomery form (k_fropen_domain, one lane per element, once per call)
BLS_HD void fropen_domain_item(const uint32_t* domain, size_t i, uint32_t* ws_dom) {
    uint32_t fl = 0;
    fropen_st(ws_dom + i * 8, fr_to_mont(fropen_image(domain, i, fl)));
}
// z^n and z^(n - 1) for n = 2^m, Montgomery form: m squarings, the product of the squares on the way being z^(2^m - 1)
struct fropen_zpow {
    fr zn, zn1;
};
BLS_HD fropen_zpow fropen_z_powers(fr zm, uint32_t m) {
    fropen_zpow o;
    o.zn1 = fr_one();
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < m; i++) {
        o.zn1 = fr_mont_mul(o.zn1, zm);
        zm = fr_sqr(zm);
    }
    o.zn = zm;
    return o;
}
// pass 1: the running products of d_i = z - x_i over the lane's chunk, a zero difference counting as 1, stored at the elements' places
// of `scan` (Montgomery form) -> the chunk's product (1 for an empty chunk).  j: set to i where d_i == 0.
BLS_HD fr fropen_eval_products(const uint32_t* ws_dom, fropen_span c, const fr& zm, uint32_t* scan, uint64_t& j) {
    const fr one = fr_one();
    fr p = one;
#pragma clang loop unroll(disable)
    for (size_t i = c.lo; i < c.hi; i++) {
        const fr d = fr_sub(zm, fropen_own(ws_dom, i));
        if (fr_is_zero(d)) j = i;
        else p = fr_mont_mul(p, d);
        fropen_st(scan + i * 8, p);
    }
    return p;
}
// 1 / (lane t's product) from the inverse of all lanes' product and the two inclusive scans (before[t] = the product of lanes 0 .. t,
// behind[t] = of lanes t .. 255)
BLS_HD fr fropen_eval_lane_inverse(const fr& inv_all, const fr* before, const fr* behind, uint32_t t) {
    fr r = inv_all;
    if (t > 0) r = fr_mont_mul(r, before[t - 1]);
    if (t + 1 < FROPEN_LANES) r = fr_mont_mul(r, behind[t + 1]);
    return r;
}
// pass 2, from the top of the chunk: run = 1 / (the running product up to i), so 1 / d_i = run * (the running product up to i - 1) and
// run *= d_i; the inverse takes the running product's place in `scan`.  -> the lane's part of sum f_i x_i / d_i over i != j, plain.
BLS_HD fr fropen_eval_invert(const uint32_t* poly, const uint32_t* ws_dom, fropen_span c, const fr& zm, fr run, uint64_t j, uint32_t* scan, uint32_t& flags) {
    const fr one = fr_one();
    fr acc{};
#pragma clang loop unroll(disable)
    for (size_t i = c.hi; i > c.lo; i--) {
        const size_t e = i - 1;
        const fr x = fropen_own(ws_dom, e);
        const fr f = fropen_image(poly, e, flags);
        if (e == j) {                                 // its difference counted as 1: run and the running product pass it unchanged
            fropen_st(scan + e * 8, one);
            continue;
        }
        const fr inv = fr_mont_mul(run, e > c.lo ? fropen_own(scan, e - 1) : one);
        run = fr_mont_mul(run, fr_sub(zm, x));
        fropen_st(scan + e * 8, inv);
        acc = fr_add(acc, fr_mont_mul(f, fr_mont_mul(x, inv)));
    }
    return acc;
}
// y from the workgroup's sum: (z^n - 1) / n * sum outside the domain (ninv: 1 / n in Montgomery form), f_j inside
BLS_HD fr fropen_eval_value(const uint32_t* poly, const fr& sum, const fr& zn, const fr& ninv, uint64_t j) {
    uint32_t fl = 0;
    if (j != FROPEN_NO_J) return fropen_image(poly, (size_t)j, fl);
    return fr_mont_mul(sum, fr_mont_mul(fr_sub(zn, fr_one()), ninv));
}
// pass 3: q_i = (y - f_i) / d_i for i != j (quot may be null: nothing is stored) -> with z in the domain the lane's part of
// sum q_i x_i over i != j, plain; 0 otherwise
BLS_HD fr fropen_eval_emit(const uint32_t* poly, const uint32_t* ws_dom, fropen_span c, const fr& y, uint64_t j, const uint32_t* scan, uint32_t* quot) {
    uint32_t fl = 0;
    fr acc{};
    if (!quot && j == FROPEN_NO_J) return acc;
#pragma clang loop unroll(disable)
    for (size_t i = c.lo; i < c.hi; i++) {
        if (i == j) continue;
        const fr q = fr_mont_mul(fr_sub(y, fropen_image(poly, i, fl)), fropen_own(scan, i));
        if (quot) fropen_st(quot + i * 8, q);
        if (j != FROPEN_NO_J) acc = fr_add(acc, fr_mont_mul(q, fropen_own(ws_dom, i)));
    }
    return acc;
}
// slot j for z = x_j: (f_i - y) x_i / (z (z - x_i)) summed over i != j is -(1 / z) sum q_i x_i; zn1 = z^(n - 1) = 1 / z
BLS_HD fr fropen_eval_slot_j(const fr& sum, const fr& zn1) { return fr_neg(fr_mont_mul(sum, zn1)); }

}  // namespace bls
