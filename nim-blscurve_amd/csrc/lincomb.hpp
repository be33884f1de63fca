// Short linear combinations for MANY groups at once (mi355_bls_p1s_lincomb_many / mi355_bls_p2s_lincomb_many): out[g] = the affine image of
// sum_p [s_p mod 2^nbits] P_(t(p)) over the positions p of group g, with the CALLER's scalars - the bodies one lane carries, written like
// recover.hpp so that the host can run them.  Terms are numbered by POSITION in the call's sequence (group g = positions [first_g,
// first_g + len_g)); the point of position p is table entry t = idx[p], or p itself without an index array; its scalar is the 32-byte
// little-endian image at position p, never taken through idx.
//   term (plain)  [s]P by signed 4-bit windows, curve.hpp jac_mul_256_w4_body's digits, walked from window ceil(nbits / 4) down: the scalar
//                 acts as an INTEGER, so the point need not be in the prime-order subgroup (G1 always; G2 with flags 0)
//   term (psi)    G2 with MI355_BLS_LINCOMB_SUBGROUP: the scalar reduced mod r and written in base X = |x|, four digits below 2^64; psi acts on G2 as
//                 [x] = -[X], so [s]Q = d0 Q - d1 psi(Q) + d2 psi^2(Q) - d3 psi^3(Q): one four-way Straus walk of 64 doublings
//   sum           combsets.hpp combsets_sum_item<F> over the items of plan.hpp aggsets_fill, level 0 reading the products by position
//   finish        a group's sum -> its canonical affine image (all zero: infinity) and its status byte
// Variable time throughout: public scalars only.
#pragma once
#include "aggsigs.hpp"
#include "combsets.hpp"
#include "fr.hpp"
#include "toaffine.hpp"

namespace bls {

constexpr uint32_t LINCOMB_F_BAD_INDEX = 1;          // a group's flag word, as its terms' lanes set it

// the low nbits bits (1..256) of the scalar whose little-endian word i is word(i)
template <class Word>
BLS_HD void lincomb_scalar(uint32_t (&kk)[8], uint32_t nbits, Word&& word) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t lo = 32u * i, w = word(i);
        kk[i] = nbits >= lo + 32u ? w : nbits <= lo ? 0u : w & ((1u << (nbits - lo)) - 1u);
    }
}

// [k]P for k < 2^nbits: the table, digits and additions of curve.hpp jac_mul_256_w4_body (see there: bit j of `cin` is the carry INTO
// window j), but the walk starts at window top = ceil(nbits / 4) - every nibble from there up is zero, so digit `top` is the carry out of
// window top - 1 and nothing lies above it.  64-bit scalars pay 64 doublings, not 256.  Complete additions; NOT constant time.
template <class F>
BLS_MID jac<F> lincomb_mul_w4_body(const aff<F>& p, const uint32_t (&kk)[8], uint32_t nbits) {
    jac<F> T[8];
    T[0] = jac_from_aff(p);
#pragma clang loop unroll(disable)
    for (int i = 1; i < 8; i++) {
        if (i & 1)
            T[i] = jac_dbl(T[i >> 1]);              // 2, 4, 6, 8 times P
        else
            T[i] = jac_add_aff(T[i - 1], p);        // 3, 5, 7 times P
    }
    uint64_t cin = 0;
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        cin |= (uint64_t)carry << j;
        carry = ((kk[j >> 3] >> (4 * (j & 7))) & 15u) + carry > 8u;
    }
    const int top = (int)((nbits + 3u) / 4u);        // 1 .. 64
    if (top < 64) carry = (uint32_t)((cin >> top) & 1u);
    jac<F> acc = jac_select(carry != 0, T[0], jac_inf<F>());      // digit `top`
    const int wtop = (top - 1) >> 3;
#pragma clang loop unroll(disable)
    for (int w = wtop; w >= 0; w--) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (q == w) word = kk[q];
#pragma clang loop unroll(disable)
        for (int n = w == wtop ? (top - 1) & 7 : 7; n >= 0; n--) {
#pragma clang loop unroll(disable)
            for (int k4 = 0; k4 < 4; k4++) acc = jac_dbl(acc);
            const int j = 8 * w + n;
            const int d = (int)((word >> (4 * n)) & 15u) + (int)((cin >> j) & 1u) - 16 * (int)carry;
            carry = (uint32_t)((cin >> j) & 1u);
            if (d != 0) {
                jac<F> t = T[(d < 0 ? -d : d) - 1];
                if (d < 0) t = jac_neg(t);
                acc = jac_add_body(acc, t);
            }
        }
    }
    return acc;
}

// k = d[0] + d[1] X + d[2] X^2 + d[3] X^3 for a canonical k < r (8 little-endian words) and X = |x| = k::X_ABS: r = X^4 - X^2 + 1 < X^4, so
// three divisions by X leave a quotient below X.  Restoring division, a bit at a time: 768 steps of a few instructions beside a scalar
// multiplication.  The running remainder is below X < 2^64, so twice it plus a bit is below 2^65: its top bit is kept aside.
struct lincomb_digits {
    uint64_t d[4];
};
BLS_HD lincomb_digits lincomb_base_x(const uint32_t (&kk)[8]) {
    uint32_t q[8];
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = kk[i];
    lincomb_digits o;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        uint64_t rem = 0;
#pragma unroll
        for (int w = 7; w >= 0; w--) {
            const uint32_t in = q[w];
            uint32_t out = 0;
#pragma clang loop unroll(disable)
            for (int b = 31; b >= 0; b--) {
                const uint32_t over = (uint32_t)(rem >> 63);
                rem = (rem << 1) | ((in >> b) & 1u);
                const uint32_t take = over | (uint32_t)(rem >= k::X_ABS);
                if (take) rem -= k::X_ABS;
                out = (out << 1) | take;
            }
            q[w] = out;
        }
        o.d[t] = rem;
    }
    o.d[3] = (uint64_t)q[0] | ((uint64_t)q[1] << 32);
    return o;
}

// [k]Q for Q in G2 (the CALLER vouches for it) and a canonical k < r: the four base-X digits walked together, most significant window
// first.  Every digit stream has the signed 4-bit digits of curve.hpp jac_mul_u64_w4_body - 16 windows and the final carry, window 16 -
// taken from the digit and its carry bits at the window they are used.  ONE table of 1 .. 8 times Q: stream i adds
// (-1)^i psi^i(entry), psi applied to the fetched entry on the fly (psi is an endomorphism: psi([e]Q) = [e]psi(Q)).  64 doublings and at
// most 68 additions.  The accumulator can meet +- a table entry and psi-images of entries (d0 = d2, d1 = d3: it meets images of itself):
// the additions are the complete ones.
BLS_MID g2_jac lincomb_mul_psi_body(const g2_aff& q, const uint32_t (&kk)[8]) {
    const lincomb_digits dg = lincomb_base_x(kk);
    g2_jac T[8];
    T[0] = jac_from_aff(q);
#pragma clang loop unroll(disable)
    for (int i = 1; i < 8; i++) {
        if (i & 1)
            T[i] = jac_dbl(T[i >> 1]);
        else
            T[i] = jac_add_aff(T[i - 1], q);
    }
    uint32_t cin[4];                                 // bit j: the carry into window j of stream i (bit 16: its final carry)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t c = 0, carry = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            c |= carry << j;
            carry = (uint32_t)((dg.d[i] >> (4 * j)) & 15u) + carry > 8u;
        }
        cin[i] = c | (carry << 16);
    }
    g2_jac acc = jac_inf<fp2>();
#pragma clang loop unroll(disable)
    for (int j = 16; j >= 0; j--) {
        if (j < 16) {
#pragma clang loop unroll(disable)
            for (int k4 = 0; k4 < 4; k4++) acc = jac_dbl(acc);
        }
#pragma clang loop unroll(disable)
        for (int i = 0; i < 4; i++) {
            uint64_t di = 0;
            uint32_t ci = 0;
#pragma unroll
            for (int s = 0; s < 4; s++)
                if (s == i) di = dg.d[s], ci = cin[s];
            const int nib = j < 16 ? (int)((di >> (4 * (j & 15))) & 15u) : 0;
            const int d = nib + (int)((ci >> j) & 1u) - 16 * (int)((ci >> (j + 1)) & 1u);
            if (d != 0) {
                g2_jac t = T[(d < 0 ? -d : d) - 1];
#pragma clang loop unroll(disable)
                for (int s = 0; s < i; s++) t = g2_psi(t);
                if ((d < 0) != ((i & 1) != 0)) t = jac_neg(t);
                acc = jac_add_body(acc, t);
            }
        }
    }
    return acc;
}

// The term at position `pos`: its point pt(t) for t = idx[pos], or pos itself when idx == nullptr, and its masked scalar, handed to
// mul(point, words).  An index that is not below n_table is never dereferenced: LINCOMB_F_BAD_INDEX, and the product is infinity.  A zero
// scalar and the all-zero (infinity) image both give infinity without a walk.
template <class F, class Point, class Word, class Mul>
BLS_HD jac<F> lincomb_term(uint32_t pos, const uint32_t* idx, size_t n_table, uint32_t nbits, Point&& pt, Word&& word, uint32_t& flags, Mul&& mul) {
    const size_t t = idx ? (size_t)idx[pos] : (size_t)pos;
    if (t >= n_table) {
        flags |= LINCOMB_F_BAD_INDEX;
        return jac_inf<F>();
    }
    uint32_t kk[8], any = 0;
    lincomb_scalar(kk, nbits, [&](int i) { return word(pos, i); });
#pragma unroll
    for (int i = 0; i < 8; i++) any |= kk[i];
    if (!any) return jac_inf<F>();
    const aff<F> p = pt(t);
    if (aff_is_inf(p)) return jac_inf<F>();
    return mul(p, kk);
}
// plain route: the scalar as an integer
template <class F, class Point, class Word>
BLS_HD jac<F> lincomb_mul_item(uint32_t pos, const uint32_t* idx, size_t n_table, uint32_t nbits, Point&& pt, Word&& word, uint32_t& flags) {
    return lincomb_term<F>(pos, idx, n_table, nbits, pt, word, flags,
                           [&](const aff<F>& p, const uint32_t (&kk)[8]) { return lincomb_mul_w4_body(p, kk, nbits); });
}
// psi route: the scalar mod r (zero there: infinity)
template <class Point, class Word>
BLS_HD g2_jac lincomb_mul_psi_item(uint32_t pos, const uint32_t* idx, size_t n_table, uint32_t nbits, Point&& pt, Word&& word, uint32_t& flags) {
    return lincomb_term<fp2>(pos, idx, n_table, nbits, pt, word, flags, [&](const g2_aff& p, const uint32_t (&kk)[8]) {
        uint32_t red[8], any = 0;
        fr_to_words(red, fr_from_words(kk));
#pragma unroll
        for (int i = 0; i < 8; i++) any |= red[i];
        return any ? lincomb_mul_psi_body(p, red) : jac_inf<fp2>();
    });
}

// A group's end: len terms, `flags` as its terms' lanes left them, p = the sum of its products (not read when len == 0).  Status by
// precedence: AGG_BAD_INDEX, AGG_EMPTY, AGG_INFINITY, AGG_OK.  img: the 24 (G1) or 48 (G2) words of the canonical Montgomery affine image,
// all zero - the library's affine infinity - unless the status is AGG_OK.
BLS_HD void lincomb_coord(uint32_t* w, const fp& a) {
    uint32_t t[12];
    fp_to_blst(t, a);
    for (int i = 0; i < 12; i++) w[i] = t[i];
}
BLS_HD void lincomb_coord(uint32_t* w, const fp2& a) {
    lincomb_coord(w, a.c0);
    lincomb_coord(w + 12, a.c1);
}
template <class F>
struct lincomb_end {
    static constexpr int W = sizeof(F) == sizeof(fp) ? 24 : 48;
    uint32_t img[W];
    uint8_t status;
};
template <class F>
BLS_HD lincomb_end<F> lincomb_finish_item(uint32_t len, uint32_t flags, const jac<F>& p) {
    lincomb_end<F> e;
    e.status = (flags & LINCOMB_F_BAD_INDEX) ? AGG_BAD_INDEX : len == 0 ? AGG_EMPTY : jac_is_inf(p) ? AGG_INFINITY : AGG_OK;
    for (int i = 0; i < lincomb_end<F>::W; i++) e.img[i] = 0;
    if (e.status != AGG_OK) return e;
    const F zi = f_inv(p.z), zi2 = f_sqr(zi);
    lincomb_coord(e.img, f_mul(p.x, zi2));
    lincomb_coord(e.img + lincomb_end<F>::W / 2, f_mul(p.y, f_mul(zi2, zi)));
    return e;
}

}  // namespace bls
