// Fr = GF(r), the scalar field of BLS12-381 (r = k::R_ORDER, 255 bits), for the Lagrange coefficients of csrc/recover.hpp.
//
// Representation: 8 saturated 32-bit limbs, Montgomery form with R = 2^256, always reduced into [0, r).  Unlike Fp (fp.hpp: 28-bit signed
// limbs, lazily reduced, every multiply-add counted) this field is a rounding error of the work it serves - a few dozen multiplications and
// one inversion beside a 255-bit G2 scalar multiplication - so it is the textbook form in plain C++: operand-scanning Montgomery products
// with 64-bit accumulators, one conditional subtraction behind every operation, Fermat inversion.  No inline assembly.
// Variable time, like everything on this device: ids are public, secret keys never come here.
#pragma once
#include "fp.hpp"

namespace bls {

struct fr {
    uint32_t l[8];
};

// a >= r ? a - r : a, for a < 2 r given as 8 limbs and the carry word above them
BLS_HD fr fr_cond_sub(const uint32_t (&t)[8], uint32_t top) {
    uint32_t d[8];
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t s = (uint64_t)t[i] - k::R_ORDER[i] - borrow;
        d[i] = (uint32_t)s;
        borrow = (s >> 63) & 1;
    }
    const bool keep = top == 0 && borrow != 0;       // t < r
    fr o;
#pragma unroll
    for (int i = 0; i < 8; i++) o.l[i] = keep ? t[i] : d[i];
    return o;
}

// a b / R mod r for a < 2^256 and b < r (or the other way round): the product is below r R, so the reduced sum is below 2 r
// By value and fully unrolled: one out-of-line copy whose operands and 10-word accumulator stay in registers (128 multiply-adds).
BLS_HDN fr fr_mont_mul(fr a, fr b) {
    uint32_t t[10] = {};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t s = (uint64_t)a.l[j] * b.l[i] + t[j] + c;
            t[j] = (uint32_t)s;
            c = s >> 32;
        }
        uint64_t s = (uint64_t)t[8] + c;
        t[8] = (uint32_t)s;
        t[9] = (uint32_t)(s >> 32);
        const uint32_t m = t[0] * k::FR_N0;
        c = ((uint64_t)m * k::R_ORDER[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            s = (uint64_t)m * k::R_ORDER[j] + t[j] + c;
            t[j - 1] = (uint32_t)s;
            c = s >> 32;
        }
        s = (uint64_t)t[8] + c;
        t[7] = (uint32_t)s;
        t[8] = t[9] + (uint32_t)(s >> 32);
    }
    const uint32_t lo[8] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]};
    return fr_cond_sub(lo, t[8]);
}

BLS_HD fr fr_mul(const fr& a, const fr& b) { return fr_mont_mul(a, b); }

// ANY 256-bit value, as 8 little-endian words or 32 little-endian bytes, reduced mod r: one Montgomery product with R^2 mod r
BLS_HD fr fr_from_words(const uint32_t (&w)[8]) {
    fr x, rr;
#pragma unroll
    for (int i = 0; i < 8; i++) x.l[i] = w[i], rr.l[i] = k::FR_RR[i];
    return fr_mont_mul(x, rr);
}
BLS_HD fr fr_from_le32(const uint8_t* b) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
    return fr_from_words(w);
}
// the canonical value in [0, r), little-endian words
BLS_HD void fr_to_words(uint32_t (&w)[8], const fr& a) {
    fr one{};
    one.l[0] = 1;
    const fr v = fr_mont_mul(a, one);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = v.l[i];
}
BLS_HD fr fr_one() {
    uint32_t w[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    return fr_from_words(w);
}

BLS_HD bool fr_is_zero(const fr& a) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= a.l[i];
    return any == 0;
}
BLS_HD fr fr_add(const fr& a, const fr& b) {
    uint32_t t[8];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t s = (uint64_t)a.l[i] + b.l[i] + c;
        t[i] = (uint32_t)s;
        c = s >> 32;
    }
    return fr_cond_sub(t, (uint32_t)c);
}
BLS_HD fr fr_sub(const fr& a, const fr& b) {
    uint32_t d[8];
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t s = (uint64_t)a.l[i] - b.l[i] - borrow;
        d[i] = (uint32_t)s;
        borrow = (s >> 63) & 1;
    }
    fr o;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {                     // + r where the difference went below zero
        const uint64_t s = (uint64_t)d[i] + (borrow ? k::R_ORDER[i] : 0u) + c;
        o.l[i] = (uint32_t)s;
        c = s >> 32;
    }
    return o;
}
// a^(r - 2): 1 / a, and 0 for a = 0.  Square and multiply from the top bit of the exponent (bit 254); the exponent is shifted out of its
// eight words a bit at a time, so no array is indexed by the loop counter.
BLS_HDN fr fr_inv(fr a) {
    // r - 2: word 0 of r is 1, so it becomes 0xffffffff and word 1 gives up the borrow
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = i == 0 ? 0xffffffffu : i == 1 ? k::R_ORDER[1] - 1u : k::R_ORDER[i];
    fr acc = a;
#pragma clang loop unroll(disable)
    for (int i = 255; i >= 0; i--) {
        const uint32_t bit = e[7] >> 31;
#pragma unroll
        for (int j = 7; j > 0; j--) e[j] = (e[j] << 1) | (e[j - 1] >> 31);
        e[0] <<= 1;
        if (i >= 254) continue;                       // bit 255 is 0, bit 254 is the leading 1: acc = a
        acc = fr_mont_mul(acc, acc);
        if (bit) acc = fr_mont_mul(acc, a);
    }
    return acc;
}

// ---- what the vectors of csrc/fropen.hpp need beside the above (which stays as it is: the recovery depends on it bit for bit)
BLS_HD fr fr_neg(const fr& a) { return fr_sub(fr{}, a); }
BLS_HD fr fr_sqr(const fr& a) { return fr_mont_mul(a, a); }
// ANY 256-bit value -> the value in [0, r), in the SAME form (no Montgomery factor comes or goes): 2^256 < 3 r, so two conditional
// subtractions.  reduced: the value was >= r.
BLS_HD fr fr_canon_words(const uint32_t (&w)[8], bool& reduced) {
    const fr a = fr_cond_sub(w, 0);
    const fr b = fr_cond_sub(a.l, 0);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= b.l[i] ^ w[i];
    reduced = diff != 0;
    return b;
}
// a value in [0, r) to Montgomery form and back: a chunk converts once.  A product of a plain value and a Montgomery one is plain.
BLS_HD fr fr_to_mont(const fr& a) { return fr_from_words(a.l); }
BLS_HD fr fr_from_mont(const fr& a) {
    fr o;
    fr_to_words(o.l, a);
    return o;
}
// a^e for a in Montgomery form, e >= 0 (a^0 = 1); square and multiply from the low bit
BLS_HD fr fr_pow_u64(fr a, uint64_t e) {
    fr acc = fr_one();
#pragma clang loop unroll(disable)
    for (; e; e >>= 1) {
        if (e & 1) acc = fr_mont_mul(acc, a);
        a = fr_mont_mul(a, a);
    }
    return acc;
}

}  // namespace bls
