// Number-theoretic transforms of MANY vectors over Fr at once (mi355_bls_fr_ntt_many, mi355_bls_fr_domain): for k vectors of n = 2^m scalars
// the values of sum_j c_j X^j over the n-th roots of unity omega^i (or over the coset g omega^i), and the exact inverse map - the bodies one
// lane carries between two barriers, written like fropen.hpp so that the host can run them (tests/host_emu/frntt.cpp walks them with 256
// emulated lanes; csrc/kernels.hip k_frntt_* with a workgroup).
//   Forms of a value: as in fropen.hpp the DATA stay PLAIN, brought below r by fr_canon_words only, and every MULTIPLIER - the twiddles
//   omega^j, the shift powers g^j, 1 / n - is in Montgomery form, so the outputs come out plain and canonical with no conversion per element.
//   The k vectors of a call are ONE array of k x n elements: bit b < m of an element's index is bit b of its place in its vector, the bits
//   from m up are the vector's number.  A radix-2 stage pairs the elements whose indices differ in one bit b < m (half-span h = 2^b):
//     decimation in frequency (DIF)   (a, b) -> (a + b, (a - b) w), stages from bit m - 1 down to 0: natural order in, bit-reversed order out
//     decimation in time (DIT)        (a, b) -> (a + b w, a - b w), stages from bit 0 up to m - 1:   bit-reversed order in, natural order out
//   with w = root^((index mod h) 2^(m - 1 - b)), read from a table of the n / 2 powers of root (omega, or 1 / omega for the inverse) that
//   k_frntt_twiddle builds once per call.  Which one runs (csrc/host_api.inc frntt_run): forward with BITREV is DIF, inverse with BITREV
//   is DIT over 1 / omega, and without BITREV both are DIF (over omega, over 1 / omega) with the bit-reversal made by the last store.
//   A PASS (k_frntt_pass) takes tp consecutive stages, bits [sigma, sigma + tp): a workgroup of 256 lanes holds 2^L elements in LDS,
//   L = clo + tp + chi <= the tile: the 2^tp elements those stages connect, for 2^clo adjacent columns (index bits [0, clo), clo <= sigma:
//   its global accesses are runs of 2^clo 32-byte elements) and 2^chi adjacent blocks above (bits [sigma + tp, sigma + tp + chi), which may
//   reach into the vector number: short vectors share a workgroup; an element of a vector >= k is a zero that is never stored).  LDS is
//   limb-major: word l of slot e at l 2^L + e, so consecutive lanes touch consecutive banks.  One barrier per stage.
//   The shift and 1 / n are an elementwise kernel of their own (k_frntt_scale: g^j before the forward passes, g^-j / n behind the inverse
//   ones), a lane taking a run of FRNTT_RUN elements with one fr_pow_u64 and a running product; the same body copies and reduces where a
//   call has no stage at all (n = 1).
// Variable time throughout: public vectors only.
#pragma once
#include "fropen.hpp"

namespace bls {

constexpr uint32_t FRNTT_LANES = 256, FRNTT_RUN = 16;
constexpr uint32_t FRNTT_ST_REDUCED = FROPEN_ST_REDUCED;                  // the status byte's bit: the same as fr_open_many's

// i with its m low bits reversed, m <= 32
BLS_HD uint64_t frntt_rev(uint64_t i, uint32_t m) {
    uint32_t v = (uint32_t)i;
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return m ? v >> (32 - m) : 0;
}
// omega_(2^m) in Montgomery form: the constant omega_(2^32) = 7^((r - 1) / 2^32) squared 32 - m times (host: once per call)
BLS_HD fr frntt_omega(uint32_t m) {
    fr w;
#pragma unroll
    for (int i = 0; i < 8; i++) w.l[i] = k::FR_OMEGA32[i];
#pragma clang loop unroll(disable)
    for (uint32_t i = m; i < 32; i++) w = fr_sqr(w);
    return w;
}

// ---- the powers of one root: the twiddle table and the domain.  Lane `run` owns entries [run FRNTT_RUN, (run + 1) FRNTT_RUN) cut to count:
// one fr_pow_u64 for the first, a running product for the rest.
// the table: root^j in Montgomery form, j < count = n / 2
BLS_HD void frntt_twiddle_run(const fr& root, uint64_t run, uint64_t count, uint32_t* tw) {
    const uint64_t lo = run * FRNTT_RUN, hi = count - lo < FRNTT_RUN ? count : lo + FRNTT_RUN;
    if (lo >= count) return;
    fr p = fr_pow_u64(root, lo);
#pragma clang loop unroll(disable)
    for (uint64_t j = lo; j < hi; j++) {
        fropen_st(tw + j * 8, p);
        p = fr_mont_mul(p, root);
    }
}
// the domain: omega^i as a canonical image at slot i, or at slot rev_m(i) (then slot s holds omega^rev_m(s)), i < n = 2^m
BLS_HD void frntt_domain_run(const fr& omega, uint64_t run, uint32_t m, bool bitrev, uint32_t* out) {
    const uint64_t n = (uint64_t)1 << m, lo = run * FRNTT_RUN, hi = n - lo < FRNTT_RUN ? n : lo + FRNTT_RUN;
    if (lo >= n) return;
    fr p = fr_pow_u64(omega, lo);
#pragma clang loop unroll(disable)
    for (uint64_t i = lo; i < hi; i++) {
        fropen_st(out + (bitrev ? frntt_rev(i, m) : i) * 8, fr_from_mont(p));
        p = fr_mont_mul(p, omega);
    }
}

// ---- the elementwise kernel's lane: run `run` of the k x n array (runs never cross a vector: a vector holds ceil(n / FRNTT_RUN) of them).
// dst_j = src_j * base * ratio^j, j the element's place in its vector; base and ratio in Montgomery form.  mult false: a copy.  use_ratio
// false: ratio is 1 and no power is made.  raw: src holds the caller's images (reduced here; -> true when one was not below r).
struct frntt_scale_args {
    uint32_t m;
    uint64_t k;
    bool raw, mult, use_ratio;
    fr base, ratio;
};
BLS_HD bool frntt_scale_run(const frntt_scale_args& a, uint64_t run, const uint32_t* src, uint32_t* dst, uint64_t& vec) {
    const uint64_t n = (uint64_t)1 << a.m, per_vec = (n + FRNTT_RUN - 1) / FRNTT_RUN;
    vec = run / per_vec;
    if (vec >= a.k) return false;
    const uint64_t lo = (run % per_vec) * FRNTT_RUN, hi = n - lo < FRNTT_RUN ? n : lo + FRNTT_RUN;
    fr p = a.base;
    if (a.mult && a.use_ratio) p = fr_mont_mul(p, fr_pow_u64(a.ratio, lo));
    uint32_t fl = 0;
#pragma clang loop unroll(disable)
    for (uint64_t j = lo; j < hi; j++) {
        const size_t e = (size_t)(vec * n + j);
        fr x = a.raw ? fropen_image(src, e, fl) : fropen_own(src, e);
        if (a.mult) x = fr_mont_mul(x, p);
        fropen_st(dst + e * 8, x);
        if (a.mult && a.use_ratio) p = fr_mont_mul(p, a.ratio);
    }
    return fl != 0;
}

// ---- a pass
// m: n = 2^m; k: the vectors of the array; the pass's stages are bits [sigma, sigma + tp); clo, chi, L as above (csrc/plan.hpp frntt_geo_for)
struct frntt_geo {
    uint32_t m, sigma, tp, clo, chi, L;
    uint64_t k;
};
// the workgroups of a pass: 2^(sigma - clo) column groups times the groups of 2^chi blocks, k 2^(m - sigma - tp) blocks in all
BLS_HD uint64_t frntt_workgroups(const frntt_geo& g) {
    const uint64_t blocks = g.k << (g.m - g.sigma - g.tp), per = (uint64_t)1 << g.chi;
    return ((blocks + per - 1) >> g.chi) << (g.sigma - g.clo);
}
// LDS slot l of workgroup w -> the element's index in the k x n array
BLS_HD uint64_t frntt_index(const frntt_geo& g, uint64_t w, uint32_t l) {
    const uint32_t lo_bits = g.sigma - g.clo;
    const uint64_t col = l & ((1u << g.clo) - 1), rest = l >> g.clo, w_lo = w & (((uint64_t)1 << lo_bits) - 1), w_hi = w >> lo_bits;
    return col | (w_lo << g.clo) | (rest << g.sigma) | (w_hi << (g.sigma + g.tp + g.chi));
}
BLS_HD fr frntt_lds_ld(const uint32_t* lds, uint32_t L, uint32_t e) {
    fr a;
#pragma unroll
    for (int i = 0; i < 8; i++) a.l[i] = lds[((uint32_t)i << L) + e];
    return a;
}
BLS_HD void frntt_lds_st(uint32_t* lds, uint32_t L, uint32_t e, const fr& a) {
#pragma unroll
    for (int i = 0; i < 8; i++) lds[((uint32_t)i << L) + e] = a.l[i];
}
// slot l from global memory (raw: the caller's images, reduced here -> true when one was not below r; vec: the element's vector, which is
// a zero and not a load from k on)
BLS_HD bool frntt_load_item(const frntt_geo& g, uint64_t w, uint32_t l, const uint32_t* src, bool raw, uint32_t* lds, uint64_t& vec) {
    const uint64_t at = frntt_index(g, w, l);
    vec = at >> g.m;
    uint32_t fl = 0;
    fr x{};
    if (vec < g.k) x = raw ? fropen_image(src, (size_t)at, fl) : fropen_own(src, (size_t)at);
    frntt_lds_st(lds, g.L, l, x);
    return fl != 0;
}
// butterfly bf (of 2^(L - 1)) of the stage at LDS bit `pos` in [clo, clo + tp): index bit b = sigma + pos - clo
template <bool DIT>
BLS_HD void frntt_butterfly(const frntt_geo& g, uint64_t w, uint32_t bf, uint32_t pos, const uint32_t* tw, uint32_t* lds) {
    const uint32_t l0 = ((bf >> pos) << (pos + 1)) | (bf & ((1u << pos) - 1)), l1 = l0 | (1u << pos);
    const uint32_t b = g.sigma + pos - g.clo;
    const uint64_t j = frntt_index(g, w, l0) & (((uint64_t)1 << b) - 1);
    const fr wj = fropen_own(tw, (size_t)(j << (g.m - 1 - b)));
    const fr x = frntt_lds_ld(lds, g.L, l0), y = frntt_lds_ld(lds, g.L, l1);
    if (DIT) {
        const fr yw = fr_mont_mul(y, wj);
        frntt_lds_st(lds, g.L, l0, fr_add(x, yw));
        frntt_lds_st(lds, g.L, l1, fr_sub(x, yw));
    } else {
        frntt_lds_st(lds, g.L, l0, fr_add(x, y));
        frntt_lds_st(lds, g.L, l1, fr_mont_mul(fr_sub(x, y), wj));
    }
}
// slot l to global memory; permute: at the bit-reversed place in its vector
BLS_HD void frntt_store_item(const frntt_geo& g, uint64_t w, uint32_t l, const uint32_t* lds, bool permute, uint32_t* dst) {
    uint64_t at = frntt_index(g, w, l);
    const uint64_t vec = at >> g.m, mask = ((uint64_t)1 << g.m) - 1;
    if (vec >= g.k) return;
    if (permute) at = (at & ~mask) | frntt_rev(at & mask, g.m);
    fropen_st(dst + (size_t)at * 8, frntt_lds_ld(lds, g.L, l));
}

}  // namespace bls
