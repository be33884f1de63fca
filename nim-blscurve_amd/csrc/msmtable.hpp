// Fixed-base G1 MSM over a precomputed window table (mi355_bls_p1s_table_* / mi355_bls_p1s_mult_table*; plan.hpp fixed_win / fixed_for): the
// bodies one lane carries, written so that the host can run them (tests/host_emu/msmtable.cpp).
//   the table    entry w x n + i = the affine row T[w][i] = [2^(w wbits)] P_i as k_pip_convert's record: x (14 limbs, infinity flag, pad), y (14
//                limbs, 2 pad words) - 32 words.  ptab_rows_lane makes the W rows of one point.
//   the sort     a pass holds `pairs` (point, scalar) pairs over MSMs of n points each; pair p reads scalar p of the pass.
//     owner      pair p -> its MSM j = p / n; its point i = p - j n
//     digit      the signed digit of window w: msmmany.hpp many_digit under plan.hpp fixed_win (uniform windows)
//     set        (j, w) -> the bucket set j S + w mod S: the W windows of an MSM fold into its S sets, no set is shared between MSMs
//     bucket     (j, w, |digit|) -> the global bucket (set << cbk) + |digit| - 1: what k_msm_order_*, k_pip_bucket and k_pip_segred(_team) index by
//     entry      (w, i) -> the table entry w n + i the sorted word names, beside the digit's sign in bit 31
//     list start where set v's sorted list begins: MSM j's W lists of n entries follow those of the MSMs before it; inside an MSM the windows are
//                grouped by set.  k_ptab_scan adds it to the set's bucket offsets, so k_pip_bucket is launched with n = 0.
// The bounds that keep all of this in 32-bit words are plan.hpp's (FIXED_ENTRIES_MAX; a pass of one MSM, or of at most FIXED_PAIRS_MAX pairs).
#pragma once
#include "curve.hpp"
#include "msmmany.hpp"

namespace bls {

struct fixed_addr {
    uint32_t pairs;      // pairs of the pass
    uint32_t n;          // points per MSM (>= 1)
    uint32_t nwin, S;    // windows of the call, bucket sets per MSM (1 <= S <= nwin)
    uint32_t cbk;
};

BLS_HD uint32_t fixed_owner(const fixed_addr& A, uint32_t p) { return p / A.n; }
BLS_HD uint32_t fixed_point(const fixed_addr& A, uint32_t p, uint32_t j) { return p - j * A.n; }
BLS_HD uint32_t fixed_set(const fixed_addr& A, uint32_t j, uint32_t w) { return j * A.S + w % A.S; }
// mag = |digit| >= 1
BLS_HD uint32_t fixed_bucket(const fixed_addr& A, uint32_t j, uint32_t w, uint32_t mag) { return (fixed_set(A, j, w) << A.cbk) + (mag - 1); }
BLS_HD uint32_t fixed_entry(const fixed_addr& A, uint32_t w, uint32_t i) { return w * A.n + i; }
// windows of an MSM that fall into its sets 0 .. s - 1 (s <= S): set t takes the windows t, t + S, ...
BLS_HD uint32_t fixed_windows_before(const fixed_addr& A, uint32_t s) {
    const uint32_t q = A.nwin / A.S, r = A.nwin - q * A.S;
    return s * q + (s < r ? s : r);
}
BLS_HD uint32_t fixed_list_start(const fixed_addr& A, uint32_t v) {
    const uint32_t j = v / A.S, s = v - j * A.S;
    return (j * A.nwin + fixed_windows_before(A, s)) * A.n;
}
BLS_HD int32_t fixed_digit(const uint32_t k[8], const plan::pip_win& W, uint32_t w) { return many_digit(k, W, w); }

// ---- the rows of one point
BLS_HD fp ptab_ld(const uint32_t* w) {
    fp r;
#pragma unroll
    for (int i = 0; i < FP_N; i++) r.l[i] = w[i];
    BLS_SET_VB(r, 2);                                    // what ptab_rows_lane stores: reduced values and products
    return r;
}
BLS_HD void ptab_st(uint32_t* w, const fp& a) {
#pragma unroll
    for (int i = 0; i < FP_N; i++) w[i] = a.l[i];
}
// Point i of n (lane l of the launch's `cnt`): rows 0 .. nwin - 1 at tab + (w n + i) x 32 words.  The chain of (nwin - 1) x wbits doublings
// stores every row as it is reached - X, Y in the row itself, Z and the prefix product Z_0 ... Z_w (an infinite row counts as 1) in the two
// scratch columns at (w cnt + l) x 32 words - then ONE inversion of the last prefix product and a walk back (Montgomery's trick along the lane's
// own rows) bring every row to Z = 1.  An infinite row (the input, or what a point of order two doubles to) is stored as zeros with the flag.
BLS_HD void ptab_rows_lane(const g1_aff& P, uint32_t i, uint32_t n, uint32_t l, uint32_t cnt, uint32_t nwin, uint32_t wbits, uint32_t* tab, uint32_t* scratch) {
    constexpr uint32_t E = 2 * plan::FP_WORDS;
    g1_jac p = jac_from_aff(P);
    fp run = fp_one();
    for (uint32_t w = 0; w < nwin; w++) {
        if (w) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang loop unroll(disable)
#endif
            for (uint32_t d = 0; d < wbits; d++) p = jac_dbl(p);
        }
        const bool inf = jac_is_inf(p);
        const fp z = fp_select(inf, fp_one(), fp_reduce(p.z));
        run = fp_mul(run, z);
        uint32_t* row = tab + ((size_t)w * n + i) * E;
        uint32_t* col = scratch + ((size_t)w * cnt + l) * E;
        ptab_st(row, p.x);                               // reduced by the doubling
        ptab_st(row + plan::FP_WORDS, fp_reduce(p.y));
        row[FP_N] = inf ? 1u : 0u;
        ptab_st(col, z);
        ptab_st(col + plan::FP_WORDS, run);
    }
    fp inv = fp_inv(run);                                // 1 / (Z_0 ... Z_(nwin-1)): never zero
    for (uint32_t w = nwin; w-- > 0;) {
        uint32_t* row = tab + ((size_t)w * n + i) * E;
        const uint32_t* col = scratch + ((size_t)w * cnt + l) * E;
        const fp before = w ? ptab_ld(scratch + ((size_t)(w - 1) * cnt + l) * E + plan::FP_WORDS) : fp_one();
        const fp zi = fp_mul(inv, before);               // 1 / Z_w
        inv = fp_mul(inv, ptab_ld(col));
        const fp zi2 = fp_sqr(zi);
        const bool inf = row[FP_N] != 0;
        const fp x = fp_mul(ptab_ld(row), zi2), y = fp_mul(ptab_ld(row + plan::FP_WORDS), fp_mul(zi2, zi));
        ptab_st(row, fp_select(inf, fp_zero(), x));
        ptab_st(row + plan::FP_WORDS, fp_select(inf, fp_zero(), y));
    }
}

}  // namespace bls
