// k G1 MSMs in one device pass (mi355_bls_p1s_mult_pippenger_many): the index arithmetic of the counting sort over VIRTUAL windows
// v = j x nwin + w (MSM j of the pass, its window w) - the bodies one lane carries, written so that the host can run them
// (tests/host_emu/msmmany.cpp).  A pass holds `pairs` (point, scalar) pairs; pair p reads scalar p of the pass.
//   owner        pair p -> its MSM j: p / n in the shared form (every MSM over the same n points), a search in the pass's offsets in the
//                ragged form (MSM j owns pairs [offs[j], offs[j + 1]); empty members own nothing)
//   point        pair p -> the point it multiplies: p - j n (shared: the points are converted once), p (ragged)
//   digit        the signed digit of window w of a scalar, as kernels.hip pip_digit defines it (plan.hpp pip_win)
//   bucket       (j, w, |digit|) -> the global bucket ((j x nwin + w) << cbk) + |digit| - 1: what k_msm_order_*, k_pip_bucket and
//                k_pip_segred(_team) index by
//   list start   where virtual window v's sorted list begins: v x n (shared), offs[j] x nwin + w x n_j (ragged: MSM j's nwin lists of n_j
//                entries follow those of the MSMs before it).  k_pipm_scan adds it to the window's bucket offsets, so k_pip_bucket - which
//                adds window x n to an offset - is launched with n = 0.
// The bounds that keep all of this in 32-bit words are plan.hpp's (MSM_MANY_PAIRS_MAX x MSM_WINDOWS_MAX < 2^31).
#pragma once
#include "fp.hpp"
#include "plan.hpp"

namespace bls {

struct many_addr {
    uint32_t pairs;      // pairs of the pass
    uint32_t k;          // MSMs of the pass
    uint32_t n;          // shared form: points per MSM (>= 1); ragged form: 0
    uint32_t nwin, cbk;  // the call's window plan
};

// offs: the ragged pass's k + 1 offsets, offs[0] = 0, non-decreasing, offs[k] = pairs (not read in the shared form); p < pairs
BLS_HD uint32_t many_owner(const many_addr& A, const uint32_t* offs, uint32_t p) {
    if (A.n) return p / A.n;
    uint32_t lo = 0, hi = A.k;                 // the largest j < k with offs[j] <= p: offs[j + 1] > p follows, so an empty member is never it
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offs[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}
BLS_HD uint32_t many_point(const many_addr& A, uint32_t p, uint32_t j) { return A.n ? p - j * A.n : p; }
BLS_HD uint32_t many_vwin(const many_addr& A, uint32_t j, uint32_t w) { return j * A.nwin + w; }
// mag = |digit| >= 1
BLS_HD uint32_t many_bucket(const many_addr& A, uint32_t j, uint32_t w, uint32_t mag) { return (many_vwin(A, j, w) << A.cbk) + (mag - 1); }
BLS_HD uint32_t many_list_start(const many_addr& A, const uint32_t* offs, uint32_t v) {
    if (A.n) return v * A.n;
    const uint32_t j = v / A.nwin, w = v - j * A.nwin, first = offs[j], len = offs[j + 1] - first;
    return first * A.nwin + w * len;
}

BLS_HD uint32_t many_win_off(const plan::pip_win& W, uint32_t w) { return w < W.wrem ? w * (W.wbase + 1) : W.wrem * (W.wbase + 1) + (w - W.wrem) * W.wbase; }
// k: the eight little-endian words of a 32-byte scalar image.  k' = (k mod 2^nbits) + H; the len bits of k' at the window's offset, minus
// the half (the top window is unbiased and takes the carry of the bias).
BLS_HD int32_t many_digit(const uint32_t k[8], const plan::pip_win& W, uint32_t w) {
    const uint32_t len = w < W.wrem ? W.wbase + 1 : W.wbase, bit0 = many_win_off(W, w), wi = bit0 >> 5, sh = bit0 & 31;
    uint32_t carry = 0, lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t b0 = (uint32_t)(32 * j), v = k[j];
        if (W.nbits <= b0) v = 0;
        else if (W.nbits < b0 + 32) v &= (1u << (W.nbits - b0)) - 1u;
        const uint64_t t = (uint64_t)v + W.H[j] + carry;
        carry = (uint32_t)(t >> 32);
        if ((uint32_t)j == wi) lo = (uint32_t)t;
        if ((uint32_t)j == wi + 1) hi = (uint32_t)t;
    }
    const uint32_t k8 = W.H[8] + carry;
    if (wi == 8) lo = k8;
    if (wi == 7) hi = k8;
    const int32_t raw = (int32_t)((uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & ((1u << len) - 1u));       // len <= 17
    return w + 1 == W.nwin ? raw : raw - (int32_t)(1u << (len - 1));
}

// The per-MSM tail of the G2 form (k_pip_tail_many_g2): ONE Horner walk over an MSM's window sums R_w from the top window down,
// acc = 2^(width of window w) acc + R_w - nbits doublings in all, whatever the number of windows.  The schedule only: which window, how many
// doublings, and whether the accumulator has started (empty top windows cost no doubling: the walk starts at the first window whose sum
// is not infinity, and an MSM of empty windows only returns infinity without one).  The point operations are the caller's:
//   Ops::point                     the accumulator's type
//   inf(), is_inf(p), window(w)    the neutral element, the test for it, R_w
//   dbl(p), add(p, q)              add must be COMPLETE: 2^width acc == +-R_w happens (tests/test_msm_many_g2_emu.py), and acc may turn infinite midway
// The device passes the 8-lane cooperative doubling and the out-of-line complete addition, the host emulation jac_dbl and jac_add.
template <class Ops>
BLS_HD typename Ops::point many_tail_walk(const plan::pip_win& W, const Ops& ops) {
    typename Ops::point acc = ops.inf();
    bool started = false;
#pragma clang loop unroll(disable)
    for (uint32_t w = W.nwin; w-- > 0;) {
        if (started) {
            const uint32_t sh = many_win_off(W, w + 1) - many_win_off(W, w);
#pragma clang loop unroll(disable)
            for (uint32_t i = 0; i < sh; i++) acc = ops.dbl(acc);
        }
        const typename Ops::point R = ops.window(w);
        if (started) {
            acc = ops.add(acc, R);
        } else if (!ops.is_inf(R)) {
            acc = R;
            started = true;
        }
    }
    return acc;
}

}  // namespace bls
