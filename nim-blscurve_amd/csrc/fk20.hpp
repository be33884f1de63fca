// All n openings of a polynomial over the n-th roots of unity at once, for MANY polynomials (mi355_bls_fk20_open_all_many): the
// Feist-Khovratovich route.  For setup points S_0 .. S_(n-1), n = 2^m, and coefficients c_0 .. c_(n-1) the call is DEFINED as
//     h_t  = sum_{i=0}^{n-2-t} [c_(i+t+1)] S_i     t = 0 .. n-2,   h_(n-1) = infinity
//     pi_l = sum_{t=0}^{n-1} [omega_n^(l t)] h_t   l = 0 .. n-1
// for ANY G1 points; for S_j = [tau^j]G, pi_l is the commitment to (p(X) - p(omega^l)) / (X - omega^l), the KZG proof at omega^l.
//   The h_t are a Toeplitz product, which a cyclic convolution of length 2n carries: with
//     s^_u = S_(n-2-u) for u <= n-2, infinity for n-1 <= u < 2n          (fk20_setup_src)
//     b    = [c_(n-1), 0 (n times), c_0, ..., c_(n-2)]                   (fk20_circ_src)
//   (b * s^)_t = sum_u b_((t-u) mod 2n) s^_u.  Put i = n-2-u: the index t-u = t-n+2+i is 0 for i = n-2-t, where b gives c_(n-1) =
//   c_(i+t+1); it is in 1 .. t <= n-1 for larger i, where b is 0; and it is negative for smaller i, where b_(2n+t-u) = c_(n-1+t-u) =
//   c_(i+t+1).  So (b * s^)_t = h_t for t < n, and t = n-1 meets nothing but zeros: h_(n-1) comes out as infinity by itself.
//   Hence h = the first n entries of NTT^-1_2n(NTT_2n(b) . NTT_2n(s^)), and pi = NTT_n(h).  What runs, per pass of whole polynomials:
//     the SETUP (once per SRS)  NTT_2n(s^) as canonical affine images in BIT-REVERSED order: p1ntt.hpp's forward DIF walk, no permutation
//     1 the circulant layout    b / (2n) as plain canonical scalars straight into the Fr transform's array (fk20_circ_run), then frntt.hpp's
//                               forward DIF passes of length 2n, no permutation: slot s holds NTT_2n(b)_rev(s) / (2n), the setup's order.
//                               1 / (2n) rides on the layout's one Fr product per coefficient - the transform is linear - so the point
//                               inverse below has NO scaled stage
//     2 the pointwise product   [v_s] X_s for every slot, a lane each, by curve.hpp's affine-base window walk (fk20_pointwise), into the
//                               Jacobian workspace
//     3 the inverse, length 2n  p1ntt.hpp's DIT stages over 1 / omega_2n from bit 0 up to bit m: bit-reversed in, natural order out,
//                               unscaled.  Entries t < n of each vector are h; the others are computed and never read (the last stage's
//                               difference costs one complete addition beside a 255-bit walk: no kernel of its own)
//     4 the forward, length n   p1ntt.hpp's DIF stages over omega_n on the FIRST n entries of each 2n-vector where they lie (fk20_at maps
//                               the element of a k x n array to its place in the k x 2n workspace): no affine round trip, no copy
//     the finish                p1ntt_finish_run over the same mapping: natural order where the store permutes, bit-reversed with
//                               MI355_BLS_FK20_BITREV; with MI355_BLS_FK20_H directly behind 3, h in natural order
//   n == 1: one stage of length 2 over infinities, no forward stage; every output is infinity.
// Written like p1ntt.hpp so that the host can run the bodies (tests/host_emu/fk20.cpp; csrc/kernels.hip k_fk20_*).  Variable time
// throughout: public polynomials only.  That the points are in G1 is not checked.
#pragma once
#include "p1ntt.hpp"

namespace bls {

constexpr uint32_t FK20_ST_REDUCED = FRNTT_ST_REDUCED;                    // the status byte's bit: fr_ntt_many's

// slot u < 2n of s^: -> true and j, the setup point S_j it holds; false: infinity
BLS_HD bool fk20_setup_src(uint64_t n, uint64_t u, uint64_t& j) {
    if (u + 2 > n) return false;
    j = n - 2 - u;
    return true;
}
// slot s < 2n of b: -> true and j, the coefficient c_j it holds; false: zero
BLS_HD bool fk20_circ_src(uint64_t n, uint64_t s, uint64_t& j) {
    if (s == 0) {
        j = n - 1;
        return true;
    }
    if (s <= n) return false;
    j = s - n - 1;
    return true;
}
// element e of the k x n array of first halves -> its place in the k x 2n workspace
BLS_HD uint64_t fk20_at(uint32_t m, uint64_t e) { return ((e >> m) << (m + 1)) | (e & (((uint64_t)1 << m) - 1)); }

// ---- step 1's layout: run `run` of the k x 2n array (frntt_scale_run's runs: FRNTT_RUN slots of ONE vector).  polys: the caller's k x n
// images, each read exactly once (-> true when one of this run was not below r; vec: its polynomial); dst: plain canonical b_s / (2n),
// inv2n in Montgomery form.
BLS_HD bool fk20_circ_run(uint32_t m, uint64_t k, const fr& inv2n, uint64_t run, const uint32_t* polys, uint32_t* dst, uint64_t& vec) {
    const uint64_t n = (uint64_t)1 << m, n2 = n << 1, per_vec = (n2 + FRNTT_RUN - 1) / FRNTT_RUN;
    vec = run / per_vec;
    if (vec >= k) return false;
    const uint64_t lo = (run % per_vec) * FRNTT_RUN, hi = n2 - lo < FRNTT_RUN ? n2 : lo + FRNTT_RUN;
    uint32_t fl = 0;
#pragma clang loop unroll(disable)
    for (uint64_t s = lo; s < hi; s++) {
        uint64_t j;
        fr x{};
        if (fk20_circ_src(n, s, j)) x = fr_mont_mul(fropen_image(polys, (size_t)(vec * n + j), fl), inv2n);
        fropen_st(dst + (size_t)(vec * n2 + s) * 8, x);
    }
    return fl != 0;
}

// ---- step 2: [v]X for one slot.  The affine-base walk has no branch for a base at infinity: it is answered here.
template <class F>
BLS_HD jac<F> fk20_pointwise(const aff<F>& x, const fr& v) {
    if (aff_is_inf(x)) return jac_inf<F>();
    uint32_t kk[8];
#pragma unroll
    for (int i = 0; i < 8; i++) kk[i] = v.l[i];
    return jac_mul_256_w4_body(x, kk);
}

}  // namespace bls
