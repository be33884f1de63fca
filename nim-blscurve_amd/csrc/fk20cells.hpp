// The proofs of ALL cells of a polynomial at once, for MANY polynomials (mi355_bls_fk20_open_cells_many): the Feist-Khovratovich route over
// cosets.  A cell is a coset of l = 2^c evaluation points.  For setup points S_0 .. S_(n-1), n = 2^m, coefficients c_0 .. c_(n-1), q = n / l
// and N = q 2^ext cells the call is DEFINED as
//     h_s  = sum_{i=0}^{n-1-l(s+1)} [c_(i + l(s+1))] S_i     s = 0 .. q-2,   h_(q-1) = infinity
//     pi_j = sum_{s=0}^{q-1} [omega_N^(j s)] h_s              j = 0 .. N-1
// for ANY G1 points; for S_i = [tau^i]G, pi_j is the commitment to the polynomial quotient p(X) div (X^l - omega_N^j): dividing by X^l - a
// gives the quotient coefficients sum_t a^t c_(e + l(t+1)), and at tau that is sum_t a^t h_t.  It is the KZG multi-proof of the coset
// {x : x^l = omega_N^j} = {omega_(lN)^(j + N u), u < l} of the domain of n 2^ext points.  l = 1, ext = 0 is fk20.hpp's definition.
//   ORDER.  With MI355_BLS_FK20_BITREV slot j holds pi_rev(j) (rev over log2 N bits).  For n = 4 096, l = 64, ext = 1 that is PeerDAS' cell
//   order: cell i of the bit-reversed extended evaluation (8 192 points, 128 cells of 64 neighbours) is the coset x^64 = omega_128^rev7(i).
//   THE SPLIT.  Write i = l u + v, v < l.  The bound l u + v <= n-1-l(s+1) is u <= q-2-s for every v, so h_s = sum_{v<l} h^(v)_s where
//   h^(v) is fk20.hpp's Toeplitz product (its l = 1 case) of length q over the sub-setup S^(v)_u = S_(l u + v) and the sub-polynomial
//   c^(v)_u = c_(l u + v).  Each is a cyclic convolution of length 2q, and the transform is linear, so the l products are summed in the
//   Fourier domain, BEFORE the one inverse:
//     h = first q entries of NTT^-1_2q( sum_v NTT_2q(b^(v)) . NTT_2q(s^(v)) )
//   with b^(v) = fk20_circ_src and s^(v) = fk20_setup_src at length q over the sub-sequences.  What runs, per pass of whole polynomials:
//     the SETUP (once per SRS)  the l transforms NTT_2q(s^(v)), each bit-reversed within its vector, as 2n canonical affine images stored
//                               slot-major with v minor: image slot l + v, the l terms of a slot adjacent (fk20c_setup_src lays the
//                               l vectors out, p1ntt.hpp's forward DIF walk transforms them, fk20c_setup_at places the results)
//     1 the circulant layout    b^(v) / (2q) for the k l sub-polynomials straight into the Fr transform's array, vector g l + v
//                               (fk20c_circ_run: a strided gather, every image of the caller's read once), then frntt.hpp's forward DIF
//                               passes of length 2q over k l vectors, no permutation
//     2 the product and the sum [v_(g,slot,v)] X_(slot,v), a lane per term, k 2n lanes (fk20c_term + fk20_pointwise), into the product
//                               array at (g 2q + slot) l + v; then the l terms of a (polynomial, slot) are summed by a tree of
//                               FK20C_FAN-fold levels of complete additions (fk20c_sum_item), in place in the product array, the last
//                               level into the workspace.  Equal, opposite and infinite terms are ordinary operands of that addition
//     3 the inverse, length 2q  p1ntt.hpp's DIT stages over 1 / omega_2q, unscaled; entries s < q of each vector are h
//     4 the forward, length N   entries q .. N-1 of each vector become infinity (fk20c_pad), then log2 N DIF stages over omega_N and the
//                               finish.  A polynomial's vector occupies W = max(2q, N) workspace images: fk20c_at maps element e of a
//                               k x 2^a array to its place in the k x W workspace, so that for N = q the stages run on first halves
//                               (fk20_at's places), for N = 2q on the whole vector, and for N > 2q the inverse runs on the first 2q
//                               entries of vectors N apart.  With MI355_BLS_FK20_H the finish follows 3 directly: h_0 .. h_(q-1)
//   q == 1 (cell == n, and n == 1): one stage of length 2 over infinities; every output is infinity.
// Written like fk20.hpp so that the host can run the bodies (tests/host_emu/fk20cells.cpp; csrc/kernels.hip k_fk20c_*).  Variable time
// throughout: public polynomials only.  That the points are in G1 is not checked.
#pragma once
#include "fk20.hpp"

namespace bls {

constexpr uint32_t FK20C_FAN_LOG2 = 3, FK20C_FAN = 1u << FK20C_FAN_LOG2;   // the images one lane of a sum level adds

// element e of a k x 2^a array -> its place in the k x 2^w workspace, a <= w (fk20_at: w = a + 1)
BLS_HD uint64_t fk20c_at(uint32_t a, uint32_t w, uint64_t e) { return ((e >> a) << w) | (e & (((uint64_t)1 << a) - 1)); }

// ---- the setup.  Entry t < 2n of the l vectors s^(v) laid out one after the other (vector v at [v 2q, (v + 1) 2q)): -> true and i, the
// setup point S_i it holds; false: infinity.  c: l = 2^c; mq: q = 2^mq.
BLS_HD bool fk20c_setup_src(uint32_t mq, uint32_t c, uint64_t t, uint64_t& i) {
    const uint64_t q = (uint64_t)1 << mq, v = t >> (mq + 1), u = t & (2 * q - 1);
    uint64_t j;
    if (!fk20_setup_src(q, u, j)) return false;
    i = (j << c) | v;
    return true;
}
// entry t = v 2q + slot of the transformed vectors -> its image in the handle: slot l + v
BLS_HD uint64_t fk20c_setup_at(uint32_t mq, uint32_t c, uint64_t t) { return ((t & (((uint64_t)2 << mq) - 1)) << c) | (t >> (mq + 1)); }

// ---- step 1's layout: run `run` of the (k l) x 2q array (frntt_scale_run's runs: FRNTT_RUN slots of ONE vector).  polys: the caller's
// k x n images, each read exactly once (-> true when one of this run was not below r; poly: its polynomial); dst: plain canonical
// b^(v)_s / (2q), inv2q in Montgomery form.
BLS_HD bool fk20c_circ_run(uint32_t mq, uint32_t c, uint64_t k, const fr& inv2q, uint64_t run, const uint32_t* polys, uint32_t* dst, uint64_t& poly) {
    const uint64_t q = (uint64_t)1 << mq, q2 = q << 1, per_vec = (q2 + FRNTT_RUN - 1) / FRNTT_RUN;
    const uint64_t vec = run / per_vec;
    poly = vec >> c;
    if (poly >= k) return false;
    const uint64_t v = vec & (((uint64_t)1 << c) - 1);
    const uint64_t lo = (run % per_vec) * FRNTT_RUN, hi = q2 - lo < FRNTT_RUN ? q2 : lo + FRNTT_RUN;
    uint32_t fl = 0;
#pragma clang loop unroll(disable)
    for (uint64_t s = lo; s < hi; s++) {
        uint64_t j;
        fr x{};
        if (fk20_circ_src(q, s, j)) x = fr_mont_mul(fropen_image(polys, (size_t)((poly << (mq + c)) + (j << c) + v), fl), inv2q);
        fropen_st(dst + (size_t)(vec * q2 + s) * 8, x);
    }
    return fl != 0;
}

// ---- step 2.  Term e < k 2n of the product array, (g 2q + slot) l + v: where its scalar lies in the transformed (k l) x 2q array and
// which image of the handle it multiplies.
struct fk20c_term_at {
    uint64_t scalar, setup;
};
BLS_HD fk20c_term_at fk20c_term(uint32_t mq, uint32_t c, uint64_t e) {
    const uint32_t M = mq + 1;
    const uint64_t v = e & (((uint64_t)1 << c) - 1), slot = (e >> c) & (((uint64_t)1 << M) - 1), g = e >> (c + M);
    return fk20c_term_at{((((g << c) | v)) << M) | slot, (slot << c) | v};
}
// One lane of a level of the sum: the `fan` images `stride` apart from `first` on, added in order to an accumulator that starts at
// infinity - every image, the first included, goes through the complete addition (with the first image as the start value instead, hipcc
// parks four registers of the kernel in AGPRs; this form keeps them all: one addition more per lane beside a level's 255-bit walks).
template <class F, class Load>
BLS_HD jac<F> fk20c_sum_item(uint64_t first, uint64_t stride, uint32_t fan, Load&& load) {
    jac<F> acc = jac_inf<F>();
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < fan; j++) acc = jac_add_body(acc, load(first + j * stride));
    return acc;
}
// The levels of the sum over l = 2^c terms (plan.hpp fk20_cells_sum_levels): level t adds 2^fk20c_level_bits(c, t) images that lie
// 2^(t FK20C_FAN_LOG2) apart and leaves its result at the first of them; the last level stores into the workspace instead.  c == 0 is
// one level of one image: the copy.
BLS_HD uint32_t fk20c_level_bits(uint32_t c, uint32_t t) { return c - t * FK20C_FAN_LOG2 < FK20C_FAN_LOG2 ? c - t * FK20C_FAN_LOG2 : FK20C_FAN_LOG2; }

// ---- step 4's padding: element e of the k x N array, N = 2^a -> true when it is one of entries q .. N-1 of its vector
BLS_HD bool fk20c_pad(uint32_t mq, uint32_t a, uint64_t e) { return (e & (((uint64_t)1 << a) - 1)) >= ((uint64_t)1 << mq); }

}  // namespace bls
