// Per-batch verdicts for MANY batches at once (mi355_bls_batch_verify_many_each): batchVerify (bls_batch_verifier.nim:420-495) for k batches of
// 320-byte SignatureSet records in one device pass, every batch as a product of its own - the bodies one lane carries, written so that the
// host can run them.  Batch b is one group of the per-group path (csrc/aggveach.hpp):
//   pairs_b   = ([r_i]PK_i, H(m_i)) for its sets i, r_i the scalar set i has in a batchVerify of batch b alone
//   sigpair_b = (-G1, S_b),  S_b = sum_{i in b} [r_i]S_i
//   value_b   = final_exp( conj( Horner_s  L_s(sigpair_b) * prod_i L_s(pairs_b,i) ) )
//   verdict_b = value_b == 1 and batch b has a set and no key of it is the point at infinity
// e(-G1, S_b) = prod_i e(-[r_i]G1, S_i), so value_b is the value the single-batch path reaches through its bucket fold, bit for bit after
// the final exponentiation.  [r_i]PK_i is k_pkmul's, [r_i]S_i combsets_mul_item's, S_b a segmented sum of combsets_sum_item; what is new
// here is the lane that joins them: a pair slot's setup.
#pragma once
#include "curve.hpp"

namespace bls {

// The 24 words of a record's key are the blst_p1_affine image of infinity: all zero (what combsets_check_item asks of a member's key).
// update() refuses such a key (BLST_PK_IS_INFINITY), so the batch that holds it verifies false whatever its product is.
BLS_HD bool manyeach_key_is_inf(const uint32_t* rec) {
    uint32_t any = 0;
    for (int i = 0; i < 24; i++) any |= rec[i];
    return any == 0;
}
// The group of the slice that pair slot i < (sets of the slice) belongs to: the last group whose first pair is not behind i.
// first(l): the first pair of group l, l < ng (ascending; ng >= 1 and first(0) == 0).
template <class First>
BLS_HD uint32_t manyeach_group_of(uint32_t i, uint32_t ng, First&& first) {
    uint32_t lo = 0, hi = ng - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (first(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// A batch's signature pair as the line kernels take a pair: P = -G1 (Jacobian, Z = 1), Q = the batch's signature sum as the segmented sum
// left it (Jacobian, any Z; Z == 0 - every signature of the batch at infinity, or terms that cancel - makes the pair contribute 1).
struct manyeach_pair {
    g1_jac p;
    g2_jac q;
};
BLS_HD manyeach_pair manyeach_sig_pair(const g2_jac& sum) {
    return manyeach_pair{g1_jac{fp_from_const(k::G1_X), fp_from_const(k::G1_NEG_Y), fp_one()}, sum};
}

}  // namespace bls
