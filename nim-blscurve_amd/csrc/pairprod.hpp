// Pairing-product checks over pairs the caller holds (mi355_bls_pairing_check_each, mi355_bls_pairing_products,
// mi355_bls_batch_pairing_check; the device counterpart of blst_miller_loop_n + blst_final_exp + blst_fp12_finalverify with
// blst_p1_affine_in_g1 / blst_p2_affine_in_g2 in front, blst_abi.nim:294,317,453-461): the bodies one lane carries for one pair slot,
// written so that the host can run them.
//   value_g   = final_exp( conj( Horner_s  prod_j L_s(P_gj, Q_gj) ) )      a group of the per-group path (csrc/aggveach.hpp) with no signature pair
//   verdict_g = value_g == 1 and no pair of the group failed validation     (the empty group: the empty product, 1)
//   blinded   : one value over all pairs ([r_g]P_gj, Q_gj), r_g the group's 64-bit scalar; [r]P is k_pkmul's
// A pair with an operand at infinity (the all-zero affine image) has line_one() lines in the line store and contributes 1, as
// blst_miller_loop_n skips it.  A pair that fails validation is given infinite operands: its own coordinates never reach the line kernels.
#pragma once
#include "deser.hpp"
#include "manyeach.hpp"

namespace bls {

enum pairprod_status : uint8_t {
    PAIRPROD_OK = 0,
    PAIRPROD_P_OFF_CURVE = 1,
    PAIRPROD_P_NOT_IN_G1 = 2,
    PAIRPROD_Q_OFF_CURVE = 3,
    PAIRPROD_Q_NOT_IN_G2 = 4,
};

// y^2 == x^3 + b, the comparison g1_deserialize / g2_deserialize make for the uncompressed wire form (BLST_POINT_NOT_ON_CURVE)
BLS_HD bool pairprod_g1_on_curve(const g1_aff& p) {
    const fp rhs = fp_add(fp_mul(fp_sqr(p.x), p.x), fp_from_const(k::B1));
    return fp_eq(fp_sqr(p.y), rhs);
}
BLS_HD bool pairprod_g2_on_curve(const g2_aff& q) {
    const fp2 b2{fp_from_const(k::B1), fp_from_const(k::B1)};                  // 4(1 + u)
    const fp2 rhs = fp2_add(fp2_mul(fp2_sqr(q.x), q.x), b2);
    return fp2_eq(fp2_sqr(q.y), rhs);
}
// MI355_BLS_PAIR_VALIDATE: every finite operand on its curve and in its subgroup (deser.hpp's endomorphism tests); P first.  Infinity passes.
BLS_HD uint8_t pairprod_validate(const g1_aff& p, const g2_aff& q) {
    if (!aff_is_inf(p)) {
        if (!pairprod_g1_on_curve(p)) return PAIRPROD_P_OFF_CURVE;
        if (!g1_in_subgroup(p)) return PAIRPROD_P_NOT_IN_G1;
    }
    if (!aff_is_inf(q)) {
        if (!pairprod_g2_on_curve(q)) return PAIRPROD_Q_OFF_CURVE;
        if (!g2_in_subgroup(q)) return PAIRPROD_Q_NOT_IN_G2;
    }
    return PAIRPROD_OK;
}
// The pair as the line kernels take it (Jacobian, Z = 1; Z = 0 for the point at infinity).  status != 0: both operands infinite.
struct pairprod_pair {
    g1_jac p;
    g2_jac q;
};
BLS_HD pairprod_pair pairprod_operands(const g1_aff& p, const g2_aff& q, uint8_t status) {
    if (status != PAIRPROD_OK) return pairprod_pair{jac_inf<fp>(), jac_inf<fp2>()};
    return pairprod_pair{jac_from_aff(p), jac_from_aff(q)};
}
// The blinded form's key slot: the 24 words k_pkmul reads as a key.  A failed pair's are zero (the image of infinity: [r]inf = inf).
BLS_HD uint32_t pairprod_key_word(const uint32_t* p1_words, int j, uint8_t status) { return status != PAIRPROD_OK ? 0u : p1_words[j]; }
// A group scalar expanded to its pairs: pair slot i of a slice whose groups start at first(l), l < ng (ascending, first(0) == 0; empty
// groups have no entry), and have the numbers number(l) in the call -> r[number(group of i)].
template <class First, class Number>
BLS_HD uint64_t pairprod_scalar_of(uint32_t i, uint32_t ng, First&& first, Number&& number, const uint64_t* r) {
    return r[number(manyeach_group_of(i, ng, first))];
}

}  // namespace bls
