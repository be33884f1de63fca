// Threshold-signature recovery for MANY groups at once (mi355_bls_recover_signature_sets): recover(signs, ids) of blst_recovery.nim:150-156,
// i.e. lagrangeInterpolation (:90-121) at 0 in the exponent - the bodies one lane carries, written like aggsigs.hpp / combsets.hpp so that
// the host can run them.  Members are numbered by POSITION in the call's member sequence (group g = positions [first_g, first_g + len_g));
// ids[p] is the 32-byte little-endian blst_scalar of position p, taken mod r (fr_from_le32).
//   coefficient  for the member at `self` of a group with ids x_first .. x_(first+count-1):  a = prod x_j,  b = x_self prod_(j != self) (x_j - x_self),
//                l = a / b  (:101-118); O(count) products per member, O(t^2) per group as in the reference
//   product      [l] S for the member's share S: curve.hpp jac_mul_256_w4
//   sum          combsets.hpp combsets_sum_item<fp2> over the items of plan.hpp aggsets_fill, level 0 reading the products by position
//   finish       a group's sum -> its blst_p2_affine image, its 96-byte wire form and its status byte
// Variable time throughout: shares of a SIGNATURE and public ids only.  The secret-key half of blst_recovery.nim (genSecretShare,
// recover(secrets, ids), add) stays on the CPU.
#pragma once
#include "aggsigs.hpp"
#include "fr.hpp"

namespace bls {

constexpr uint8_t REC_ZERO_ID = 6, REC_DUP_ID = 7;                               // status bytes beyond aggsets.hpp's AGG_* (4 and 5 are COMB_* / DESER_*)
constexpr uint32_t REC_F_BAD_INDEX = 1, REC_F_ZERO_ID = 2, REC_F_DUP_ID = 4;     // a group's flag word, as its members' lanes set it

struct fr_words {
    uint32_t w[8];
};

// The canonical words of the coefficient of the member at position `self`; load_id(pos) -> fr.  A group of one: coefficient 1 whatever the
// id (the reference returns the share before it looks at the id, :95-96).  Otherwise a == 0 raises REC_F_ZERO_ID, some x_j == x_self with
// j != self raises REC_F_DUP_ID, and a flagged member's coefficient is 0.
template <class LoadId>
BLS_HD fr_words recover_coeff_item(uint32_t self, uint32_t first, uint32_t count, LoadId&& load_id, uint32_t& flags) {
    fr_words o{};
    if (count == 1) {
        o.w[0] = 1;
        return o;
    }
    const fr xs = load_id(self);
    fr a = fr_one(), b = xs;
    uint32_t fl = 0;
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < count; j++) {
        const fr x = load_id(first + j);
        a = fr_mul(a, x);
        if (first + j == self) continue;
        const fr d = fr_sub(x, xs);
        if (fr_is_zero(d)) fl |= REC_F_DUP_ID;
        b = fr_mul(b, d);
    }
    if (fr_is_zero(a)) fl |= REC_F_ZERO_ID;
    flags |= fl;
    if (fl) return o;
    fr_to_words(o.w, fr_mul(a, fr_inv(b)));
    return o;
}

// [coeff] S for the share at position `pos`: S = sig(t) with t = idx[pos], or pos itself when idx == nullptr.  An index that is not below
// n_table is never dereferenced: REC_F_BAD_INDEX, and the product is infinity.  The all-zero (infinity) image gives infinity.
template <class LoadSig>
BLS_HD g2_jac recover_mul_item(const fr_words& coeff, uint32_t pos, const uint32_t* idx, size_t n_table, LoadSig&& sig, uint32_t& flags) {
    const size_t t = idx ? (size_t)idx[pos] : (size_t)pos;
    if (t >= n_table) {
        flags |= REC_F_BAD_INDEX;
        return jac_inf<fp2>();
    }
    uint32_t any = 0;
    for (int i = 0; i < 8; i++) any |= coeff.w[i];
    if (!any) return jac_inf<fp2>();                  // a flagged member: nothing to multiply
    return jac_mul_256_w4_body(sig(t), coeff.w);
}

// A group's end: len members, `flags` as its members' lanes left them, p = the sum of its products (not read when len == 0).  Status by
// precedence: AGG_BAD_INDEX, AGG_EMPTY ("invalid inputs"), REC_ZERO_ID and REC_DUP_ID (len >= 2 only; the reference tests zero first),
// AGG_INFINITY, AGG_OK.  Any status but AGG_OK: the encodings of infinity (for AGG_INFINITY they are the point's valid encodings).
BLS_HD aggsigs_end recover_finish_item(uint32_t len, uint32_t flags, const g2_jac& p) {
    const uint8_t refuse = (flags & REC_F_BAD_INDEX)                 ? AGG_BAD_INDEX
                           : len == 0                                ? AGG_EMPTY
                           : (len >= 2 && (flags & REC_F_ZERO_ID))   ? REC_ZERO_ID
                           : (len >= 2 && (flags & REC_F_DUP_ID))    ? REC_DUP_ID
                                                                     : AGG_OK;
    aggsigs_end e = aggsigs_finish_item(refuse != AGG_OK, false, p);
    if (refuse != AGG_OK) e.status = refuse;
    return e;
}

}  // namespace bls
