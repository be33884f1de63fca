// Per-set verification (verify, bls_sig_min_pubkey.nim:108-125 -> coreVerifyNoGroupCheck, blst_min_pubkey_sig_core.nim:269-297) for MANY sets at
// once: the pairing tail of ONE set, written so that one lane can carry it and the host can run it.
//   f_i       = MillerLoop((pk_i, H(msg_i)), (-G1, sig_i))   one two-pair loop: the two lines of a step meet before they meet f, one squaring per step
//   value_i   = final_exp(f_i)                                 pairing.hpp's final_exp: the same fixed exponent 3 (p^12 - 1) / r as every other path
//   verdict_i = value_i == 1 and pk_i is not the point at infinity
// Nothing here depends on anything but the set's own two pairs: no blinding, no neighbour, no position.
// The lines come from the line store the batch path fills (k_lines / the lane-team engine): a pair with an operand at infinity has line_one()
// lines there, so an infinity signature leaves e(pk, H) alone (verdict 0 for a valid key) and an infinity key leaves e(-G1, sig) - its verdict is
// forced to 0 as BLST_PK_IS_INFINITY does.
//
// Two forms (plan.hpp each_for): small calls walk the same steps on the lane-cooperative Fp12 engine (kernels.hip each_engine_body, which forms
// the step values La_s * Lb_s with the same line product and hands them to k_tail's body); large calls run this header as it stands:
// tower arithmetic on one lane per set (tower.hpp's fp12_sqr / fp12_mul, out of line).  Per step the two sparse lines are multiplied into one
// Fp12 by the line product (fp12_mul_by_line on fp12_from_line of the first: inputs as the line store holds them, output already what fp12_mul takes), then
// f <- f^2 * that: one squaring, one sparse and one full product per doubling step.
#pragma once
#include "pairing.hpp"

namespace bls {

// f = conj( Horner_s (f^2 [at doubling steps] * La_s * Lb_s) ), lines in miller_lines step order
template <class SrcA, class SrcB>
BLS_HD fp12 vereach_miller(SrcA&& la, SrcB&& lb) {
    fp12 f = fp12_one();
    int bit = 62;
    bool add = false;                                   // step s is the addition step behind a set bit of |x| (no squaring in front of it)
#pragma clang loop unroll(disable)
    for (int s = 0; s < N_LINES; s++) {
        if (!add) f = fp12_sqr(f);
        f = fp12_mul(f, fp12_mul_by_line(fp12_from_line(la(s)), lb(s)));
        if (!add && ((k::X_ABS >> bit) & 1)) {
            add = true;
        } else {
            add = false;
            bit--;
        }
    }
    return fp12_conj(f);
}

struct vereach_out {
    fp12 value;        // final_exp(f): canonical after fp12_store_le / the blst image store
    bool ok;
};
template <class SrcA, class SrcB>
BLS_HD vereach_out vereach_set(SrcA&& la, SrcB&& lb, bool pk_inf) {
    const fp12 v = final_exp(vereach_miller(la, lb));
    const bool one = fp12_is_one(v);
    return vereach_out{v, one && !pk_inf};
}

}  // namespace bls
