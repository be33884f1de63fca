// aggregateVerify (bls_sig_min_pubkey.nim:127-199 -> ContextCoreAggregateVerify, blst_min_pubkey_sig_core.nim:305-414) for MANY groups at once:
// the bodies one lane carries for one group, written so that the host can run them.
//   V_g,s   = L_s(-G1, sig_g) * prod_j L_s(pk_gj, H(m_gj))      the step values, s = 0 .. 67
//   f_g     = conj( Horner_s (f^2 [at doubling steps] * V_g,s) )
//   value_g = final_exp(f_g)                                     pairing.hpp's final_exp: the same fixed exponent as every other path
//   verdict = value_g == 1 and the group has a pair and no key of it is the point at infinity or out of the table
// The lines come from the line store the batch path fills: a pair with an operand at infinity has line_one() lines there, so an infinity
// signature contributes e(-G1, inf) = 1 and an infinity key 1 for its pair - the verdict of its group is forced to 0 as update() does.
// The products of a step are formed in levels of items (plan.hpp aggveach_fill): level 0 multiplies lines, higher levels partials; a group
// longer than a slice of the pair store is walked in parts whose Miller values (Horner done, no final exponentiation) are multiplied together.
#pragma once
#include "pairing.hpp"

namespace bls {

// Level 0: the product of the lines of pairs first .. first + count - 1 of the slice at one step (count >= 1) and, with_sig, of the line of
// pair sig_slot.  The first two meet sparse times sparse (fp12_from_line, then fp12_mul_by_line), every further one is a sparse product into
// the Fp12.  Operands: lines as the line kernels store them (limbs within one unit, |v| < 2p).  Result: canonical limbs, |v| < 2p per
// coefficient - what fp12_mul_by_line returns and takes, and what fp12_mul takes: a partial is stored as it is.  A step value owes an
// fp12_reduce (the caller's, once per group and step): the Fp12 engine takes |v| < 0.51p.
template <class Line>
BLS_HD fp12 aggveach_l0_item(uint32_t first, uint32_t count, bool with_sig, uint32_t sig_slot, Line&& line) {
    fp12 acc = fp12_from_line(line(first));
#pragma clang loop unroll(disable)
    for (uint32_t j = 1; j < count; j++) acc = fp12_mul_by_line(acc, line(first + j));
    if (with_sig) acc = fp12_mul_by_line(acc, line(sig_slot));
    return acc;
}
// A higher level: the product of partials first .. first + count - 1 (count >= 1).  Operands |v| < 2p (level 0's) or reduced (a level
// above); the result of fp12_mul is reduced (|v| < 0.51p), a lone operand is handed on as it is.
template <class Part>
BLS_HD fp12 aggveach_ln_item(uint32_t first, uint32_t count, Part&& part) {
    fp12 acc = part(first);
#pragma clang loop unroll(disable)
    for (uint32_t j = 1; j < count; j++) acc = fp12_mul(acc, part(first + j));
    return acc;
}
// f = conj( Horner_s (f^2 [at doubling steps] * V_s) ) over a group's 68 dense step values (reduced, as the step store holds them).
// Result reduced but for the conjugation's negations (what final_exp and fp12_mul take: vereach_miller returns the same).
template <class Src>
BLS_HD fp12 aggveach_horner(Src&& v) {
    fp12 f = fp12_one();
    int bit = 62;
    bool add = false;                                   // step s is the addition step behind a set bit of |x| (no squaring in front of it)
#pragma clang loop unroll(disable)
    for (int s = 0; s < N_LINES; s++) {
        if (!add) f = fp12_sqr(f);
        f = fp12_mul(f, v(s));
        if (!add && ((k::X_ABS >> bit) & 1)) {
            add = true;
        } else {
            add = false;
            bit--;
        }
    }
    return fp12_conj(f);
}
// the Miller value of a part times the value carried from the parts before it (canonical: it comes from a blst_fp12 image); reduced
BLS_HD fp12 aggveach_carry(const fp12& f, const fp12& carry) { return fp12_mul(f, carry); }

struct aggveach_out {
    fp12 value;        // final_exp(f): canonical after fp12_store_le / the blst image store
    bool ok;
};
// bad: a key of the group is the point at infinity or its index is out of range
BLS_HD aggveach_out aggveach_verdict(const fp12& f, bool bad) {
    const fp12 v = final_exp(f);
    const bool one = fp12_is_one(v);
    return aggveach_out{v, one && !bad};
}

}  // namespace bls
