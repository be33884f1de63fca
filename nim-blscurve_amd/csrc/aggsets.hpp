// Per-set key aggregation (mi355_bls_aggregate_sets): aggregateAll (blst_min_pubkey_sig_core.nim:179-195) for MANY key lists at once, the step
// in front of fastAggregateVerify's pairing (bls_sig_min_pubkey.nim:234-258) - the bodies of ONE item of the segmented sum that plan.hpp
// aggsets_measure / aggsets_fill lays out, written so that one lane can carry an item and the host can run it.
//   level 0      up to AGG_C keys of one segment (blst_p1_affine images, through an optional index array into a key table) -> one Jacobian partial
//   level >= 1   up to AGG_C partials of one segment -> one partial
//   finish       a segment's last partial -> its affine key and its status byte
// Both additions are the complete ones of curve.hpp (infinity operands, P = Q, P = -Q), so a segment may hold a key twice, a key and its
// negative, or the affine infinity image (all zero: adds nothing, as in mi355_bls_g1_aggregate).  Where the keys and partials live is the
// caller's business: it hands in loaders.
#pragma once
#include "curve.hpp"

namespace bls {

constexpr uint8_t AGG_OK = 0, AGG_EMPTY = 1, AGG_INFINITY = 2, AGG_BAD_INDEX = 3;      // a segment's status byte

// keys [first, first + count) of the call's key sequence; idx == nullptr: the sequence is the table itself.  A position whose table index is
// not below n_table is never loaded: bad() is told, and the key counts as the point at infinity.
template <class LoadKey, class Bad>
BLS_HD g1_jac aggsets_l0_item(uint32_t first, uint32_t count, const uint32_t* idx, size_t n_table, LoadKey&& key, Bad&& bad) {
    g1_jac acc = jac_inf<fp>();
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < count; j++) {
        const size_t at = (size_t)first + j, t = idx ? (size_t)idx[at] : at;
        if (t >= n_table) {
            bad();
            continue;
        }
        acc = jac_add_aff(acc, key(t));
    }
    return acc;
}

// partials [first, first + count), count >= 1
template <class LoadPart>
BLS_HD g1_jac aggsets_ln_item(uint32_t first, uint32_t count, LoadPart&& part) {
    g1_jac acc = part(first);
#pragma clang loop unroll(disable)
    for (uint32_t j = 1; j < count; j++) acc = jac_add_body(acc, part(first + j));
    return acc;
}

// A segment's end: `empty` = it has no key (then p is not read), `bad` = one of its indices was out of range.  status as above, bad index
// first; pk = the 24 words of the blst_p1_affine image of the sum, all zero - the image of infinity, for which every verifier answers
// false - unless the status is AGG_OK.
struct aggsets_end {
    uint32_t pk[24];
    uint8_t status;
};
BLS_HD aggsets_end aggsets_finish_item(bool empty, bool bad, const g1_jac& p) {
    aggsets_end e;
    e.status = bad ? AGG_BAD_INDEX : empty ? AGG_EMPTY : jac_is_inf(p) ? AGG_INFINITY : AGG_OK;
    if (e.status != AGG_OK) {
        for (int i = 0; i < 24; i++) e.pk[i] = 0;
        return e;
    }
    const fp zi = fp_inv(p.z), zi2 = fp_sqr(zi);
    uint32_t x[12], y[12];
    fp_to_blst(x, fp_mul(p.x, zi2));
    fp_to_blst(y, fp_mul(p.y, fp_mul(zi2, zi)));
    for (int i = 0; i < 12; i++) e.pk[i] = x[i], e.pk[12 + i] = y[i];
    return e;
}

}  // namespace bls
