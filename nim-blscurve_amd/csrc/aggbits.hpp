// Key aggregation by participation bits (mi355_bls_aggregate_sets_bits): aggregateAll (blst_min_pubkey_sig_core.nim:179-195) over the
// committee keys whose bit is 1, or - when the committee's own aggregate is known and more than half of it signed - subtractAll
// (blst_min_pubkey_sig_core.nim:197-209) of the keys whose bit is 0 from that aggregate; the step in front of fastAggregateVerify's pairing
// (bls_sig_min_pubkey.nim:234-258).  The bodies of ONE item over the tables of plan.hpp aggbits_measure / aggbits_fill, written like
// aggsets.hpp so that one lane can carry an item and the host can run it.
//   mode         a set's field -> its route (sum the participants | subtract the absentees from the base) and whether no bit is set
//   level 0      up to AGGB_P positions of one set: the keys its bits select (the complement on the exclusion route) -> one Jacobian partial
//   level >= 1   aggsets.hpp aggsets_ln_item, unchanged
//   finish       direct: aggsets_finish_item.  Exclusion: base - partial by the complete addition (no absentee: the base itself; base ==
//                sum: infinity, status 2; base == -sum: the doubling branch), then the same conversion and status.
// The output is an affine image, so a record does not tell by which route its key was reached.
#pragma once
#include "aggsets.hpp"

namespace bls {

constexpr uint8_t AGGB_EXCLUDE = 1, AGGB_EMPTY = 2;      // a set's mode byte

// bit `i` of a field, i < 32 and inside the field's ceil(len / 8) bytes: the bytes [0, ceil(count / 8)) as one little-endian word
BLS_HD uint32_t aggbits_word(const uint8_t* bytes, uint32_t count) {
    uint32_t w = 0;
    for (uint32_t b = 0; 8 * b < count; b++) w |= (uint32_t)bytes[b] << (8 * b);
    return w;
}

// field: the set's ceil(len / 8) bytes (bits at positions >= len are ignored); base_zero: no aggregate was given for the committee, or its
// 96-byte image is all zero.  The exclusion route iff a base is there and 2 * popcount > len.
BLS_HD uint8_t aggbits_mode_item(const uint8_t* field, uint32_t len, bool base_zero) {
    uint32_t pop = 0;
#pragma clang loop unroll(disable)
    for (uint32_t at = 0; at < len; at += 8) {
        const uint32_t left = len - at, byte = field[at / 8] & (left < 8 ? (1u << left) - 1 : 0xffu);
        pop += (uint32_t)__builtin_popcount(byte);
    }
    return (uint8_t)((!base_zero && 2 * (uint64_t)pop > len ? AGGB_EXCLUDE : 0) | (pop == 0 ? AGGB_EMPTY : 0));
}

// positions [first, first + count) of the key sequence, count <= 32, of which `bytes` (the item's own bytes of the field) select the ones
// to add - or, exclude set, the ones NOT selected.  The walk is over the selected positions only, so a lane's time is its number of
// selected keys.  idx and the bounds check as in aggsets_l0_item: an index not below n_table is never loaded and bad() is told.
template <class LoadKey, class Bad>
BLS_HD g1_jac aggbits_l0_item(uint32_t first, uint32_t count, const uint8_t* bytes, bool exclude, const uint32_t* idx, size_t n_table, LoadKey&& key,
                              Bad&& bad) {
    uint32_t sel = aggbits_word(bytes, count);
    if (exclude) sel = ~sel;
    if (count < 32) sel &= (1u << count) - 1;
    g1_jac acc = jac_inf<fp>();
#pragma clang loop unroll(disable)
    while (sel) {
        const uint32_t j = (uint32_t)__builtin_ctz(sel);
        sel &= sel - 1;
        const size_t at = (size_t)first + j, t = idx ? (size_t)idx[at] : at;
        if (t >= n_table) {
            bad();
            continue;
        }
        acc = jac_add_aff(acc, key(t));
    }
    return acc;
}

// A set's end.  mode: aggbits_mode_item's byte; p: the set's last partial (not read for a committee of length 0: has_partial false);
// base: the committee's aggregate, read on the exclusion route only.
template <class LoadBase>
BLS_HD aggsets_end aggbits_finish_item(uint8_t mode, bool has_partial, bool bad, const g1_jac& p, LoadBase&& base) {
    if (!(mode & AGGB_EXCLUDE) || !has_partial) return aggsets_finish_item((mode & AGGB_EMPTY) != 0 || !has_partial, bad, p);
    return aggsets_finish_item(false, bad, jac_add_aff(jac_neg(p), base()));
}

}  // namespace bls
