// batchVerify by message (mi355_bls_batch_verify_by_message): the sets of a batch that share a 32-byte message are found on the device, so
// that hashing and the Miller loop run once per DISTINCT message - the bodies one lane carries, written so that the host can run them.
//   insert       set i into an open-addressing table of set indices (a power of two of at least 2 n slots); a slot's key is the message of
//                the index it holds, and the slot ends up holding the SMALLEST index with that message: the group's representative
//   flag / rank  a set is a representative iff its slot holds its own index; a group's number is the rank of its representative among the
//                representatives (an exclusive scan of the flags), which is the order in which the messages first appear in the input
//   count        members per group; offsets = their exclusive scan; scatter: the members of group g at [offsets[g], offsets[g + 1]), any order
//   sum item     up to AGG_C of k_pkmul's products, addressed through the member list (level 0 of plan.hpp aggsets_fill's tables; the levels
//                above are aggsets_ln_item's)
// Equality is ALWAYS decided on all 32 bytes; the hash only picks where the probe starts.  What makes a memory access atomic is the
// caller's business (the kernels use vector atomics, the CPU tests plain code): it hands in cas / min / add.
#pragma once
#include "aggsets.hpp"

namespace bls {

constexpr uint32_t BYMSG_EMPTY = 0xffffffffu;      // a free slot (no set has this index: n < 2^32 - 1)

// (the table's size is plan.hpp bymsg_table_slots)
// where a message's probe starts: every one of the eight words goes through a multiply-xorshift round, so messages that differ in one byte
// anywhere start at unrelated slots
BLS_HD uint32_t bymsg_hash(const uint32_t* m) {
    uint32_t h = 0x9e3779b9u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h = (h ^ m[i]) * 0x85ebca6bu;
        h ^= h >> 15;
        h *= 0xc2b2ae35u;
        h ^= h >> 13;
    }
    return h;
}
BLS_HD bool bymsg_equal(const uint32_t* a, const uint32_t* b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
    return d == 0;
}
// Set i -> the slot of its group.  msg(j): the eight message words of set j; cas(slot, expect, val) -> the slot's old value, val stored iff
// it was `expect`; amin(slot, val): slot <- min(slot, val).  A claimed slot never changes its KEY: whatever amin installs carries the same
// message, so the comparison against any index read from it stays valid.  Terminates: n sets fill at most half of the slots.
template <class Msg, class Cas, class Min>
BLS_HD uint32_t bymsg_insert(uint32_t i, uint32_t slots, Msg&& msg, Cas&& cas, Min&& amin) {
    const uint32_t* mine = msg(i);
    uint32_t h = bymsg_hash(mine) & (slots - 1);
    for (;;) {
        const uint32_t was = cas(h, BYMSG_EMPTY, i);
        if (was == BYMSG_EMPTY) return h;                  // claimed: i is the first of its message here
        if (bymsg_equal(mine, msg(was))) {
            amin(h, i);
            return h;
        }
        h = (h + 1) & (slots - 1);
    }
}
// One lane's part of an exclusive scan of in[0 .. n) over `lanes` lanes (the k_msm_scan shape): lane l owns in[l per .. (l + 1) per).
BLS_HD uint32_t bymsg_scan_per(uint32_t n, uint32_t lanes) { return (n + lanes - 1) / lanes; }
BLS_HD uint32_t bymsg_scan_sum(const uint32_t* in, uint32_t n, uint32_t per, uint32_t lane) {
    const uint64_t lo = (uint64_t)lane * per, hi = lo + per < n ? lo + per : n;
    uint32_t s = 0;
    for (uint64_t j = lo; j < hi; j++) s += in[j];
    return s;
}
// `run` = the sum of everything in front of the lane's part (the caller's cross-lane prefix; it also writes out[n] = the total)
BLS_HD void bymsg_scan_write(const uint32_t* in, uint32_t n, uint32_t per, uint32_t lane, uint32_t run, uint32_t* out) {
    const uint64_t lo = (uint64_t)lane * per, hi = lo + per < n ? lo + per : n;
    for (uint64_t j = lo; j < hi; j++) {
        out[j] = run;
        run += in[j];
    }
}
// level 0 of the group sums: members [first, first + count) of the member list, count >= 1; pt(j): the product [r_j]PK_j of SET j
template <class LoadPt>
BLS_HD g1_jac bymsg_l0_item(uint32_t first, uint32_t count, const uint32_t* members, LoadPt&& pt) {
    return aggsets_ln_item(first, count, [&](uint32_t pos) { return pt(members[pos]); });
}
// A group's end: its sum as the P of its Miller pair.  An infinite sum is stored as THE infinity image (Z = 0 in every limb): the line
// kernels test exactly that and give the pair the value 1.
BLS_HD g1_jac bymsg_finish_item(const g1_jac& sum, bool* infinite) {
    *infinite = jac_is_inf(sum);
    return *infinite ? jac_inf<fp>() : sum;
}

}  // namespace bls
