// CPU execution of the device grouping of batchVerify by message (csrc/bymsg.hpp bodies, walked kernel by kernel as host_api.inc
// run_pairs_grouped launches them) for tests/test_bymsg_emu.py.  TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "bymsg.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
unsigned emu_bymsg_table_slots(size_t n) { return plan::bymsg_table_slots(n); }
unsigned emu_bymsg_hash(const uint32_t msg[8]) { return bymsg_hash(msg); }
// sets: n x 320 B (4-byte aligned).  order: the order in which the "lanes" insert and scatter (a permutation of 0 .. n-1, or NULL for input
// order): the result must not depend on it, but for the order of members inside a group.
// -> slot_of[n], rep[n], gid[n], offsets[n + 1] (k + 1 written), members[n], reps[n] (k written); returns k, or -1 if an index left its array
int emu_bymsg_group(const uint8_t* sets, size_t n, const uint32_t* order, uint32_t* slot_of, uint32_t* rep, uint32_t* gid, uint32_t* offsets, uint32_t* members,
                    uint32_t* reps) {
    const uint32_t n32 = (uint32_t)n, slots = plan::bymsg_table_slots(n), lanes = 64;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(sets);
    std::vector<uint32_t> table(slots, BYMSG_EMPTY), flag(n), rank(n + 1), counts(n + 1, 0), cursor(n + 1, 0);
    bool oob = false;
    // k_bymsg_insert
    for (uint32_t t = 0; t < n32; t++) {
        const uint32_t i = order ? order[t] : t;
        slot_of[i] = bymsg_insert(i, slots, [&](uint32_t j) { oob |= j >= n32; return w + (size_t)(j < n32 ? j : 0) * 80 + 24; },
                                  [&](uint32_t h, uint32_t expect, uint32_t val) {
                                      oob |= h >= slots;
                                      const uint32_t was = table[h];
                                      if (was == expect) table[h] = val;
                                      return was;
                                  },
                                  [&](uint32_t h, uint32_t val) { if (val < table[h]) table[h] = val; });
    }
    // k_bymsg_flag
    for (uint32_t i = 0; i < n32; i++) {
        oob |= slot_of[i] >= slots;
        rep[i] = table[slot_of[i]];
        flag[i] = rep[i] == i;
        oob |= rep[i] >= n32;
    }
    if (oob) return -1;
    // k_bymsg_scan: the lanes' sums, the cross-lane prefix, the lanes' writes
    const auto scan = [&](const uint32_t* in, uint32_t m, uint32_t* out) {
        const uint32_t per = bymsg_scan_per(m, lanes);
        uint32_t run = 0;
        for (uint32_t l = 0; l < lanes; l++) {
            const uint32_t s = bymsg_scan_sum(in, m, per, l);
            bymsg_scan_write(in, m, per, l, run, out);
            run += s;
        }
        out[m] = run;
    };
    scan(flag.data(), n32, rank.data());
    const uint32_t k = rank[n];
    // k_bymsg_group
    for (uint32_t i = 0; i < n32; i++) {
        oob |= rep[i] >= n32;
        const uint32_t g = rank[rep[i]];
        oob |= g >= k;
        gid[i] = g;
        counts[g]++;
        if (flag[i]) reps[g] = i;
    }
    scan(counts.data(), k, offsets);
    // k_bymsg_scatter
    for (uint32_t t = 0; t < n32; t++) {
        const uint32_t i = order ? order[t] : t, g = gid[i], at = offsets[g] + cursor[g]++;
        oob |= at >= n32;
        if (at < n32) members[at] = i;
    }
    return oob ? -1 : (int)k;
}
}
