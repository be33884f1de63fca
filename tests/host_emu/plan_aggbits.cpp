// The plan of the key aggregation by participation bits of csrc/plan.hpp (aggbits_measure, aggbits_fill) as a host library for ctypes -
// tests/test_aggbits_plan.py.
#include "plan.hpp"
using namespace plan;

extern "C" {
uint32_t aggbits_plan_p(void) { return AGGB_P; }
uint32_t aggbits_plan_c(void) { return AGG_C; }
uint32_t aggbits_plan_none(void) { return AGG_NONE; }
// -> 1 and levels, level_first[0 .. levels], items, the bytes of the packed fields | 0: the plan refuses the arguments
int aggbits_plan_measure(const size_t* c_offsets, size_t m, const uint32_t* which, size_t k, uint32_t* levels, size_t level_first[AGG_MAX_LEVELS + 1], size_t* items,
                         size_t* bits_bytes) {
    const aggbits_plan p = aggbits_measure(c_offsets, m, which, k);
    if (!p.ok) return 0;
    *levels = p.levels, *items = p.items, *bits_bytes = p.bits_bytes;
    for (uint32_t l = 0; l <= AGG_MAX_LEVELS; l++) level_first[l] = l <= p.levels ? p.level_first[l] : p.items;
    return 1;
}
// items: 4 words each (src_first, count, dst | byte offset at level 0, set), sets: 4 words each (bits_first, len, committee, final_of)
int aggbits_plan_fill(const size_t* c_offsets, size_t m, const uint32_t* which, size_t k, uint32_t* items, uint32_t* sets) {
    const aggbits_plan p = aggbits_measure(c_offsets, m, which, k);
    if (!p.ok) return 0;
    aggbits_fill(p, c_offsets, which, k, reinterpret_cast<agg_item*>(items), reinterpret_cast<aggb_set*>(sets));
    return 1;
}
}
