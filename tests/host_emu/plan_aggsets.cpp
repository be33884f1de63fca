// The per-set key aggregation plan of csrc/plan.hpp (aggsets_measure, aggsets_fill) as a host library for ctypes - tests/test_aggsets_plan.py.
#include "plan.hpp"
using namespace plan;

extern "C" {
uint32_t aggsets_plan_c(void) { return AGG_C; }
uint32_t aggsets_plan_none(void) { return AGG_NONE; }
// -> 1 and levels, level_first[0 .. levels], items (= the partials the buffer must hold) | 0: the plan refuses the offsets
int aggsets_plan_measure(const size_t* offsets, size_t k, uint32_t* levels, size_t level_first[AGG_MAX_LEVELS + 1], size_t* items) {
    const aggsets_plan p = aggsets_measure(offsets, k);
    if (!p.ok) return 0;
    *levels = p.levels, *items = p.items;
    for (uint32_t l = 0; l <= AGG_MAX_LEVELS; l++) level_first[l] = l <= p.levels ? p.level_first[l] : p.items;
    return 1;
}
// items: 4 words each (src_first, count, dst, seg), final_of: k words
int aggsets_plan_fill(const size_t* offsets, size_t k, uint32_t* items, uint32_t* final_of) {
    const aggsets_plan p = aggsets_measure(offsets, k);
    if (!p.ok) return 0;
    aggsets_fill(p, offsets, k, reinterpret_cast<agg_item*>(items), final_of);
    return 1;
}
}
