// The per-group aggregateVerify plan of csrc/plan.hpp (aggveach_cut, aggveach_groups, aggveach_measure, aggveach_fill, aggveach_for) as a
// host library for ctypes - tests/test_aggveach_plan.py.
#include <vector>
#include "plan.hpp"
using namespace plan;

extern "C" {
uint32_t aggveach_plan_c(void) { return AGGV_C; }
uint32_t aggveach_plan_max_levels(void) { return AGGV_MAX_LEVELS; }
void aggveach_plan_flags(uint32_t out[5]) { out[0] = AGGV_FINAL, out[1] = AGGV_SIG, out[2] = AGGV_COUNT, out[3] = AGGV_OPEN_IN, out[4] = AGGV_OPEN_OUT; }
// Walks the whole call as the host layer does.  Every array may be null (a first call for the counts).  Per slice, 10 size_t:
// g0, g1, pos0, pos1, ng, open_in, open_out, levels, items, partials, then AGGV_MAX_LEVELS + 1 of level_first; the slices' groups and items
// (4 words each) follow each other in `groups` and `items`.  counts: slices, groups, items.
void aggveach_plan_walk(const size_t* offsets, size_t k, size_t cap, uint32_t C, size_t* slices, uint32_t* groups, uint32_t* items, size_t counts[3]) {
    const size_t W = 10 + AGGV_MAX_LEVELS + 1;
    size_t ns = 0, ngr = 0, nit = 0, g = 0, pos = k ? offsets[0] : 0;
    for (;;) {
        const aggv_slice s = aggveach_cut(offsets, k, g, pos, cap);
        if (s.pairs() == 0) break;
        std::vector<aggv_group> gr(s.ng);
        aggveach_groups(offsets, s, gr.data());
        const aggveach_tab t = aggveach_measure(gr.data(), s.ng, C);
        if (slices) {
            size_t* o = slices + ns * W;
            o[0] = s.g0, o[1] = s.g1, o[2] = s.pos0, o[3] = s.pos1, o[4] = s.ng, o[5] = s.open_in, o[6] = s.open_out;
            o[7] = t.levels, o[8] = t.items, o[9] = t.partials;
            for (uint32_t l = 0; l <= AGGV_MAX_LEVELS; l++) o[10 + l] = l <= t.levels ? t.level_first[l] : t.items;
        }
        if (groups)
            for (uint32_t i = 0; i < s.ng; i++) {
                uint32_t* o = groups + (ngr + i) * 4;
                o[0] = gr[i].g, o[1] = gr[i].first, o[2] = gr[i].count, o[3] = gr[i].flags;
            }
        if (items) aggveach_fill(t, gr.data(), s.ng, reinterpret_cast<agg_item*>(items + nit * 4), C);
        ns++, ngr += s.ng, nit += t.items;
        g = s.next_g(), pos = s.pos1;
    }
    counts[0] = ns, counts[1] = ngr, counts[2] = nit;
}
// a slice's launch shapes: setup_grid, lines.main_pairs, lines.main.team, tail_engine, tail_grid
void aggveach_plan_for(uint32_t slots, int coop, uint32_t pairs, uint32_t sigs, uint32_t ng, uint32_t out[5]) {
    const aggveach_plan p = aggveach_for(slots, coop != 0, pairs, sigs, ng);
    out[0] = p.setup_grid, out[1] = p.lines.main_pairs, out[2] = p.lines.main.team, out[3] = p.tail_engine, out[4] = p.tail_grid;
}
uint32_t aggveach_plan_engine_max(uint32_t slots) { return each_engine_max(slots); }
size_t aggveach_plan_part_words(size_t partials) { return aggveach_part_words(partials); }
size_t aggveach_plan_step_words(size_t ng) { return aggveach_step_words(ng); }
}
