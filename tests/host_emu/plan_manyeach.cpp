// The per-batch plan of csrc/plan.hpp (manyeach_cut, manyeach_as_groups, manyeach_sum_offsets over aggveach_groups / aggveach_measure /
// aggveach_fill and aggsets_measure / aggsets_fill) as a host library for ctypes - tests/test_manyeach_plan.py.
#include <vector>
#include "plan.hpp"
using namespace plan;

extern "C" {
int manyeach_plan_fits_alone(size_t n, size_t cap_sets, size_t cap_pairs) { return manyeach_fits_alone(n, cap_sets, cap_pairs); }
int manyeach_plan_pkmul_spread(uint32_t slots, int coop, uint32_t n) { return pkmul_spread_for(slots, coop != 0, n); }
// Walks the whole call as the host layer does.  Every array may be null (a first call for the counts).  Per slice, 9 size_t: b0, b1, set0,
// sets, nb, single, line-product items, G2-sum items, G2-sum levels.  The tables of the slices that are not `single` follow each other: groups
// (4 words each), line-product items (4 words each), G2-sum items (4 words each), final_of (a word per group).
// out[4]: slices, groups, line-product items, G2-sum items.
void manyeach_plan_walk(const size_t* counts, size_t k, size_t cap_sets, size_t cap_pairs, size_t* slices, uint32_t* groups, uint32_t* items, uint32_t* sum_items,
                        uint32_t* final_of, size_t out[4]) {
    std::vector<size_t> offs(k + 1, 0), rel;
    for (size_t b = 0; b < k; b++) offs[b + 1] = offs[b] + counts[b];
    size_t ns = 0, ngr = 0, nit = 0, nsum = 0;
    for (size_t b = 0; b < k;) {
        const manyeach_slice s = manyeach_cut(counts, k, b, offs[b], cap_sets, cap_pairs);
        if (s.b1 == b) break;                        // (never: a slice takes a batch at least)
        b = s.b1;
        size_t n_items = 0, n_sum = 0, sum_levels = 0;
        if (s.nb && !s.single) {
            std::vector<aggv_group> gr(s.nb);
            aggveach_groups(offs.data(), manyeach_as_groups(s), gr.data());
            const aggveach_tab t = aggveach_measure(gr.data(), s.nb);
            rel.resize((size_t)s.nb + 1);
            manyeach_sum_offsets(gr.data(), s.nb, rel.data());
            const aggsets_plan p = aggsets_measure(rel.data(), s.nb);
            n_items = t.items, n_sum = p.items, sum_levels = p.levels;
            if (groups)
                for (uint32_t i = 0; i < s.nb; i++) {
                    uint32_t* o = groups + (ngr + i) * 4;
                    o[0] = gr[i].g, o[1] = gr[i].first, o[2] = gr[i].count, o[3] = gr[i].flags;
                }
            if (items) aggveach_fill(t, gr.data(), s.nb, reinterpret_cast<agg_item*>(items + nit * 4));
            if (sum_items && final_of) aggsets_fill(p, rel.data(), s.nb, reinterpret_cast<agg_item*>(sum_items + nsum * 4), final_of + ngr);
            ngr += s.nb, nit += n_items, nsum += n_sum;
        }
        if (slices) {
            size_t* o = slices + ns * 9;
            o[0] = s.b0, o[1] = s.b1, o[2] = s.set0, o[3] = s.sets, o[4] = s.nb, o[5] = s.single, o[6] = n_items, o[7] = n_sum, o[8] = sum_levels;
        }
        ns++;
    }
    out[0] = ns, out[1] = ngr, out[2] = nit, out[3] = nsum;
}
}
