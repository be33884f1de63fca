// CPU execution of the per-set key aggregation (csrc/aggsets.hpp item bodies over the tables of csrc/plan.hpp aggsets_fill) for
// tests/test_aggsets_emu.py, bounds tracked like tests/host_emu/emu.hip.  TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "aggsets.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// what mi355_bls_aggregate_sets computes, level by level and item by item as the kernels walk them: keys n_table x 96 B, idx nullable,
// offsets k + 1, msgs k x 32 B, sigs k x 192 B -> records k x 320 B, status k bytes.  1: every status 0 | 0 | -3: the plan refuses the offsets
int emu_aggregate_sets(const uint8_t* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const uint8_t* msgs, const uint8_t* sigs,
                       uint8_t* records, uint8_t* status) {
    const plan::aggsets_plan p = plan::aggsets_measure(offsets, k);
    if (!p.ok || (!idx && k && offsets[k] > n_table)) return -3;
    std::vector<plan::agg_item> items(p.items);
    std::vector<uint32_t> final_of(k);
    plan::aggsets_fill(p, offsets, k, items.data(), final_of.data());
    std::vector<g1_jac> part(p.items);
    std::vector<uint8_t> bad(k, 0);
    for (uint32_t l = 0; l < p.levels; l++)
        for (size_t i = p.level_first[l]; i < p.level_first[l + 1]; i++) {
            const plan::agg_item& it = items[i];
            part[it.dst] = l == 0 ? aggsets_l0_item(it.src_first, it.count, idx, n_table, [&](size_t t) { return g1_aff_load(keys + t * 96); }, [&]() { bad[it.seg] = 1; })
                                  : aggsets_ln_item(it.src_first, it.count, [&](uint32_t j) { return part[j]; });
        }
    int all = 1;
    for (size_t s = 0; s < k; s++) {
        const bool empty = final_of[s] == plan::AGG_NONE;
        const aggsets_end e = aggsets_finish_item(empty, bad[s] != 0, empty ? jac_inf<fp>() : part[final_of[s]]);
        std::memcpy(records + s * 320, e.pk, 96);
        std::memcpy(records + s * 320 + 96, msgs + s * 32, 32);
        std::memcpy(records + s * 320 + 128, sigs + s * 192, 192);
        status[s] = e.status;
        all &= e.status == AGG_OK;
    }
    return all;
}
}
