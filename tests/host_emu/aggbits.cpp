// CPU execution of the key aggregation by participation bits (csrc/aggbits.hpp item bodies over the tables of csrc/plan.hpp aggbits_fill) for
// tests/test_aggbits_emu.py, bounds tracked like tests/host_emu/emu.hip.  TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "aggbits.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// what mi355_bls_aggregate_sets_bits computes, kernel by kernel and item by item: keys n_table x 96 B, idx nullable, c_offsets m + 1, aggs
// nullable (m images agg_stride bytes apart), which k, bits packed, msgs k x 32 B, sigs k x 192 B -> records k x 320 B, status k bytes,
// routes[2] = sets summed directly / by exclusion.  1: every status 0 | 0 | -3: the arguments are refused
int emu_aggregate_sets_bits(const uint8_t* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m, const uint8_t* aggs, size_t agg_stride,
                            const uint32_t* which, const uint8_t* bits, size_t k, const uint8_t* msgs, const uint8_t* sigs, uint8_t* records, uint8_t* status,
                            uint32_t routes[2]) {
    if (aggs && (agg_stride < 96 || agg_stride % 4)) return -3;
    const plan::aggbits_plan p = plan::aggbits_measure(c_offsets, m, which, k);
    if (!p.ok || (!idx && m && c_offsets[m] > n_table)) return -3;
    std::vector<plan::agg_item> items(p.items);
    std::vector<plan::aggb_set> sets(k);
    plan::aggbits_fill(p, c_offsets, which, k, items.data(), sets.data());
    std::vector<uint8_t> mode(k), bad(k, 0);
    routes[0] = routes[1] = 0;
    for (size_t s = 0; s < k; s++) {
        bool zero = true;
        if (aggs)
            for (int i = 0; i < 96; i++) zero &= aggs[sets[s].committee * agg_stride + i] == 0;
        mode[s] = aggbits_mode_item(bits + sets[s].bits_first, sets[s].len, zero);
        routes[mode[s] & AGGB_EXCLUDE]++;
    }
    std::vector<g1_jac> part(p.items);
    for (uint32_t l = 0; l < p.levels; l++)
        for (size_t i = p.level_first[l]; i < p.level_first[l + 1]; i++) {
            const plan::agg_item& it = items[i];
            if (l == 0)
                part[i] = aggbits_l0_item(it.src_first, it.count, bits + it.dst, (mode[it.seg] & AGGB_EXCLUDE) != 0, idx, n_table,
                                          [&](size_t t) { return g1_aff_load(keys + t * 96); }, [&]() { bad[it.seg] = 1; });
            else
                part[it.dst] = aggsets_ln_item(it.src_first, it.count, [&](uint32_t j) { return part[j]; });
        }
    int all = 1;
    for (size_t s = 0; s < k; s++) {
        const bool has = sets[s].final_of != plan::AGG_NONE;
        const aggsets_end e = aggbits_finish_item(mode[s], has, bad[s] != 0, has ? part[sets[s].final_of] : jac_inf<fp>(),
                                                  [&]() { return g1_aff_load(aggs + sets[s].committee * agg_stride); });
        std::memcpy(records + s * 320, e.pk, 96);
        std::memcpy(records + s * 320 + 96, msgs + s * 32, 32);
        std::memcpy(records + s * 320 + 128, sigs + s * 192, 192);
        status[s] = e.status;
        all &= e.status == AGG_OK;
    }
    return all;
}
}
