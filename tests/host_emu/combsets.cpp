// CPU execution of the same-message pre-aggregation (csrc/combsets.hpp bodies over the tables of csrc/plan.hpp combsets_measure /
// aggsets_fill) for tests/test_combsets_emu.py, bounds tracked like tests/host_emu/emu.hip.  TEST INFRASTRUCTURE: never linked into the
// product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "combsets.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// the scalars of a group of n members
void emu_combsets_chain(const uint8_t rnd[32], size_t n, uint64_t* out) {
    combsets_chain(rnd, n, [&](size_t j, uint64_t v) { out[j] = v; });
}
// what mi355_bls_combine_sets computes, stage by stage and item by item as the kernels walk them: sets n_sets x 320 B, idx nullable,
// offsets k + 1, rnds k x 32 B -> records k x 320 B, status k bytes.  1: every status 0 | 0 | -3: the plan refuses the offsets
int emu_combine_sets(const uint8_t* sets, size_t n_sets, const uint32_t* idx_all, const size_t* offsets, size_t k, const uint8_t* rnds, uint8_t* records,
                     uint8_t* status) {
    const plan::combsets_plan cp = plan::combsets_measure(offsets, k);
    if (!cp.ok || (!idx_all && k && offsets[k] > n_sets)) return -3;
    const size_t N = cp.members;
    std::vector<size_t> rel(k + 1);
    for (size_t g = 0; g <= k; g++) rel[g] = offsets[g] - cp.lo;
    const plan::aggsets_plan p = plan::aggsets_measure(rel.data(), k);
    if (!p.ok) return -3;
    std::vector<plan::agg_item> items(p.items);
    std::vector<uint32_t> final_of(k);
    plan::aggsets_fill(p, rel.data(), k, items.data(), final_of.data());
    const uint32_t* idx = idx_all ? idx_all + cp.lo : nullptr;
    // the records by position (k_combsets_gather: an index out of range leaves a zero record and is never dereferenced)
    std::vector<uint32_t> recs(N * 80 + 1, 0);
    for (size_t pos = 0; pos < N; pos++) {
        const size_t at = idx ? idx[pos] : cp.lo + pos;
        if (at < n_sets) std::memcpy(&recs[pos * 80], sets + at * 320, 320);
    }
    const auto bad = [&](uint32_t pos) { return idx && idx[pos] >= n_sets; };
    const auto rec = [&](uint32_t pos) { return (const uint32_t*)&recs[(size_t)pos * 80]; };
    // scalars: a lane per group (k_combsets_scalars; the host walks the same body for a long group)
    std::vector<uint64_t> s(N + 1, 0);
    for (size_t g = 0; g < k; g++) {
        const size_t len = rel[g + 1] - rel[g];
        if (len >= 2) combsets_chain(rnds + g * 32, len, [&](size_t j, uint64_t v) { s[rel[g] + j] = v; });
    }
    // per member: the two products, each with a window table of its own
    std::vector<g1_jac> m1(N);
    std::vector<g2_jac> m2(N);
    for (size_t pos = 0; pos < N; pos++) {
        const uint8_t* r = (const uint8_t*)rec((uint32_t)pos);
        g1_jac t1[8];
        g2_jac t2[8];
        m1[pos] = combsets_mul_item(g1_aff_load(r), s[pos], [&](int e, const g1_jac& t) { t1[e] = t; }, [&](int e) { return t1[e]; });
        m2[pos] = combsets_mul_item(g2_aff_load(r + 128), s[pos], [&](int e, const g2_jac& t) { t2[e] = t; }, [&](int e) { return t2[e]; });
    }
    // per group: the segmented sums and the checks of the level-0 items
    std::vector<g1_jac> part1(p.items);
    std::vector<g2_jac> part2(p.items);
    std::vector<uint32_t> flags(k, 0);
    for (uint32_t l = 0; l < p.levels; l++)
        for (size_t i = p.level_first[l]; i < p.level_first[l + 1]; i++) {
            const plan::agg_item& it = items[i];
            if (l == 0) {
                flags[it.seg] |= combsets_check_item(it.src_first, it.count, (uint32_t)rel[it.seg], bad, rec);
                part1[it.dst] = aggsets_ln_item(it.src_first, it.count, [&](uint32_t j) { return m1[j]; });
                part2[it.dst] = combsets_sum_item<fp2>(it.src_first, it.count, [&](uint32_t j) { return m2[j]; });
            } else {
                part1[it.dst] = aggsets_ln_item(it.src_first, it.count, [&](uint32_t j) { return part1[j]; });
                part2[it.dst] = combsets_sum_item<fp2>(it.src_first, it.count, [&](uint32_t j) { return part2[j]; });
            }
        }
    int all = 1;
    for (size_t g = 0; g < k; g++) {
        const uint32_t len = (uint32_t)(rel[g + 1] - rel[g]), first = (uint32_t)rel[g];
        const bool sums = len >= 2 && final_of[g] != plan::AGG_NONE, have_first = len >= 1 && !bad(first);
        const combsets_end e = combsets_finish_item(len, flags[g], sums ? part1[final_of[g]] : jac_inf<fp>(), sums ? part2[final_of[g]] : jac_inf<fp2>(),
                                                    have_first ? rec(first) : nullptr);
        std::memcpy(records + g * 320, e.rec, 320);
        status[g] = e.status;
        all &= e.status == AGG_OK;
    }
    return all;
}
}
