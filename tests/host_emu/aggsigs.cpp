// CPU execution of the per-group signature aggregation (csrc/aggsigs.hpp item bodies and combsets.hpp's G2 sum item over the tables of
// csrc/plan.hpp aggsets_fill), of the signature compression and of the signature-only decoder, for tests/test_aggsigs_emu.py, bounds tracked
// like tests/host_emu/emu.hip; and the workspace sizes of csrc/plan.hpp aggsigs_sizes_for for tests/test_aggsigs_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "aggsigs.hpp"
#include "combsets.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// what mi355_bls_aggregate_signature_sets computes, level by level and item by item as the kernels walk them: sigs n_table x 192 B, idx
// nullable, offsets k + 1 -> out192 k x 192 B, out96 k x 96 B (either nullable), status k bytes.
// 1: every status 0 | 0 | -3: the plan refuses the offsets
int emu_aggregate_signature_sets(const uint8_t* sigs, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, uint8_t* out192, uint8_t* out96,
                                 uint8_t* status) {
    const plan::aggsets_plan p = plan::aggsets_measure(offsets, k);
    if (!p.ok || (!idx && k && offsets[k] > n_table)) return -3;
    std::vector<plan::agg_item> items(p.items);
    std::vector<uint32_t> final_of(k);
    plan::aggsets_fill(p, offsets, k, items.data(), final_of.data());
    std::vector<g2_jac> part(plan::aggsigs_sizes_for(p, k).part / (plan::G2_WORDS * 4));
    std::vector<uint8_t> bad(k, 0);
    for (uint32_t l = 0; l < p.levels; l++)
        for (size_t i = p.level_first[l]; i < p.level_first[l + 1]; i++) {
            const plan::agg_item& it = items[i];
            part.at(it.dst) = l == 0 ? aggsigs_l0_item(it.src_first, it.count, idx, n_table, [&](size_t t) { return g2_aff_load(sigs + t * 192); }, [&]() { bad[it.seg] = 1; })
                                     : combsets_sum_item<fp2>(it.src_first, it.count, [&](uint32_t j) { return part.at(j); });
        }
    int all = 1;
    for (size_t g = 0; g < k; g++) {
        const bool empty = final_of[g] == plan::AGG_NONE;
        const aggsigs_end e = aggsigs_finish_item(empty, bad[g] != 0, empty ? jac_inf<fp2>() : part.at(final_of[g]));
        if (out192) std::memcpy(out192 + g * 192, e.sig, 192);
        if (out96) std::memcpy(out96 + g * 96, e.wire, 96);
        status[g] = e.status;
        all &= e.status == AGG_OK;
    }
    return all;
}
// mi355_bls_compress_signatures: n x 192 B images -> n x 96 B, by the words a lane writes and by the byte form
int emu_compress_signatures(const uint8_t* sigs, size_t n, uint8_t* out96) {
    for (size_t i = 0; i < n; i++) {
        const g2_aff a = g2_aff_load(sigs + i * 192);
        uint32_t wire[24];
        uint8_t b[96];
        aggsigs_compress_item(wire, a);
        g2_compress(b, a);
        if (std::memcmp(wire, b, 96) != 0) return -1;
        std::memcpy(out96 + i * 96, wire, 96);
    }
    return 0;
}
// mi355_bls_deserialize_signatures: deser.hpp deserialize_signature per signature; images zeroed where the status is not 0.  1: every status 0
int emu_deserialize_signatures(const uint8_t* sigs, size_t n, uint32_t flags, uint8_t* out192, uint8_t* status) {
    int all = 1;
    for (size_t i = 0; i < n; i++) {
        g2_aff sg;
        status[i] = deserialize_signature(sg, sigs + i * ((flags & DESER_F_SIG_UNCOMPRESSED) ? 192 : 96), flags);
        all &= status[i] == DESER_OK;
        if (status[i] != DESER_OK) sg = g2_aff{fp2_zero(), fp2_zero()};
        fp2_store_le(out192 + i * 192, sg.x);
        fp2_store_le(out192 + i * 192 + 96, sg.y);
    }
    return all;
}
// plan.hpp aggsigs_sizes_for beside aggsets_measure's numbers: -> 1 and sizes[6] = part, tab, bad, status, out192, out96 (bytes), items | 0
int aggsigs_plan_sizes(const size_t* offsets, size_t k, size_t sizes[6], size_t* items) {
    const plan::aggsets_plan p = plan::aggsets_measure(offsets, k);
    if (!p.ok) return 0;
    const plan::aggsigs_sizes s = plan::aggsigs_sizes_for(p, k);
    sizes[0] = s.part, sizes[1] = s.tab, sizes[2] = s.bad, sizes[3] = s.status, sizes[4] = s.out192, sizes[5] = s.out96;
    *items = p.items;
    return 1;
}
uint32_t aggsigs_plan_g2_words(void) { return plan::G2_WORDS; }
}
