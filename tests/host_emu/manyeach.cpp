// CPU execution of the per-batch pass of mi355_bls_batch_verify_many_each: the lane bodies of csrc/manyeach.hpp and the bodies it joins
// (csrc/combsets.hpp: the 64-bit G2 multiplication and the sum item; csrc/aggveach.hpp: the line-product levels, the Horner, the verdict) over
// the plan's own slices and tables (csrc/plan.hpp manyeach_cut, aggveach_*, aggsets_*) for tests/test_manyeach_emu.py, bounds tracked like
// tests/host_emu/emu.hip.  TEST INFRASTRUCTURE: never linked into the product library.
#include <vector>
#include "fp.hpp"
#include "tower.hpp"
#include "curve.hpp"
#include "h2c.hpp"
#include "pairing.hpp"
#include "aggveach.hpp"
#include "combsets.hpp"
#include "manyeach.hpp"
#include "plan.hpp"
using namespace bls;

namespace {
struct lines68 {
    line_t l[N_LINES];
};
}

extern "C" {
// k batches of counts[b] 320-byte records laid end to end, r: the blinding scalar of every set (the caller's: what set i has in its own
// batch), walked as the host layer walks them: slices of whole batches within cap_sets sets and cap_pairs pair slots.  verdicts: k bytes;
// gts: k x 576 bytes (zero for an empty batch).  A batch that fits no slice (`single`) is not this pass's: its verdict byte is set to 2.
// -> the number of slices walked
int emu_manyeach(const uint8_t* sets, const size_t* counts, size_t k, const uint64_t* r, size_t cap_sets, size_t cap_pairs, uint8_t* verdicts, uint8_t* gts) {
    static const uint8_t dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    std::vector<uint32_t> bad(k, 0);
    std::vector<size_t> offs(k + 1, 0), rel;
    for (size_t b = 0; b < k; b++) {
        offs[b + 1] = offs[b] + counts[b];
        verdicts[b] = 0;
        for (int i = 0; i < 576; i++) gts[b * 576 + i] = 0;
    }
    int nslices = 0;
    for (size_t b = 0; b < k;) {
        const plan::manyeach_slice sl = plan::manyeach_cut(counts, k, b, offs[b], cap_sets, cap_pairs);
        b = sl.b1;
        nslices++;
        if (sl.nb == 0) continue;
        if (sl.single) {
            for (size_t x = sl.b0; x < sl.b1; x++)
                if (counts[x]) verdicts[x] = 2;
            continue;
        }
        const uint32_t ng = sl.nb, n = (uint32_t)sl.sets;
        std::vector<plan::aggv_group> gr(ng);
        plan::aggveach_groups(offs.data(), plan::manyeach_as_groups(sl), gr.data());
        const plan::aggveach_tab tab = plan::aggveach_measure(gr.data(), ng);
        std::vector<plan::agg_item> items(tab.items);
        plan::aggveach_fill(tab, gr.data(), ng, items.data());
        rel.resize((size_t)ng + 1);
        plan::manyeach_sum_offsets(gr.data(), ng, rel.data());
        const plan::aggsets_plan sp = plan::aggsets_measure(rel.data(), ng);
        std::vector<plan::agg_item> sum_items(sp.items);
        std::vector<uint32_t> final_of(ng);
        plan::aggsets_fill(sp, rel.data(), ng, sum_items.data(), final_of.data());
        const uint8_t* rec0 = sets + sl.set0 * 320;
        // the signature side: a product per set (k_combsets_g2mul), the segmented sum per batch (k_combsets_g2_sum)
        std::vector<g2_jac> prod(n), part(sp.items ? sp.items : 1);
        for (uint32_t i = 0; i < n; i++) {
            g2_jac T[8];
            prod[i] = combsets_mul_item(g2_aff_load(rec0 + (size_t)i * 320 + 128), r[sl.set0 + i], [&](int e, const g2_jac& t) { T[e] = t; }, [&](int e) { return T[e]; });
        }
        for (uint32_t l = 0; l < sp.levels; l++)
            for (size_t it = sp.level_first[l]; it < sp.level_first[l + 1]; it++) {
                const plan::agg_item& I = sum_items[it];
                part[I.dst] = combsets_sum_item<fp2>(I.src_first, I.count, [&](uint32_t j) { return l == 0 ? prod[j] : part[j]; });
            }
        // the pair slots: k_pkmul's [r_i]PK_i against H(m_i), then what k_manyeach_setup's lanes do
        std::vector<lines68> L((size_t)n + ng);
        for (uint32_t i = 0; i < n + ng; i++) {
            if (i < n) {
                const uint8_t* rec = rec0 + (size_t)i * 320;
                if (manyeach_key_is_inf(reinterpret_cast<const uint32_t*>(rec)))
                    bad[gr[manyeach_group_of(i, ng, [&](uint32_t l) { return gr[l].first; })].g] |= 1u;
                const g1_jac p = jac_mul_u64_w4_body(g1_aff_load(rec), r[sl.set0 + i]);
                const g2_jac h = hash_to_g2(rec + 96, 32, dst, sizeof(dst) - 1);
                miller_lines(p, h, [&](int s, const line_t& l) { L[i].l[s] = l; });
            } else {
                const manyeach_pair pr = manyeach_sig_pair(part[final_of[i - n]]);
                miller_lines(pr.p, pr.q, [&](int s, const line_t& l) { L[i].l[s] = l; });
            }
        }
        // the levels of the line product, step by step, and the tail
        std::vector<fp12> lpart(tab.partials ? tab.partials : 1), step((size_t)ng * N_LINES);
        for (int s = 0; s < N_LINES; s++)
            for (uint32_t l = 0; l < tab.levels; l++)
                for (size_t it = tab.level_first[l]; it < tab.level_first[l + 1]; it++) {
                    const plan::agg_item& I = items[it];
                    const uint32_t cnt = I.count & plan::AGGV_COUNT;
                    const fp12 v = l == 0 ? aggveach_l0_item(I.src_first, cnt, (I.count & plan::AGGV_SIG) != 0, n + I.seg, [&](uint32_t j) { return L[j].l[s]; })
                                          : aggveach_ln_item(I.src_first, cnt, [&](uint32_t j) { return lpart[j]; });
                    if (I.count & plan::AGGV_FINAL) step[(size_t)I.dst * N_LINES + s] = fp12_reduce(v);
                    else lpart[I.dst] = v;
                }
        for (uint32_t i = 0; i < ng; i++) {
            const fp12 f = aggveach_horner([&](int s) { return step[(size_t)i * N_LINES + s]; });
            const aggveach_out o = aggveach_verdict(f, bad[gr[i].g] != 0);
            fp12_store_le(gts + (size_t)gr[i].g * 576, o.value);
            verdicts[gr[i].g] = o.ok ? 1 : 0;
        }
    }
    return nslices;
}
}
