// CPU execution of the per-group aggregateVerify bodies (csrc/aggveach.hpp) over the plan's own slices and item tables (csrc/plan.hpp
// aggveach_cut / aggveach_groups / aggveach_fill) for tests/test_aggveach_emu.py, bounds tracked like tests/host_emu/emu.hip.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <vector>
#include "fp.hpp"
#include "tower.hpp"
#include "curve.hpp"
#include "h2c.hpp"
#include "pairing.hpp"
#include "aggveach.hpp"
#include "plan.hpp"
using namespace bls;

namespace {
struct lines68 {
    line_t l[N_LINES];
};
}

extern "C" {
// k groups in CSR form (group g = pairs [offsets[g], offsets[g + 1]) of pks96 / msgs32, sigs192: one signature per group), walked as the
// host layer walks them: slices of at most `cap` pairs, item tables of width C, the open group's Miller value carried through a
// blst_fp12 image.  verdicts: k bytes; gts: k x 576 bytes, final_exp(f_g) (zero for an empty group).  The lines of a pair are what the line
// kernels store: miller_lines of (pk, H(msg)) and of (-G1, sig), line_one() throughout for a pair with an operand at infinity.
// -> the number of slices walked
int emu_aggveach(const uint8_t* pks96, const uint8_t* msgs32, const size_t* offsets, size_t k, const uint8_t* sigs192, uint32_t C, size_t cap,
                 uint8_t* verdicts, uint8_t* gts) {
    static const uint8_t dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    std::vector<uint8_t> bad(k, 0);
    for (size_t g = 0; g < k; g++) {
        verdicts[g] = 0;
        for (int i = 0; i < 576; i++) gts[g * 576 + i] = 0;
    }
    uint8_t carry[576];
    int nslices = 0;
    size_t g = 0, pos = k ? offsets[0] : 0;
    for (;;) {
        const plan::aggv_slice sl = plan::aggveach_cut(offsets, k, g, pos, cap);
        if (sl.pairs() == 0) break;
        nslices++;
        std::vector<plan::aggv_group> gr(sl.ng);
        plan::aggveach_groups(offsets, sl, gr.data());
        const plan::aggveach_tab tab = plan::aggveach_measure(gr.data(), sl.ng, C);
        std::vector<plan::agg_item> items(tab.items);
        plan::aggveach_fill(tab, gr.data(), sl.ng, items.data(), C);
        const size_t P = sl.pairs();
        // the slice's pair slots: the pairs, then the signature pair of every group that ends here
        std::vector<lines68> L(P + sl.sigs());
        for (size_t i = 0; i < P; i++) {
            const g1_aff pk = g1_aff_load(pks96 + (sl.pos0 + i) * 96);
            const g2_jac h = hash_to_g2(msgs32 + (sl.pos0 + i) * 32, 32, dst, sizeof(dst) - 1);
            miller_lines(jac_from_aff(pk), h, [&](int s, const line_t& l) { L[i].l[s] = l; });
        }
        for (uint32_t i = 0; i < sl.ng; i++) {
            for (uint32_t j = 0; j < gr[i].count; j++)
                if (aff_is_inf(g1_aff_load(pks96 + (sl.pos0 + gr[i].first + j) * 96))) bad[gr[i].g] = 1;
            if (gr[i].flags & plan::AGGV_OPEN_OUT) continue;
            const g2_aff sig = g2_aff_load(sigs192 + (size_t)gr[i].g * 192);
            miller_lines(g1_jac{fp_from_const(k::G1_X), fp_from_const(k::G1_NEG_Y), fp_one()}, jac_from_aff(sig),
                         [&](int s, const line_t& l) { L[P + i].l[s] = l; });
        }
        // the levels, step by step: partials and step values as the device stores hold them
        std::vector<fp12> part(tab.partials ? tab.partials : 1), step((size_t)sl.ng * N_LINES);
        for (int s = 0; s < N_LINES; s++)
            for (uint32_t l = 0; l < tab.levels; l++)
                for (size_t it = tab.level_first[l]; it < tab.level_first[l + 1]; it++) {
                    const plan::agg_item& I = items[it];
                    const uint32_t cnt = I.count & plan::AGGV_COUNT;
                    const fp12 v = l == 0 ? aggveach_l0_item(I.src_first, cnt, (I.count & plan::AGGV_SIG) != 0, (uint32_t)P + I.seg,
                                                             [&](uint32_t j) { return L[j].l[s]; })
                                          : aggveach_ln_item(I.src_first, cnt, [&](uint32_t j) { return part[j]; });
                    if (I.count & plan::AGGV_FINAL) step[(size_t)I.dst * N_LINES + s] = fp12_reduce(v);
                    else part[I.dst] = v;
                }
        for (uint32_t i = 0; i < sl.ng; i++) {
            fp12 f = aggveach_horner([&](int s) { return step[(size_t)i * N_LINES + s]; });
            if (gr[i].flags & plan::AGGV_OPEN_IN) f = aggveach_carry(f, fp12_load_le(carry));
            if (gr[i].flags & plan::AGGV_OPEN_OUT) {
                fp12_store_le(carry, f);
                continue;
            }
            const aggveach_out o = aggveach_verdict(f, bad[gr[i].g] != 0);
            fp12_store_le(gts + (size_t)gr[i].g * 576, o.value);
            verdicts[gr[i].g] = o.ok ? 1 : 0;
        }
        g = sl.next_g(), pos = sl.pos1;
    }
    return nslices;
}
}
