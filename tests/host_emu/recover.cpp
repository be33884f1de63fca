// CPU execution of the threshold-signature recovery (csrc/fr.hpp, curve.hpp jac_mul_256_w4, csrc/recover.hpp item bodies and combsets.hpp's
// G2 sum item over the tables of csrc/plan.hpp recover_fill / aggsets_fill, chunk by chunk as host_api.inc walks them) for
// tests/test_recover_emu.py, bounds tracked like tests/host_emu/emu.hip; and the numbers of csrc/plan.hpp recover_measure /
// recover_chunk_end / recover_sizes_for for tests/test_recover_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "recover.hpp"
#include "combsets.hpp"
#include "plan.hpp"
using namespace bls;

static void words_out(uint8_t* out, const uint32_t (&w)[8]) {
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(w[i] >> (8 * b));
}

extern "C" {
// r, R^2 mod r (8 little-endian words each) and -1/r mod 2^32, as the device code holds them
void emu_fr_constants(uint32_t r[8], uint32_t rr[8], uint32_t* n0) {
    for (int i = 0; i < 8; i++) r[i] = k::R_ORDER[i], rr[i] = k::FR_RR[i];
    *n0 = k::FR_N0;
}
// op 0 mul, 1 add, 2 sub, 3 inv (of a), 4 a itself, 5 is_zero (out[0]); a, b: any 32 little-endian bytes, through fr_from_le32; out:
// the canonical value, 32 little-endian bytes
void emu_fr_op(int op, const uint8_t* a32, const uint8_t* b32, uint8_t* out32) {
    const fr a = fr_from_le32(a32), b = fr_from_le32(b32);
    if (op == 5) {
        std::memset(out32, 0, 32);
        out32[0] = fr_is_zero(a);
        return;
    }
    const fr v = op == 0 ? fr_mul(a, b) : op == 1 ? fr_add(a, b) : op == 2 ? fr_sub(a, b) : op == 3 ? fr_inv(a) : a;
    uint32_t w[8];
    fr_to_words(w, v);
    words_out(out32, w);
}
// [k]S by jac_mul_256_w4 and by jac_mul_256 (S: a 192-byte blst_p2_affine image, k: 32 little-endian bytes, any value): both finished to
// their 192-byte images and status bytes by aggsigs_finish_item -> 1 when the two agree
int emu_mul_256_w4(const uint8_t* sig192, const uint8_t* k32, uint8_t* out_w4, uint8_t* out_ref, uint8_t status[2]) {
    uint32_t kk[8];
    for (int i = 0; i < 8; i++) kk[i] = (uint32_t)k32[4 * i] | ((uint32_t)k32[4 * i + 1] << 8) | ((uint32_t)k32[4 * i + 2] << 16) | ((uint32_t)k32[4 * i + 3] << 24);
    const g2_aff s = g2_aff_load(sig192);
    const aggsigs_end a = aggsigs_finish_item(false, false, jac_mul_256_w4(s, kk)), b = aggsigs_finish_item(false, false, jac_mul_256(s, kk));
    std::memcpy(out_w4, a.sig, 192);
    std::memcpy(out_ref, b.sig, 192);
    status[0] = a.status, status[1] = b.status;
    return a.status == b.status && std::memcmp(a.sig, b.sig, 192) == 0 && std::memcmp(a.wire, b.wire, 96) == 0;
}
// recover_coeff_item for the member at position `self` of the group at positions [first, first + count) of ids (32 bytes per position)
// -> the flags it raises; out32: the coefficient
uint32_t emu_recover_coeff(const uint8_t* ids, uint32_t first, uint32_t count, uint32_t self, uint8_t* out32) {
    uint32_t fl = 0;
    const fr_words c = recover_coeff_item(self, first, count, [&](uint32_t pos) { return fr_from_le32(ids + (size_t)pos * 32); }, fl);
    words_out(out32, c.w);
    return fl;
}
// what mi355_bls_recover_signature_sets computes, chunk by chunk (chunks of `chunk` members: the product passes plan::REC_MEMBERS_CHUNK),
// level by level and item by item as the kernels walk them.  1: every status 0 | 0 | -3: the plan refuses the offsets
int emu_recover_signature_sets(const uint8_t* sigs, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const uint8_t* ids, size_t chunk,
                               uint8_t* out192, uint8_t* out96, uint8_t* status, size_t* chunks_walked) {
    const plan::recover_plan rp = plan::recover_measure(offsets, k, chunk);
    if (!rp.ok || (!idx && k && offsets[k] > n_table)) return -3;
    int all = 1;
    size_t walked = 0;
    for (size_t g0 = 0; g0 < k; walked++) {
        const size_t g1 = plan::recover_chunk_end(offsets, k, g0, chunk), kc = g1 - g0, base = offsets[g0], m = offsets[g1] - base;
        if (m > rp.max_members || kc > rp.max_groups) return -4;
        std::vector<size_t> ro(kc + 1);
        for (size_t i = 0; i <= kc; i++) ro[i] = offsets[g0 + i] - base;
        const plan::aggsets_plan p = plan::aggsets_measure(ro.data(), kc);
        if (!p.ok) return -3;
        const plan::recover_sizes sz = plan::recover_sizes_for(p, m, kc);
        std::vector<plan::rec_item> members(m);
        std::vector<plan::agg_item> items(p.items);
        std::vector<uint32_t> final_of(kc), flags(sz.flags / 4, 0);
        plan::recover_fill(offsets, g0, g1, members.data());
        plan::aggsets_fill(p, ro.data(), kc, items.data(), final_of.data());
        std::vector<g2_jac> prod(sz.prod / (plan::G2_WORDS * 4)), part(sz.part / (plan::G2_WORDS * 4));
        for (size_t i = 0; i < m; i++) {
            const plan::rec_item& it = members[i];
            uint32_t fl = 0;
            const fr_words cf = recover_coeff_item(it.pos, it.seg_first, it.seg_len, [&](uint32_t pos) { return fr_from_le32(ids + (size_t)pos * 32); }, fl);
            prod.at(it.pos - base) = recover_mul_item(cf, it.pos, idx, n_table, [&](size_t t) { return g2_aff_load(sigs + t * 192); }, fl);
            flags.at(it.seg) |= fl;
        }
        for (uint32_t l = 0; l < p.levels; l++)
            for (size_t i = p.level_first[l]; i < p.level_first[l + 1]; i++) {
                const plan::agg_item& it = items[i];
                part.at(it.dst) = combsets_sum_item<fp2>(it.src_first, it.count, [&](uint32_t j) { return l == 0 ? prod.at(j) : part.at(j); });
            }
        for (size_t g = 0; g < kc; g++) {
            const aggsigs_end e = recover_finish_item((uint32_t)(ro[g + 1] - ro[g]), flags[g], final_of[g] == plan::AGG_NONE ? jac_inf<fp2>() : part.at(final_of[g]));
            if (out192) std::memcpy(out192 + (g0 + g) * 192, e.sig, 192);
            if (out96) std::memcpy(out96 + (g0 + g) * 96, e.wire, 96);
            status[g0 + g] = e.status;
            all &= e.status == AGG_OK;
        }
        g0 = g1;
    }
    if (walked != rp.chunks) return -4;
    if (chunks_walked) *chunks_walked = walked;
    return all;
}
// plan.hpp recover_measure: -> 1 and out[5] = lo, members, chunks, max_members, max_groups | 0.  chunk == 0: the product's constant.
int recover_plan_measure(const size_t* offsets, size_t k, size_t chunk, size_t out[5]) {
    const plan::recover_plan p = chunk ? plan::recover_measure(offsets, k, chunk) : plan::recover_measure(offsets, k);
    if (!p.ok) return 0;
    out[0] = p.lo, out[1] = p.members, out[2] = p.chunks, out[3] = p.max_members, out[4] = p.max_groups;
    return 1;
}
size_t recover_plan_chunk_end(const size_t* offsets, size_t k, size_t g0, size_t chunk) {
    return chunk ? plan::recover_chunk_end(offsets, k, g0, chunk) : plan::recover_chunk_end(offsets, k, g0);
}
size_t recover_plan_chunk(void) { return plan::REC_MEMBERS_CHUNK; }
// the workspace of the chunk of groups [g0, g1): -> 1, sizes[7] = prod, part, tab, flags, status, out192, out96 (bytes) and the sum's items | 0
int recover_plan_sizes(const size_t* offsets, size_t g0, size_t g1, size_t sizes[7], size_t* items) {
    std::vector<size_t> ro(g1 - g0 + 1);
    for (size_t i = 0; i <= g1 - g0; i++) ro[i] = offsets[g0 + i] - offsets[g0];
    const plan::aggsets_plan p = plan::aggsets_measure(ro.data(), g1 - g0);
    if (!p.ok) return 0;
    const plan::recover_sizes s = plan::recover_sizes_for(p, offsets[g1] - offsets[g0], g1 - g0);
    sizes[0] = s.prod, sizes[1] = s.part, sizes[2] = s.tab, sizes[3] = s.flags, sizes[4] = s.status, sizes[5] = s.out192, sizes[6] = s.out96;
    *items = p.items;
    // the member items a chunk's table starts with: positions in order, every one inside its group
    std::vector<plan::rec_item> members(offsets[g1] - offsets[g0]);
    plan::recover_fill(offsets, g0, g1, members.data());
    for (size_t i = 0; i < members.size(); i++) {
        const plan::rec_item& it = members[i];
        if (it.pos != offsets[g0] + i || it.seg >= g1 - g0 || it.seg_first != offsets[g0 + it.seg] || it.seg_len != offsets[g0 + it.seg + 1] - offsets[g0 + it.seg] ||
            it.pos < it.seg_first || it.pos - it.seg_first >= it.seg_len)
            return 0;
    }
    return 1;
}
}
