// CPU execution of the short linear combinations (csrc/lincomb.hpp item bodies and combsets.hpp's sum item over the tables of csrc/plan.hpp
// recover_fill / aggsets_fill, chunk by chunk as host_api.inc walks them) for tests/test_lincomb_emu.py, bounds tracked like
// tests/host_emu/emu.hip; and the numbers of csrc/plan.hpp lincomb_measure / lincomb_chunk_end / lincomb_sizes_for for
// tests/test_lincomb_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "lincomb.hpp"
#include "plan.hpp"
using namespace bls;

static void words_in(uint32_t (&w)[8], const uint8_t* b) {
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
static g1_aff aff_load(const uint8_t* p, const g1_aff*) { return g1_aff_load(p); }
static g2_aff aff_load(const uint8_t* p, const g2_aff*) { return g2_aff_load(p); }

// the two multiplications of one point by one scalar, each against the bit-serial jac_mul_256 on the masked scalar as an integer; all
// four finished by lincomb_finish_item.  -> 1 when image and status agree.  psi: lincomb_mul_psi_item's reduction and walk (G2 only).
template <class F>
static int mul_pair(const uint8_t* pt, const uint8_t* k32, uint32_t nbits, bool psi, uint8_t* out, uint8_t* out_ref, uint8_t status[2]) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192;
    const aff<F> p = aff_load(pt, (const aff<F>*)nullptr);
    uint32_t raw[8], kk[8], fl = 0;
    words_in(raw, k32);
    lincomb_scalar(kk, nbits, [&](int i) { return raw[i]; });
    const auto point = [&](size_t) { return p; };
    const auto word = [&](uint32_t, int i) { return raw[i]; };
    jac<F> r;
    if constexpr (sizeof(F) != sizeof(fp)) r = psi ? lincomb_mul_psi_item(0, nullptr, 1, nbits, point, word, fl) : lincomb_mul_item<F>(0, nullptr, 1, nbits, point, word, fl);
    else r = lincomb_mul_item<F>(0, nullptr, 1, nbits, point, word, fl);
    const lincomb_end<F> a = lincomb_finish_item<F>(1, fl, r), b = lincomb_finish_item<F>(1, 0, jac_mul_256(p, kk));
    std::memcpy(out, a.img, AFFB);
    std::memcpy(out_ref, b.img, AFFB);
    status[0] = a.status, status[1] = b.status;
    return a.status == b.status && std::memcmp(a.img, b.img, AFFB) == 0;
}

// what mi355_bls_p?s_lincomb_many computes, chunk by chunk (forced: the test hook's chunk, 0: the product's), level by level and item by item
// as the kernels walk them.  1: every status 0 | 0 | -3: the plan refuses the offsets | -4: a chunk outgrew the measured workspace
template <class F>
static int many(const uint8_t* pts, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const uint8_t* sc, uint32_t nbits, bool psi, size_t forced,
                uint8_t* out, uint8_t* status, size_t* chunks_walked) {
    constexpr bool G2 = sizeof(F) != sizeof(fp);
    constexpr size_t AFFB = G2 ? 192 : 96, JACB = (G2 ? plan::G2_WORDS : plan::G1_WORDS) * 4;
    const plan::recover_plan rp = plan::lincomb_measure(offsets, k, forced);
    if (!rp.ok || (!idx && k && offsets[k] > n_table)) return -3;
    int all = 1;
    size_t walked = 0;
    for (size_t g0 = 0; g0 < k; walked++) {
        const size_t g1 = plan::lincomb_chunk_end(offsets, k, g0, forced), kc = g1 - g0, base = offsets[g0], m = offsets[g1] - base;
        if (m > rp.max_members || kc > rp.max_groups) return -4;
        std::vector<size_t> ro(kc + 1);
        for (size_t i = 0; i <= kc; i++) ro[i] = offsets[g0 + i] - base;
        const plan::aggsets_plan p = plan::aggsets_measure(ro.data(), kc);
        if (!p.ok) return -3;
        const plan::lincomb_sizes sz = plan::lincomb_sizes_for(p, m, kc, G2);
        std::vector<plan::rec_item> terms(m);
        std::vector<plan::agg_item> items(p.items);
        std::vector<uint32_t> final_of(kc), flags(sz.flags / 4, 0);
        plan::recover_fill(offsets, g0, g1, terms.data());
        plan::aggsets_fill(p, ro.data(), kc, items.data(), final_of.data());
        std::vector<jac<F>> prod(sz.prod / JACB), part(sz.part / JACB);
        const auto point = [&](size_t t) { return aff_load(pts + t * AFFB, (const aff<F>*)nullptr); };
        const auto word = [&](uint32_t pos, int i) {
            const uint8_t* b = sc + (size_t)pos * 32 + 4 * i;
            return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        };
        for (size_t i = 0; i < m; i++) {
            const plan::rec_item& it = terms[i];
            uint32_t fl = 0;
            jac<F> r;
            if constexpr (G2) r = psi ? lincomb_mul_psi_item(it.pos, idx, n_table, nbits, point, word, fl) : lincomb_mul_item<F>(it.pos, idx, n_table, nbits, point, word, fl);
            else r = lincomb_mul_item<F>(it.pos, idx, n_table, nbits, point, word, fl);
            prod.at(it.pos - base) = r;
            flags.at(it.seg) |= fl;
        }
        for (uint32_t l = 0; l < p.levels; l++)
            for (size_t i = p.level_first[l]; i < p.level_first[l + 1]; i++) {
                const plan::agg_item& it = items[i];
                part.at(it.dst) = combsets_sum_item<F>(it.src_first, it.count, [&](uint32_t j) { return l == 0 ? prod.at(j) : part.at(j); });
            }
        for (size_t g = 0; g < kc; g++) {
            const lincomb_end<F> e = lincomb_finish_item<F>((uint32_t)(ro[g + 1] - ro[g]), flags[g], final_of[g] == plan::AGG_NONE ? jac_inf<F>() : part.at(final_of[g]));
            std::memcpy(out + (g0 + g) * AFFB, e.img, AFFB);
            status[g0 + g] = e.status;
            all &= e.status == AGG_OK;
        }
        g0 = g1;
    }
    if (walked != rp.chunks) return -4;
    if (chunks_walked) *chunks_walked = walked;
    return all;
}

extern "C" {
// the base-X digits lincomb_mul_psi_item walks for the scalar k32 (any 32 little-endian bytes) under nbits: mask, reduce mod r, expand
void emu_lincomb_base_x(const uint8_t* k32, uint32_t nbits, uint64_t out[4]) {
    uint32_t raw[8], kk[8], red[8];
    words_in(raw, k32);
    lincomb_scalar(kk, nbits, [&](int i) { return raw[i]; });
    fr_to_words(red, fr_from_words(kk));
    const lincomb_digits d = lincomb_base_x(red);
    for (int i = 0; i < 4; i++) out[i] = d.d[i];
}
uint64_t emu_lincomb_x_abs(void) { return k::X_ABS; }
int emu_lincomb_mul(int g2, const uint8_t* pt, const uint8_t* k32, uint32_t nbits, int psi, uint8_t* out, uint8_t* out_ref, uint8_t status[2]) {
    return g2 ? mul_pair<fp2>(pt, k32, nbits, psi != 0, out, out_ref, status) : mul_pair<fp>(pt, k32, nbits, false, out, out_ref, status);
}
int emu_lincomb_many(int g2, const uint8_t* pts, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const uint8_t* sc, uint32_t nbits, int psi,
                     size_t forced, uint8_t* out, uint8_t* status, size_t* chunks_walked) {
    return g2 ? many<fp2>(pts, n_table, idx, offsets, k, sc, nbits, psi != 0, forced, out, status, chunks_walked)
              : many<fp>(pts, n_table, idx, offsets, k, sc, nbits, false, forced, out, status, chunks_walked);
}
// plan.hpp lincomb_measure: -> 1 and out[5] = lo, members, chunks, max_members, max_groups | 0.  forced == 0: the product's constant.
int lincomb_plan_measure(const size_t* offsets, size_t k, size_t forced, size_t out[5]) {
    const plan::recover_plan p = plan::lincomb_measure(offsets, k, forced);
    if (!p.ok) return 0;
    out[0] = p.lo, out[1] = p.members, out[2] = p.chunks, out[3] = p.max_members, out[4] = p.max_groups;
    return 1;
}
size_t lincomb_plan_chunk_end(const size_t* offsets, size_t k, size_t g0, size_t forced) { return plan::lincomb_chunk_end(offsets, k, g0, forced); }
size_t lincomb_plan_chunk(size_t forced) { return plan::lincomb_chunk(forced); }
// the workspace of the chunk of groups [g0, g1): -> 1, sizes[6] = prod, part, tab, flags, status, out (bytes) and the sum's items | 0
int lincomb_plan_sizes(const size_t* offsets, size_t g0, size_t g1, int g2, size_t sizes[6], size_t* items) {
    std::vector<size_t> ro(g1 - g0 + 1);
    for (size_t i = 0; i <= g1 - g0; i++) ro[i] = offsets[g0 + i] - offsets[g0];
    const plan::aggsets_plan p = plan::aggsets_measure(ro.data(), g1 - g0);
    if (!p.ok) return 0;
    const plan::lincomb_sizes s = plan::lincomb_sizes_for(p, offsets[g1] - offsets[g0], g1 - g0, g2 != 0);
    sizes[0] = s.prod, sizes[1] = s.part, sizes[2] = s.tab, sizes[3] = s.flags, sizes[4] = s.status, sizes[5] = s.out;
    *items = p.items;
    return 1;
}
}
