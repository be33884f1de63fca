// CPU execution of the openings over Fr (csrc/fropen.hpp lane bodies, phase by phase with 256 emulated lanes and the workgroup's arrays as
// csrc/kernels.hip k_fropen_coef / k_fropen_domain / k_fropen_eval walk them) for tests/test_fropen_emu.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "fropen.hpp"
using namespace bls;

static constexpr uint32_t T = FROPEN_LANES;

static std::vector<uint32_t> words_of(const uint8_t* b, size_t images) {
    std::vector<uint32_t> w(images * 8 + 4);          // (the tail keeps an empty array's data() non-null)
    if (images) std::memcpy(w.data(), b, images * 32);
    return w;
}
static void wg_sum(fr* sh) {
    for (uint32_t dist = T / 2; dist; dist >>= 1)
        for (uint32_t t = 0; t < T; t++) fropen_sum_step(sh, t, dist);
}

extern "C" {
// k polynomials in coefficient form -> ys (k x 32), quot (k x n x 32), status (k); returns the polynomials with FROPEN_ST_REDUCED
int emu_fropen_coef(const uint8_t* polys32, size_t n, const uint8_t* zs32, size_t k, uint8_t* ys, uint8_t* quot, uint8_t* status) {
    const std::vector<uint32_t> polys = words_of(polys32, k * n), zs = words_of(zs32, k);
    std::vector<uint32_t> q(n * 8);
    int reduced = 0;
    for (size_t g = 0; g < k; g++) {
        const uint32_t* poly = polys.data() + g * n * 8;
        fr sh[T], next[T];
        uint32_t flags = 0;
        const fr zm = fr_to_mont(fropen_image(zs.data(), g, flags));
        for (uint32_t t = 0; t < T; t++) sh[t] = fropen_coef_horner(poly, fropen_chunk(t, n), zm, flags);
        fr pw = fr_pow_u64(zm, fropen_chunk_len(n));
        for (uint32_t s = 0; s < FROPEN_SCAN_STEPS; s++) {
            for (uint32_t t = 0; t < T; t++) next[t] = fropen_coef_scan_step(sh, t, s, pw);
            for (uint32_t t = 0; t < T; t++) sh[t] = next[t];
            pw = fr_sqr(pw);
        }
        for (uint32_t t = 0; t < T; t++) fropen_coef_emit(poly, fropen_chunk(t, n), zm, t + 1 < T ? sh[t + 1] : fr{}, q.data());
        std::memcpy(quot + g * n * 32, q.data(), n * 32);
        std::memcpy(ys + g * 32, sh[0].l, 32);
        status[g] = (uint8_t)flags;
        reduced += (flags & FROPEN_ST_REDUCED) != 0;
    }
    return reduced;
}
// the same in evaluation form over the n = 2^log2n domain images; -1: n is no power of two
int emu_fropen_eval(const uint8_t* polys32, size_t n, const uint8_t* zs32, size_t k, const uint8_t* domain32, uint8_t* ys, uint8_t* quot, uint8_t* status,
                    size_t* inversions) {
    if (n == 0 || (n & (n - 1))) return -1;
    uint32_t log2n = 0;
    while (((size_t)1 << log2n) < n) log2n++;
    const std::vector<uint32_t> polys = words_of(polys32, k * n), zs = words_of(zs32, k), dom = words_of(domain32, n);
    std::vector<uint32_t> ws_dom(n * 8), scan(n * 8), q(n * 8);
    for (size_t i = 0; i < n; i++) fropen_domain_item(dom.data(), i, ws_dom.data());
    const uint32_t nw[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
    const fr ninv = fr_inv(fr_from_words(nw));
    const auto mul = [](const fr& a, const fr& b) { return fr_mont_mul(a, b); };
    int reduced = 0;
    size_t invs = 0;
    for (size_t g = 0; g < k; g++) {
        const uint32_t* poly = polys.data() + g * n * 8;
        std::fill(q.begin(), q.end(), 0xa5a5a5a5u);
        fr before[T], behind[T], na[T], nb[T], part[T];
        uint32_t flags = 0;
        uint64_t j = FROPEN_NO_J;
        const fr zm = fr_to_mont(fropen_image(zs.data(), g, flags));
        for (uint32_t t = 0; t < T; t++) {
            uint64_t mine = FROPEN_NO_J;
            before[t] = behind[t] = fropen_eval_products(ws_dom.data(), fropen_chunk(t, n), zm, scan.data(), mine);
            if (mine != FROPEN_NO_J) j = mine;
        }
        for (uint32_t s = 0; s < FROPEN_SCAN_STEPS; s++) {
            for (uint32_t t = 0; t < T; t++) na[t] = fropen_scan_step(before, t, 1u << s, false, mul), nb[t] = fropen_scan_step(behind, t, 1u << s, true, mul);
            for (uint32_t t = 0; t < T; t++) before[t] = na[t], behind[t] = nb[t];
        }
        const fr inv_all = fr_inv(behind[0]);
        invs++;
        for (uint32_t t = 0; t < T; t++)
            part[t] = fropen_eval_invert(poly, ws_dom.data(), fropen_chunk(t, n), zm, fropen_eval_lane_inverse(inv_all, before, behind, t), j, scan.data(), flags);
        wg_sum(part);
        const fropen_zpow zp = fropen_z_powers(zm, log2n);
        const fr y = fropen_eval_value(poly, part[0], zp.zn, ninv, j);
        for (uint32_t t = 0; t < T; t++) part[t] = fropen_eval_emit(poly, ws_dom.data(), fropen_chunk(t, n), y, j, scan.data(), q.data());
        if (j != FROPEN_NO_J) {
            wg_sum(part);
            fropen_st(q.data() + (size_t)j * 8, fropen_eval_slot_j(part[0], zp.zn1));
        }
        std::memcpy(quot + g * n * 32, q.data(), n * 32);
        std::memcpy(ys + g * 32, y.l, 32);
        status[g] = (uint8_t)(flags | (j != FROPEN_NO_J ? FROPEN_ST_IN_DOMAIN : 0u));
        reduced += (flags & FROPEN_ST_REDUCED) != 0;
    }
    if (inversions) *inversions = invs;
    return reduced;
}
// fr.hpp's additions on one value each: out = neg | sqr (Montgomery in, Montgomery out: the test converts) | canon | to_mont then from_mont
void emu_fr_ops(const uint8_t* a32, uint8_t* neg, uint8_t* sqr, uint8_t* canon, uint8_t* round_trip, int* reduced) {
    uint32_t w[8];
    std::memcpy(w, a32, 32);
    bool red;
    const fr a = fr_canon_words(w, red);
    *reduced = red;
    std::memcpy(canon, a.l, 32);
    std::memcpy(neg, fr_neg(a).l, 32);
    std::memcpy(sqr, fr_from_mont(fr_sqr(fr_to_mont(a))).l, 32);
    std::memcpy(round_trip, fr_from_mont(fr_to_mont(a)).l, 32);
}
// a^e through fr_pow_u64
void emu_fr_pow(const uint8_t* a32, uint64_t e, uint8_t* out) {
    uint32_t w[8];
    std::memcpy(w, a32, 32);
    std::memcpy(out, fr_from_mont(fr_pow_u64(fr_from_words(w), e)).l, 32);
}
}
