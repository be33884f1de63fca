// CPU execution of the transforms over G1 (csrc/p1ntt.hpp lane bodies, lane by lane as csrc/kernels.hip k_p1ntt_twiddle / k_p1ntt_stage /
// k_p1ntt_finish walk them, in the order and with the launch shapes csrc/host_api.inc p1ntt_run uses) for tests/test_p1ntt_emu.py, bounds
// tracked like tests/host_emu/lincomb.cpp.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "p1ntt.hpp"
#include "plan.hpp"
using namespace bls;

static constexpr uint32_t T = plan::WAVE;

static std::vector<uint32_t> twiddles(size_t n, const fr& root) {
    std::vector<uint32_t> tw(n / 2 * 8 + 8);
    const uint64_t runs = (n / 2 + FRNTT_RUN - 1) / FRNTT_RUN;
    for (uint64_t lane = 0; lane < (runs + FRNTT_LANES - 1) / FRNTT_LANES * FRNTT_LANES; lane++) p1ntt_twiddle_run(root, lane, n / 2, tw.data());
    return tw;
}
static void words_in(uint32_t (&w)[8], const uint8_t* b) {
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
static void image_out(uint8_t* out, const g1_jac& p) {
    std::memset(out, 0, 96);
    if (jac_is_inf(p)) return;
    const fp zi = f_inv(p.z), zi2 = f_sqr(zi);
    fp_store_le(out, f_mul(p.x, zi2));
    fp_store_le(out + 48, f_mul(p.y, f_mul(zi2, zi)));
}

extern "C" {
// k vectors of n images -> out (k x n x 96; out == in is allowed).  0, or -1: the plan refuses n.  slices_run, if wanted: the slices walked;
// twiddle_loads: the butterflies that read the table, which is those that multiply by a twiddle.
int emu_p1ntt(const uint8_t* in96, size_t n, size_t k, uint32_t flags, size_t forced_vecs, uint8_t* out96, size_t* slices_run, size_t* twiddle_loads) {
    const plan::p1ntt_sizes sz = plan::p1ntt_sizes_for(n, k, forced_vecs);
    if (!sz.ok) return -1;
    const bool inverse = flags & 1, bitrev = flags & 2;
    const uint32_t m = sz.log2n;
    const bool dit = inverse && bitrev, permute = !bitrev;
    std::vector<uint32_t> tw;
    p1ntt_stage g{};
    g.m = m;
    if (m) {
        fr root = frntt_omega(m);
        if (inverse) root = fr_inv(root);
        tw = twiddles(n, root);
    }
    if (inverse) {
        const uint32_t nw[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
        g.s_mont = fr_inv(fr_from_words(nw));
        fr_to_words(g.s, g.s_mont);
    }
    size_t loads = 0;
    std::vector<uint8_t> io(in96, in96 + k * n * 96);           // the device form in place: out == in
    std::vector<g1_jac> ws(sz.ws / (plan::G1_WORDS * 4));
    for (size_t i = 0; i < sz.slices; i++) {
        size_t g0, kc;
        plan::p1ntt_slice(sz, k, i, g0, kc);
        const plan::p1ntt_launch l = plan::p1ntt_launch_for(sz, kc);
        uint8_t* slice = io.data() + g0 * n * 96;
        g.k = kc;
        for (uint32_t s = 0; s < m; s++) {
            g.b = dit ? s : m - 1 - s;
            g.scaled = inverse && g.b == m - 1;
            const bool first = s == 0;
            const auto load = [&](uint64_t e) { return first ? jac_from_aff(g1_aff_load(slice + e * 96)) : ws.at(e); };
            const auto store = [&](uint64_t e, const g1_jac& a) { ws.at(e) = a; };
            const auto twd = [&](uint64_t t) {
                loads++;
                return fropen_own(tw.data(), (size_t)t);
            };
            for (uint64_t lane = 0; lane < (uint64_t)l.stage_grid * T; lane++) {
                if (lane >= p1ntt_lanes(g)) continue;
                if (dit) p1ntt_butterfly<true, fp>(g, lane, load, store, twd);
                else p1ntt_butterfly<false, fp>(g, lane, load, store, twd);
            }
        }
        for (uint64_t lane = 0; lane < (uint64_t)l.finish_grid * T; lane++)
            p1ntt_finish_run<fp>(
                (uint64_t)kc << m, m, permute, l.run, lane, [&](uint64_t e) { return m ? ws.at(e) : jac_from_aff(g1_aff_load(slice + e * 96)); },
                [&](uint64_t slot, const g1_aff& a) {
                    fp_store_le(slice + slot * 96, a.x);
                    fp_store_le(slice + slot * 96 + 48, a.y);
                },
                [&](uint64_t slot) { std::memset(slice + slot * 96, 0, 96); });
    }
    std::memcpy(out96, io.data(), k * n * 96);
    if (slices_run) *slices_run = sz.slices;
    if (twiddle_loads) *twiddle_loads = loads;
    return 0;
}
// [k]P by the Jacobian-base walk, the base given a Z of its own ((x z^2, y z^3, z) with z = x + 1 of the affine image), and by the
// bit-serial jac_mul_256 on the affine point; both as affine images.  -> 1 when they agree.  The all-zero image: infinity.
int emu_p1ntt_mul(const uint8_t* pt96, const uint8_t* k32, uint8_t* out96, uint8_t* out_ref96) {
    const g1_aff p = g1_aff_load(pt96);
    uint32_t kk[8];
    words_in(kk, k32);
    g1_jac base = jac_from_aff(p);
    if (!jac_is_inf(base)) {
        const fp z = f_add(p.x, f_one<fp>()), z2 = f_sqr(z);
        base = g1_jac{f_mul(p.x, z2), f_mul(p.y, f_mul(z2, z)), z};
    }
    image_out(out96, jac_mul_256_w4_jac_body(base, kk));
    image_out(out_ref96, jac_mul_256(p, kk));
    return std::memcmp(out96, out_ref96, 96) == 0;
}
// the twiddle table of n (n / 2 plain canonical entries)
void emu_p1ntt_twiddles(size_t n, int inverse, uint8_t* out32) {
    uint32_t m = 0;
    while (((size_t)1 << m) < n) m++;
    fr root = frntt_omega(m);
    if (inverse) root = fr_inv(root);
    const std::vector<uint32_t> tw = twiddles(n, root);
    std::memcpy(out32, tw.data(), n / 2 * 32);
}
// the lanes of the stage at bit b of k vectors of 2^m points, and lane -> out[3] = i0, i1, table entry
uint64_t emu_p1ntt_lanes(uint32_t m, uint32_t b, uint64_t k) {
    p1ntt_stage g{};
    g.m = m, g.b = b, g.k = k;
    return p1ntt_lanes(g);
}
void emu_p1ntt_pair(uint32_t m, uint32_t b, uint64_t k, uint64_t lane, uint64_t out[3]) {
    p1ntt_stage g{};
    g.m = m, g.b = b, g.k = k;
    const p1ntt_pair pr = p1ntt_pair_of(g, lane);
    out[0] = pr.i0, out[1] = pr.i1, out[2] = pr.tw;
}
}
