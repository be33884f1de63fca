// CPU execution of the transforms over Fr (csrc/frntt.hpp lane bodies, phase by phase with 256 emulated lanes and a workgroup's LDS array as
// csrc/kernels.hip k_frntt_twiddle / k_frntt_domain / k_frntt_scale / k_frntt_pass walk them, in the order csrc/host_api.inc frntt_run
// launches them) for tests/test_frntt_emu.py, and the numbers of csrc/plan.hpp frntt_sizes_for for tests/test_frntt_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "frntt.hpp"
#include "plan.hpp"
using namespace bls;

static constexpr uint32_t T = FRNTT_LANES;

static void scale_kernel(const frntt_scale_args& a, const uint32_t* src, uint32_t* dst, uint32_t* status) {
    const uint64_t runs = a.k * ((((uint64_t)1 << a.m) + FRNTT_RUN - 1) / FRNTT_RUN), blocks = (runs + T - 1) / T;
    for (uint64_t lane = 0; lane < blocks * T; lane++) {
        uint64_t vec;
        if (frntt_scale_run(a, lane, src, dst, vec)) status[vec] |= FRNTT_ST_REDUCED;
    }
}
template <bool DIT>
static void pass_kernel(const frntt_geo& g, const uint32_t* src, bool raw, const uint32_t* tw, bool permute, uint32_t* dst, uint32_t* status) {
    const uint32_t slots = 1u << g.L;
    std::vector<uint32_t> lds((size_t)8 << g.L);
    const uint64_t wgs = frntt_workgroups(g);
    for (uint64_t w = 0; w < wgs; w++) {
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t l = t; l < slots; l += T) {
                uint64_t vec;
                if (frntt_load_item(g, w, l, src, raw, lds.data(), vec)) status[vec] |= FRNTT_ST_REDUCED;
            }
        for (uint32_t s = 0; s < g.tp; s++) {
            const uint32_t pos = g.clo + (DIT ? s : g.tp - 1 - s);
            for (uint32_t t = 0; t < T; t++)
                for (uint32_t bf = t; bf < slots / 2; bf += T) frntt_butterfly<DIT>(g, w, bf, pos, tw, lds.data());
        }
        for (uint32_t t = 0; t < T; t++)
            for (uint32_t l = t; l < slots; l += T) frntt_store_item(g, w, l, lds.data(), permute, dst);
    }
}
static std::vector<uint32_t> twiddles(size_t n, const fr& root) {
    std::vector<uint32_t> tw(n / 2 * 8 + 8);
    const uint64_t runs = (n / 2 + FRNTT_RUN - 1) / FRNTT_RUN;
    for (uint64_t lane = 0; lane < (runs + T - 1) / T * T; lane++) frntt_twiddle_run(root, lane, n / 2, tw.data());
    return tw;
}

extern "C" {
// k vectors of n images -> out (k x n x 32; out == in is allowed), status (k); returns the vectors with FRNTT_ST_REDUCED; -1: refused
// (the sizes, or a zero shift).  shift32 null: none.  passes_run: the passes of one transform, if wanted.
int emu_frntt(const uint8_t* in32, size_t n, size_t k, uint32_t flags, const uint8_t* shift32, uint32_t forced_tile, size_t forced_vecs, uint8_t* out32,
              uint8_t* status, uint32_t* passes_run) {
    const plan::frntt_sizes sz = plan::frntt_sizes_for(n, k, forced_tile, forced_vecs);
    if (!sz.ok) return -1;
    fr gm{};
    if (shift32) {
        uint32_t w[8];
        std::memcpy(w, shift32, 32);
        bool red;
        gm = fr_to_mont(fr_canon_words(w, red));
        if (fr_is_zero(gm)) return -1;
    }
    const bool inverse = flags & 1, bitrev = flags & 2;
    const uint32_t m = sz.log2n;
    const bool dit = inverse && bitrev, permute = !bitrev, second = permute && sz.passes > 1;
    fr root = frntt_omega(m);
    if (inverse) root = fr_inv(root);
    const std::vector<uint32_t> tw = twiddles(n, root);
    frntt_scale_args sa{};
    sa.m = m;
    if (inverse) {
        const uint32_t nw[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
        sa.base = fr_inv(fr_from_words(nw));
        sa.ratio = shift32 ? fr_inv(gm) : fr_one();
        sa.mult = true, sa.use_ratio = shift32 != nullptr;
    } else {
        sa.base = fr_one(), sa.ratio = gm;
        sa.mult = sa.use_ratio = shift32 != nullptr;
    }
    const bool scale_first = !inverse && (shift32 || sz.passes == 0), scale_last = inverse;
    std::vector<uint32_t> io(k * n * 8 + 8), ws(sz.vecs * n * 8 + 8), words(sz.vecs + 1);
    std::memcpy(io.data(), in32, k * n * 32);             // the device form in place: out == in
    int reduced = 0;
    for (size_t i = 0; i < sz.slices; i++) {
        size_t g0, kc;
        plan::frntt_slice(sz, k, i, g0, kc);
        const uint32_t* src = io.data() + g0 * n * 8;
        uint32_t *out = io.data() + g0 * n * 8, *mid = second ? ws.data() : out;
        std::fill(words.begin(), words.end(), 0u);
        sa.k = kc;
        bool raw = true;
        if (scale_first) {
            sa.raw = true;
            scale_kernel(sa, src, mid, words.data());
            src = mid, raw = false;
        }
        uint32_t done = 0;
        for (uint32_t p = 0; p < sz.passes; p++) {
            const uint32_t tp = sz.stages[p], sigma = dit ? done : m - done - tp;
            const plan::frntt_shape sh = plan::frntt_geo_for(m, sz.tile, sigma, tp, kc);
            const frntt_geo g{m, sigma, tp, sh.clo, sh.chi, sh.L, kc};
            const bool last = p + 1 == sz.passes;
            uint32_t* dst = last ? out : mid;
            if (dit) pass_kernel<true>(g, src, raw, tw.data(), false, dst, words.data());
            else pass_kernel<false>(g, src, raw, tw.data(), permute && last, dst, words.data());
            src = dst, raw = false, done += tp;
        }
        if (scale_last) {
            sa.raw = raw;
            scale_kernel(sa, src, out, words.data());
        }
        for (size_t v = 0; v < kc; v++) {
            status[g0 + v] = (uint8_t)words[v];
            reduced += (words[v] & FRNTT_ST_REDUCED) != 0;
        }
    }
    std::memcpy(out32, io.data(), k * n * 32);
    if (passes_run) *passes_run = sz.passes;
    return reduced;
}
// the twiddle table of n (n / 2 entries), brought out of Montgomery form
void emu_frntt_twiddles(size_t n, int inverse, uint8_t* out32) {
    uint32_t m = 0;
    while (((size_t)1 << m) < n) m++;
    fr root = frntt_omega(m);
    if (inverse) root = fr_inv(root);
    const std::vector<uint32_t> tw = twiddles(n, root);
    for (size_t j = 0; j < n / 2; j++) std::memcpy(out32 + j * 32, fr_from_mont(fropen_own(tw.data(), j)).l, 32);
}
// omega_(2^32) out of Montgomery form, squared `squarings` times
void emu_frntt_omega32(uint32_t squarings, uint8_t* out32) {
    std::memcpy(out32, fr_from_mont(frntt_omega(32 - squarings)).l, 32);
}
void emu_frntt_domain(size_t n, int bitrev, uint8_t* out32) {
    uint32_t m = 0;
    while (((size_t)1 << m) < n) m++;
    std::vector<uint32_t> out(n * 8 + 8);
    const uint64_t runs = (n + FRNTT_RUN - 1) / FRNTT_RUN;
    for (uint64_t lane = 0; lane < (runs + T - 1) / T * T; lane++) frntt_domain_run(frntt_omega(m), lane, m, bitrev != 0, out.data());
    std::memcpy(out32, out.data(), n * 32);
}
uint64_t emu_frntt_rev(uint64_t i, uint32_t m) { return frntt_rev(i, m); }

// -> 1 and out[8] = log2n, tile, passes, vecs, slices, twiddles, status, staging; stages[passes] | 0: refused
int frntt_plan_sizes(size_t n, size_t k, uint32_t forced_tile, size_t forced_vecs, size_t out[8], uint8_t stages[32]) {
    const plan::frntt_sizes s = plan::frntt_sizes_for(n, k, forced_tile, forced_vecs);
    if (!s.ok) return 0;
    out[0] = s.log2n, out[1] = s.tile, out[2] = s.passes, out[3] = s.vecs, out[4] = s.slices, out[5] = s.twiddles, out[6] = s.status, out[7] = s.staging;
    std::memcpy(stages, s.stages, 32);
    return 1;
}
// slice i: out[2] = first, count
int frntt_plan_slice(size_t n, size_t k, size_t forced_vecs, size_t i, size_t out[2]) {
    const plan::frntt_sizes s = plan::frntt_sizes_for(n, k, 0, forced_vecs);
    if (!s.ok || i >= s.slices) return 0;
    plan::frntt_slice(s, k, i, out[0], out[1]);
    return 1;
}
// the shape of a pass and its workgroups: out[4] = clo, chi, L, workgroups
void frntt_plan_geo(uint32_t log2n, uint32_t tile, uint32_t sigma, uint32_t tp, size_t vecs, uint64_t out[4]) {
    const plan::frntt_shape sh = plan::frntt_geo_for(log2n, tile, sigma, tp, vecs);
    const frntt_geo g{log2n, sigma, tp, sh.clo, sh.chi, sh.L, vecs};
    out[0] = sh.clo, out[1] = sh.chi, out[2] = sh.L, out[3] = frntt_workgroups(g);
}
uint32_t frntt_plan_tile(void) { return plan::FRNTT_TILE_LOG2; }
uint32_t frntt_plan_tile_max(void) { return plan::FRNTT_TILE_MAX_LOG2; }
}
