// CPU execution of the all-openings call (csrc/fk20.hpp lane bodies with those of csrc/frntt.hpp and csrc/p1ntt.hpp they run between, lane by
// lane as csrc/kernels.hip k_fk20_* / k_frntt_pass / k_p1ntt_stage walk them, in the order and with the launch shapes csrc/host_api.inc
// mi355_bls_fk20_setup_create_device and fk20_run use) for tests/test_fk20_emu.py, bounds tracked like tests/host_emu/p1ntt.cpp.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "fk20.hpp"
#include "plan.hpp"
using namespace bls;

static constexpr uint32_t T = plan::WAVE;

static std::vector<uint32_t> point_twiddles(size_t count, const fr& root) {
    std::vector<uint32_t> tw(count * 8 + 8);
    const uint64_t runs = (count + FRNTT_RUN - 1) / FRNTT_RUN;
    for (uint64_t lane = 0; lane < (runs + FRNTT_LANES - 1) / FRNTT_LANES * FRNTT_LANES; lane++) p1ntt_twiddle_run(root, lane, count, tw.data());
    return tw;
}
static std::vector<uint32_t> fr_twiddles(size_t count, const fr& root) {
    std::vector<uint32_t> tw(count * 8 + 8);
    const uint64_t runs = (count + FRNTT_RUN - 1) / FRNTT_RUN;
    for (uint64_t lane = 0; lane < (runs + FRNTT_LANES - 1) / FRNTT_LANES * FRNTT_LANES; lane++) frntt_twiddle_run(root, lane, count, tw.data());
    return tw;
}
// k_frntt_pass<false> over one array, in place, no permutation
static void fr_pass(const frntt_geo& g, const uint32_t* tw, uint32_t* io) {
    const uint32_t slots = 1u << g.L;
    std::vector<uint32_t> lds((size_t)8 << g.L);
    const uint64_t wgs = frntt_workgroups(g);
    for (uint64_t w = 0; w < wgs; w++) {
        for (uint32_t l = 0; l < slots; l++) {
            uint64_t vec;
            frntt_load_item(g, w, l, io, false, lds.data(), vec);
        }
        for (uint32_t s = 0; s < g.tp; s++)
            for (uint32_t bf = 0; bf < slots / 2; bf++) frntt_butterfly<false>(g, w, bf, g.clo + g.tp - 1 - s, tw, lds.data());
        for (uint32_t l = 0; l < slots; l++) frntt_store_item(g, w, l, lds.data(), false, io);
    }
}
static void store_aff(uint8_t* at, const g1_aff& a) {
    fp_store_le(at, a.x);
    fp_store_le(at + 48, a.y);
}
// the setup: s^ laid out (k_fk20_setup_layout), then p1ntt_run's forward BITREV walk of 2n points in place -> x (2n x 96)
static void setup(const uint8_t* srs96, size_t n, std::vector<uint8_t>& x) {
    const size_t n2 = 2 * n;
    x.assign(n2 * 96, 0);
    for (uint64_t u = 0; u < n2; u++) {
        uint64_t j;
        if (fk20_setup_src(n, u, j)) std::memcpy(&x[u * 96], srs96 + j * 96, 96);
    }
    const plan::p1ntt_sizes sz = plan::p1ntt_sizes_for(n2, 1, 0);
    const plan::p1ntt_launch l = plan::p1ntt_launch_for(sz, 1);
    const uint32_t M = sz.log2n;
    const std::vector<uint32_t> tw = point_twiddles(n2 / 2, frntt_omega(M));
    std::vector<g1_jac> ws(n2);
    p1ntt_stage g{};
    g.m = M, g.k = 1;
    for (uint32_t s = 0; s < M; s++) {
        g.b = M - 1 - s;
        const bool first = s == 0;
        for (uint64_t lane = 0; lane < (uint64_t)l.stage_grid * T; lane++) {
            if (lane >= p1ntt_lanes(g)) continue;
            p1ntt_butterfly<false, fp>(
                g, lane, [&](uint64_t e) { return first ? jac_from_aff(g1_aff_load(&x.at(e * 96))) : ws.at(e); }, [&](uint64_t e, const g1_jac& a) { ws.at(e) = a; },
                [&](uint64_t t) { return fropen_own(tw.data(), (size_t)t); });
        }
    }
    for (uint64_t lane = 0; lane < (uint64_t)l.finish_grid * T; lane++)
        p1ntt_finish_run<fp>(
            n2, M, false, l.run, lane, [&](uint64_t e) { return ws.at(e); }, [&](uint64_t slot, const g1_aff& a) { store_aff(&x.at(slot * 96), a); },
            [&](uint64_t slot) { std::memset(&x.at(slot * 96), 0, 96); });
}

extern "C" {
// srs96: n setup images; polys32: k x n coefficient images -> out96 (k x n x 96), status (k).  Returns the polynomials with FK20_ST_REDUCED;
// -1: the plan refuses n.  flags: 2 BITREV, 4 H.  passes_run, if wanted: the passes walked.  h_last_z_zero, if wanted: 1 when entry n - 1
// of EVERY polynomial's inverse transform lies in the workspace as a Jacobian point with Z == 0 - infinity out of the additions themselves.
// forced_tile: mi355_bls_debug_frntt_set_tile's log2 as fk20_run hands it to frntt_sizes_for (0: the plan's own); fr_passes, if wanted: the
// passes of the Fr transform it gave.
int emu_fk20(const uint8_t* srs96, size_t n, const uint8_t* polys32, size_t k, uint32_t flags, size_t forced, uint32_t forced_tile, uint8_t* out96, uint8_t* status,
             size_t* passes_run, int* h_last_z_zero, size_t* fr_passes) {
    const plan::fk20_sizes sz = plan::fk20_sizes_for(n, k, forced);
    if (!sz.ok) return -1;
    const plan::frntt_sizes fsz = plan::frntt_sizes_for(2 * n, sz.per_pass, forced_tile, 0);
    const bool want_h = flags & 4, permute = !want_h && !(flags & 2);
    const uint32_t m = sz.log2n, M = m + 1;
    std::vector<uint8_t> x;
    setup(srs96, n, x);
    const fr w2n = frntt_omega(M);
    const std::vector<uint32_t> tw_fr = fr_twiddles(n, w2n), tw_inv = point_twiddles(n, fr_inv(w2n)), tw_fwd = point_twiddles(n / 2, frntt_omega(m));
    const uint32_t n2w[8] = {(uint32_t)(2 * (uint64_t)n), (uint32_t)((2 * (uint64_t)n) >> 32), 0, 0, 0, 0, 0, 0};
    const fr inv2n = fr_inv(fr_from_words(n2w));
    std::vector<uint32_t> scal(sz.scalars / 4 + 8), polys(k * n * 8 + 8), words(sz.per_pass);
    std::memcpy(polys.data(), polys32, k * n * 32);
    std::vector<g1_jac> ws(sz.ws / (plan::G1_WORDS * 4));
    int reduced = 0, z_zero = 1;
    for (size_t p = 0; p < sz.passes; p++) {
        size_t g0, kc;
        plan::fk20_pass(sz, k, p, g0, kc);
        const plan::fk20_launch l = plan::fk20_launch_for(sz, kc);
        const uint32_t* src = polys.data() + g0 * n * 8;
        uint8_t* out = out96 + g0 * n * 96;
        std::fill(words.begin(), words.end(), 0u);
        for (uint64_t lane = 0; lane < (uint64_t)l.circ_grid * FRNTT_LANES; lane++) {
            uint64_t vec;
            if (fk20_circ_run(m, kc, inv2n, lane, src, scal.data(), vec)) words.at(vec) |= FK20_ST_REDUCED;
        }
        uint32_t done = 0;
        for (uint32_t q = 0; q < fsz.passes; q++) {
            const uint32_t tp = fsz.stages[q], sigma = M - done - tp;
            const plan::frntt_shape sh = plan::frntt_geo_for(M, fsz.tile, sigma, tp, kc);
            fr_pass(frntt_geo{M, sigma, tp, sh.clo, sh.chi, sh.L, kc}, tw_fr.data(), scal.data());
            done += tp;
        }
        const uint64_t total = (uint64_t)kc << M, mask = ((uint64_t)1 << M) - 1;
        for (uint64_t e = 0; e < (uint64_t)l.point_grid * T; e++)
            if (e < total) ws.at(e) = fk20_pointwise<fp>(g1_aff_load(&x.at((e & mask) * 96)), fropen_own(scal.data(), (size_t)e));
        p1ntt_stage g{};
        g.k = kc, g.m = M;
        const auto load = [&](uint64_t e) { return ws.at(e); };
        const auto store = [&](uint64_t e, const g1_jac& a) { ws.at(e) = a; };
        for (uint32_t b = 0; b < M; b++) {
            g.b = b;
            for (uint64_t lane = 0; lane < (uint64_t)l.inv_grid * T; lane++)
                if (lane < p1ntt_lanes(g)) p1ntt_butterfly<true, fp>(g, lane, load, store, [&](uint64_t t) { return fropen_own(tw_inv.data(), (size_t)t); });
        }
        for (size_t v = 0; v < kc; v++) z_zero &= (int)jac_is_inf(ws.at((v << M) + n - 1));
        g.m = m;
        for (uint32_t s = 0; s < m && !want_h; s++) {
            g.b = m - 1 - s;
            for (uint64_t lane = 0; lane < (uint64_t)l.fwd_grid * T; lane++)
                if (lane < p1ntt_lanes(g))
                    p1ntt_butterfly<false, fp>(
                        g, lane, [&](uint64_t e) { return ws.at(fk20_at(m, e)); }, [&](uint64_t e, const g1_jac& a) { ws.at(fk20_at(m, e)) = a; },
                        [&](uint64_t t) { return fropen_own(tw_fwd.data(), (size_t)t); });
        }
        const uint64_t half = (uint64_t)kc << m;
        for (uint64_t lane = 0; lane < (uint64_t)l.finish_grid * T; lane++)
            p1ntt_finish_run<fp>(
                half, m, permute, l.run, lane, [&](uint64_t e) { return ws.at(fk20_at(m, e)); },
                [&](uint64_t slot, const g1_aff& a) {
                    if (slot < half) store_aff(out + slot * 96, a);
                },
                [&](uint64_t slot) {
                    if (slot < half) std::memset(out + slot * 96, 0, 96);
                });
        for (size_t v = 0; v < kc; v++) {
            status[g0 + v] = (uint8_t)words[v];
            reduced += (words[v] & FK20_ST_REDUCED) != 0;
        }
    }
    if (passes_run) *passes_run = sz.passes;
    if (h_last_z_zero) *h_last_z_zero = z_zero;
    if (fr_passes) *fr_passes = fsz.passes;
    return reduced;
}
// the 2n scalars step 1's layout writes for ONE polynomial, before the transform, with inv2n = 1 (Montgomery one): b itself, canonical
void emu_fk20_circ(const uint8_t* poly32, size_t n, uint8_t* out32) {
    const plan::fk20_sizes sz = plan::fk20_sizes_for(n, 1, 0);
    const plan::fk20_launch l = plan::fk20_launch_for(sz, 1);
    std::vector<uint32_t> src(n * 8 + 8), dst(2 * n * 8 + 8);
    std::memcpy(src.data(), poly32, n * 32);
    for (uint64_t lane = 0; lane < (uint64_t)l.circ_grid * FRNTT_LANES; lane++) {
        uint64_t vec;
        fk20_circ_run(sz.log2n, 1, fr_one(), lane, src.data(), dst.data(), vec);
    }
    std::memcpy(out32, dst.data(), 2 * n * 32);
}
// slot u of s^ -> the setup point's number, or -1: infinity
int64_t emu_fk20_setup_src(uint64_t n, uint64_t u) {
    uint64_t j;
    return fk20_setup_src(n, u, j) ? (int64_t)j : -1;
}
uint64_t emu_fk20_at(uint32_t m, uint64_t e) { return fk20_at(m, e); }
}
