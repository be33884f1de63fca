// CPU execution of the cell-proof call (csrc/fk20cells.hpp lane bodies with those of csrc/fk20.hpp, csrc/frntt.hpp and csrc/p1ntt.hpp they run
// between, lane by lane as csrc/kernels.hip k_fk20c_* / k_frntt_pass / k_p1ntt_stage walk them, in the order and with the launch shapes
// csrc/host_api.inc mi355_bls_fk20_setup_create_cells_device and fk20_cells_run use) for tests/test_fk20_cells_emu.py, bounds tracked like
// tests/host_emu/fk20.cpp.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "fk20cells.hpp"
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
// p1ntt_run's forward BITREV walk over `vecs` vectors of n2 points, in place in x (vecs x n2 x 96)
static void point_forward(std::vector<uint8_t>& x, size_t n2, size_t vecs) {
    const plan::p1ntt_sizes sz = plan::p1ntt_sizes_for(n2, vecs, 0);
    const uint32_t M = sz.log2n;
    const std::vector<uint32_t> tw = point_twiddles(n2 / 2, frntt_omega(M));
    for (size_t i = 0; i < sz.slices; i++) {
        size_t v0, vc;
        plan::p1ntt_slice(sz, vecs, i, v0, vc);
        const plan::p1ntt_launch l = plan::p1ntt_launch_for(sz, vc);
        uint8_t* io = &x.at(v0 * n2 * 96);
        const uint64_t total = (uint64_t)vc * n2;
        std::vector<g1_jac> ws(total);
        p1ntt_stage g{};
        g.m = M, g.k = vc;
        for (uint32_t s = 0; s < M; s++) {
            g.b = M - 1 - s;
            const bool first = s == 0;
            for (uint64_t lane = 0; lane < (uint64_t)l.stage_grid * T; lane++) {
                if (lane >= p1ntt_lanes(g)) continue;
                p1ntt_butterfly<false, fp>(
                    g, lane, [&](uint64_t e) { return first ? (e < total ? jac_from_aff(g1_aff_load(io + e * 96)) : ws.at(total)) : ws.at(e); },
                    [&](uint64_t e, const g1_jac& a) { ws.at(e) = a; }, [&](uint64_t t) { return fropen_own(tw.data(), (size_t)t); });
            }
        }
        for (uint64_t lane = 0; lane < (uint64_t)l.finish_grid * T; lane++)
            p1ntt_finish_run<fp>(
                total, M, false, l.run, lane, [&](uint64_t e) { return ws.at(e); },
                [&](uint64_t slot, const g1_aff& a) {
                    ws.at(slot);
                    store_aff(io + slot * 96, a);
                },
                [&](uint64_t slot) {
                    ws.at(slot);
                    std::memset(io + slot * 96, 0, 96);
                });
    }
}
// mi355_bls_fk20_setup_create_cells_device: -> x (2n x 96), the handle's contents
static void setup_cells(const uint8_t* srs96, size_t n, const plan::fk20_cells_sizes& sz, std::vector<uint8_t>& x) {
    const size_t n2 = 2 * n, cell = (size_t)1 << sz.log2cell;
    const uint32_t mq = sz.log2q, c = sz.log2cell;
    const uint64_t grid = (n2 + FRNTT_LANES - 1) / FRNTT_LANES;
    std::vector<uint8_t> tmp(n2 * 96, 0);
    for (uint64_t t = 0; t < grid * FRNTT_LANES; t++) {
        if (t >= n2) continue;
        uint64_t i;
        if (fk20c_setup_src(mq, c, t, i)) {
            if (i >= n) tmp.at(n2 * 96);                    // out of the caller's array: stop here
            std::memcpy(&tmp.at(t * 96), srs96 + i * 96, 96);
        }
    }
    point_forward(tmp, n2 / cell, cell);
    if (cell == 1) {                                        // fk20_setup_create's own path: no placing
        x = tmp;
        return;
    }
    x.assign(n2 * 96, 0xee);
    for (uint64_t t = 0; t < grid * FRNTT_LANES; t++)
        if (t < n2) std::memcpy(&x.at(fk20c_setup_at(mq, c, t) * 96), &tmp.at(t * 96), 96);
}
// fk20.cpp's setup, as mi355_bls_fk20_setup_create_device lays it out: the handle the cell == 1 one must equal
static void setup_plain(const uint8_t* srs96, size_t n, std::vector<uint8_t>& x) {
    x.assign(2 * n * 96, 0);
    for (uint64_t u = 0; u < 2 * n; u++) {
        uint64_t j;
        if (fk20_setup_src(n, u, j)) std::memcpy(&x.at(u * 96), srs96 + j * 96, 96);
    }
    point_forward(x, 2 * n, 1);
}

extern "C" {
// the handle's contents for (srs96, n, cell) -> out (2n x 96); plain != 0: fk20_setup_create's.  -1: refused
int emu_fk20c_setup(const uint8_t* srs96, size_t n, size_t cell, int plain, uint8_t* out) {
    const plan::fk20_cells_sizes sz = plan::fk20_cells_sizes_for(n, cell, 0, 1);
    if (!sz.ok) return -1;
    std::vector<uint8_t> x;
    if (plain) setup_plain(srs96, n, x);
    else setup_cells(srs96, n, sz, x);
    std::memcpy(out, x.data(), x.size());
    return 0;
}
// srs96: n setup images; polys32: k x n coefficient images -> out96 (k x N x 96, with H k x q x 96), status (k).  Returns the polynomials
// with FK20_ST_REDUCED; -1: the plan refuses.  flags: 2 BITREV, 4 H.  passes_run, if wanted: the passes walked.  The workspace and the
// product array are filled with a pattern that is no point of the curve before every pass: an image read before it is written shows.
// forced_tile: mi355_bls_debug_frntt_set_tile's log2 as fk20_cells_run hands it to frntt_sizes_for (0: the plan's own); fr_passes, if wanted:
// the passes of the Fr transform it gave.
int emu_fk20c(const uint8_t* srs96, size_t n, size_t cell, size_t ext, const uint8_t* polys32, size_t k, uint32_t flags, size_t forced, uint32_t forced_tile, uint8_t* out96,
              uint8_t* status, size_t* passes_run, size_t* fr_passes) {
    const plan::fk20_cells_sizes sz = plan::fk20_cells_sizes_for(n, cell, ext, k, forced);
    if (!sz.ok) return -1;
    const uint32_t mq = sz.log2q, cl = sz.log2cell, M = mq + 1, a = sz.log2cells, w = sz.log2w;
    const size_t q = (size_t)1 << mq, cells = (size_t)1 << a;
    const plan::frntt_sizes fsz = plan::frntt_sizes_for(2 * q, sz.per_pass << cl, forced_tile, 0);
    const bool want_h = flags & 4, permute = !want_h && !(flags & 2);
    const size_t rows = want_h ? q : cells;
    std::vector<uint8_t> x;
    setup_cells(srs96, n, plan::fk20_cells_sizes_for(n, cell, 0, 1), x);
    const fr w2q = frntt_omega(M);
    const std::vector<uint32_t> tw_fr = fr_twiddles(q, w2q), tw_inv = point_twiddles(q, fr_inv(w2q)), tw_fwd = point_twiddles(cells / 2, frntt_omega(a));
    const uint32_t q2w[8] = {(uint32_t)(2 * (uint64_t)q), (uint32_t)((2 * (uint64_t)q) >> 32), 0, 0, 0, 0, 0, 0};
    const fr inv2q = fr_inv(fr_from_words(q2w));
    std::vector<uint32_t> scal(sz.scalars / 4 + 8), polys(k * n * 8 + 8), words(sz.per_pass);
    std::memcpy(polys.data(), polys32, k * n * 32);
    std::vector<g1_jac> ws(sz.ws / (plan::G1_WORDS * 4)), prod(sz.prod / (plan::G1_WORDS * 4));
    g1_jac junk;
    std::memset(&junk, 0x5a, sizeof junk);
    const uint32_t levels = plan::fk20_cells_sum_levels(sz);
    int reduced = 0;
    for (size_t p = 0; p < sz.passes; p++) {
        size_t g0, kc;
        plan::fk20_cells_pass(sz, k, p, g0, kc);
        const plan::fk20_cells_launch l = plan::fk20_cells_launch_for(sz, kc);
        const uint32_t* src = polys.data() + g0 * n * 8;
        uint8_t* out = out96 + g0 * rows * 96;
        std::fill(words.begin(), words.end(), 0u);
        std::fill(ws.begin(), ws.end(), junk);
        std::fill(prod.begin(), prod.end(), junk);
        for (uint64_t lane = 0; lane < (uint64_t)l.circ_grid * FRNTT_LANES; lane++) {
            uint64_t poly;
            if (fk20c_circ_run(mq, cl, kc, inv2q, lane, src, scal.data(), poly)) words.at(poly) |= FK20_ST_REDUCED;
        }
        const size_t vecs = kc << cl;
        uint32_t done = 0;
        for (uint32_t i = 0; i < fsz.passes; i++) {
            const uint32_t tp = fsz.stages[i], sigma = M - done - tp;
            const plan::frntt_shape sh = plan::frntt_geo_for(M, fsz.tile, sigma, tp, vecs);
            fr_pass(frntt_geo{M, sigma, tp, sh.clo, sh.chi, sh.L, vecs}, tw_fr.data(), scal.data());
            done += tp;
        }
        const uint64_t terms = (uint64_t)kc << (sz.log2n + 1);
        for (uint64_t e = 0; e < (uint64_t)l.point_grid * T; e++) {
            if (e >= terms) continue;
            const fk20c_term_at t = fk20c_term(mq, cl, e);
            if (t.scalar >= terms) scal.at(scal.size());
            prod.at(e) = fk20_pointwise<fp>(g1_aff_load(&x.at(t.setup * 96)), fropen_own(scal.data(), (size_t)t.scalar));
        }
        for (uint32_t t = 0; t < levels; t++) {
            const uint64_t lanes = plan::fk20_cells_sum_lanes(sz, kc, t);
            const uint32_t shift = t * FK20C_FAN_LOG2, bits = fk20c_level_bits(cl, t);
            const bool last = t + 1 == levels;
            for (uint64_t o = 0; o < (lanes + T - 1) / T * T; o++) {
                if (o >= lanes) continue;
                const uint64_t first = o << (shift + bits);
                const g1_jac r = fk20c_sum_item<fp>(first, (uint64_t)1 << shift, 1u << bits, [&](uint64_t j) { return prod.at(j); });
                if (last) ws.at(fk20c_at(M, w, o)) = r;
                else prod.at(first) = r;
            }
        }
        p1ntt_stage g{};
        g.k = kc, g.m = M;
        for (uint32_t b = 0; b < M; b++) {
            g.b = b;
            for (uint64_t lane = 0; lane < (uint64_t)l.inv_grid * T; lane++)
                if (lane < p1ntt_lanes(g))
                    p1ntt_butterfly<true, fp>(
                        g, lane, [&](uint64_t e) { return ws.at(fk20c_at(M, w, e)); }, [&](uint64_t e, const g1_jac& pt) { ws.at(fk20c_at(M, w, e)) = pt; },
                        [&](uint64_t t) { return fropen_own(tw_inv.data(), (size_t)t); });
        }
        if (!want_h) {
            for (uint64_t e = 0; e < (uint64_t)l.pad_grid * T; e++)
                if (e < ((uint64_t)kc << a) && fk20c_pad(mq, a, e)) ws.at(fk20c_at(a, w, e)) = jac_inf<fp>();
            g.m = a;
            for (uint32_t s = 0; s < a; s++) {
                g.b = a - 1 - s;
                for (uint64_t lane = 0; lane < (uint64_t)l.fwd_grid * T; lane++)
                    if (lane < p1ntt_lanes(g))
                        p1ntt_butterfly<false, fp>(
                            g, lane, [&](uint64_t e) { return ws.at(fk20c_at(a, w, e)); }, [&](uint64_t e, const g1_jac& pt) { ws.at(fk20c_at(a, w, e)) = pt; },
                            [&](uint64_t t) { return fropen_own(tw_fwd.data(), (size_t)t); });
            }
        }
        const uint32_t fa = want_h ? mq : a;
        const uint64_t total = (uint64_t)kc << fa;
        for (uint64_t lane = 0; lane < (uint64_t)(want_h ? l.finish_h_grid : l.finish_grid) * T; lane++)
            p1ntt_finish_run<fp>(
                total, fa, permute, want_h ? l.run_h : l.run, lane, [&](uint64_t e) { return ws.at(fk20c_at(fa, w, e)); },
                [&](uint64_t slot, const g1_aff& pt) {
                    if (slot >= total) ws.at(ws.size());
                    store_aff(out + slot * 96, pt);
                },
                [&](uint64_t slot) {
                    if (slot >= total) ws.at(ws.size());
                    std::memset(out + slot * 96, 0, 96);
                });
        for (size_t v = 0; v < kc; v++) {
            status[g0 + v] = (uint8_t)words[v];
            reduced += (words[v] & FK20_ST_REDUCED) != 0;
        }
    }
    if (passes_run) *passes_run = sz.passes;
    if (fr_passes) *fr_passes = fsz.passes;
    return reduced;
}
}
