// The numbers of csrc/plan.hpp fk20_sizes_for / fk20_pass / fk20_launch_for, and what the kernels of csrc/fk20.hpp address under them, for
// tests/test_fk20_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "fk20.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// -> 1 and out[12] = log2n, per_pass, passes, ws, scalars, polys, out, status, tw_fr, tw_inv, tw_fwd, the pass bound in bytes | 0: refused
int fk20_plan_sizes(size_t n, size_t k, size_t forced, size_t out[12]) {
    const plan::fk20_sizes s = plan::fk20_sizes_for(n, k, forced);
    if (!s.ok) return 0;
    out[0] = s.log2n, out[1] = s.per_pass, out[2] = s.passes, out[3] = s.ws, out[4] = s.scalars, out[5] = s.polys, out[6] = s.out, out[7] = s.status;
    out[8] = s.tw_fr, out[9] = s.tw_inv, out[10] = s.tw_fwd, out[11] = plan::FK20_PASS_BYTES;
    return 1;
}
size_t fk20_plan_setup_bytes(size_t n) { return plan::fk20_setup_bytes(n); }
// pass p: out[2] = first, count
int fk20_plan_pass(size_t n, size_t k, size_t forced, size_t p, size_t out[2]) {
    const plan::fk20_sizes s = plan::fk20_sizes_for(n, k, forced);
    if (!s.ok || p >= s.passes) return 0;
    plan::fk20_pass(s, k, p, out[0], out[1]);
    return 1;
}
// the launches of a pass of `count` polynomials: out[6] = circ_grid, point_grid, inv_grid, fwd_grid, run, finish_grid
int fk20_plan_launch(size_t n, size_t count, uint32_t out[6]) {
    const plan::fk20_sizes s = plan::fk20_sizes_for(n, count, 0);
    if (!s.ok) return 0;
    const plan::fk20_launch l = plan::fk20_launch_for(s, count);
    out[0] = l.circ_grid, out[1] = l.point_grid, out[2] = l.inv_grid, out[3] = l.fwd_grid, out[4] = l.run, out[5] = l.finish_grid;
    return 1;
}
// Walks what every launched lane addresses for a pass of `count` polynomials of n coefficients: -> 1 when the layout reads every coefficient
// once and writes every scalar slot once, the pointwise grid covers count x 2n, each inverse stage pairs every element of the count x 2n
// workspace once, each forward stage every element of the first halves once and none of the second halves, the finish loads the first
// halves and stores each output slot once, and everything lies inside the plan's buffers.
int fk20_plan_walk(size_t n, size_t count, int permute) {
    const plan::fk20_sizes s = plan::fk20_sizes_for(n, count, 0);
    if (!s.ok || s.per_pass != count) return 0;
    const plan::fk20_launch l = plan::fk20_launch_for(s, count);
    const uint32_t m = s.log2n, M = m + 1;
    const uint64_t half = (uint64_t)count << m, total = half << 1;
    if (total > s.ws / (plan::G1_WORDS * 4) || total > s.scalars / 32 || half > s.polys / 32 || half > s.out / 96 || count > s.status / 4) return 0;
    {   // the layout, through its index rule
        std::vector<uint8_t> rd(half, 0), wr(total, 0);
        const uint64_t n2 = 2 * (uint64_t)n, per_vec = (n2 + FRNTT_RUN - 1) / FRNTT_RUN;
        if ((uint64_t)l.circ_grid * FRNTT_LANES < count * per_vec) return 0;
        for (uint64_t run = 0; run < (uint64_t)l.circ_grid * FRNTT_LANES; run++) {
            const uint64_t vec = run / per_vec;
            if (vec >= count) continue;
            const uint64_t lo = (run % per_vec) * FRNTT_RUN, hi = n2 - lo < FRNTT_RUN ? n2 : lo + FRNTT_RUN;
            for (uint64_t t = lo; t < hi; t++) {
                uint64_t j;
                if (fk20_circ_src(n, t, j)) {
                    if (j >= n || rd[vec * n + j]++) return 0;
                }
                if (wr[vec * n2 + t]++) return 0;
            }
        }
        for (uint64_t e = 0; e < half; e++)
            if (rd[e] != 1) return 0;
        for (uint64_t e = 0; e < total; e++)
            if (wr[e] != 1) return 0;
    }
    if ((uint64_t)l.point_grid * plan::WAVE < total) return 0;
    p1ntt_stage g{};
    g.k = count, g.m = M;
    for (uint32_t b = 0; b < M; b++) {
        g.b = b;
        std::vector<uint8_t> seen(total, 0);
        if ((uint64_t)l.inv_grid * plan::WAVE < p1ntt_lanes(g)) return 0;
        for (uint64_t lane = 0; lane < p1ntt_lanes(g); lane++) {
            const p1ntt_pair pr = p1ntt_pair_of(g, lane);
            if (pr.i0 >= total || pr.i1 >= total || pr.tw >= n || seen[pr.i0]++ || seen[pr.i1]++) return 0;
        }
        for (uint64_t e = 0; e < total; e++)
            if (seen[e] != 1) return 0;
    }
    g.m = m;
    for (uint32_t b = 0; b < m; b++) {
        g.b = b;
        std::vector<uint8_t> seen(total, 0);
        if ((uint64_t)l.fwd_grid * plan::WAVE < p1ntt_lanes(g)) return 0;
        for (uint64_t lane = 0; lane < p1ntt_lanes(g); lane++) {
            const p1ntt_pair pr = p1ntt_pair_of(g, lane);
            const uint64_t a0 = fk20_at(m, pr.i0), a1 = fk20_at(m, pr.i1);
            if (a0 >= total || a1 >= total || pr.tw >= n / 2 || seen[a0]++ || seen[a1]++) return 0;
        }
        for (uint64_t e = 0; e < total; e++)
            if (seen[e] != ((e >> m) & 1 ? 0 : 1)) return 0;
    }
    std::vector<uint8_t> loaded(total, 0), stored(half, 0);
    bool bad = false;
    for (uint64_t lane = 0; lane < (uint64_t)l.finish_grid * plan::WAVE; lane++)
        p1ntt_finish_run<fp>(
            half, m, permute != 0, l.run, lane,
            [&](uint64_t e) {
                const uint64_t a = fk20_at(m, e);
                if (a >= total) bad = true;
                else loaded[a]++;
                return jac_inf<fp>();
            },
            [&](uint64_t, const g1_aff&) { bad = true; },
            [&](uint64_t slot) {
                if (slot >= half) bad = true;
                else stored[slot]++;
            });
    for (uint64_t e = 0; e < total; e++)
        if (loaded[e] != ((e >> m) & 1 ? 0 : 2)) bad = true;      // to_affine_run loads a point twice
    for (uint64_t e = 0; e < half; e++)
        if (stored[e] != 1) bad = true;
    return !bad;
}
}
