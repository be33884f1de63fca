// The numbers of csrc/plan.hpp fk20_cells_sizes_for / fk20_cells_pass / fk20_cells_launch_for, and what the kernels of csrc/fk20cells.hpp
// address under them, for tests/test_fk20_cells_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "fk20cells.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// -> 1 and out[17] = log2n, log2cell, log2q, log2cells, log2w, per_pass, passes, scalars, prod, ws, polys, out, status, tw_fr, tw_inv, tw_fwd,
// the pass bound in bytes | 0: refused
int fk20c_plan_sizes(size_t n, size_t cell, size_t ext, size_t k, size_t forced, size_t out[17]) {
    const plan::fk20_cells_sizes s = plan::fk20_cells_sizes_for(n, cell, ext, k, forced);
    if (!s.ok) return 0;
    out[0] = s.log2n, out[1] = s.log2cell, out[2] = s.log2q, out[3] = s.log2cells, out[4] = s.log2w, out[5] = s.per_pass, out[6] = s.passes;
    out[7] = s.scalars, out[8] = s.prod, out[9] = s.ws, out[10] = s.polys, out[11] = s.out, out[12] = s.status;
    out[13] = s.tw_fr, out[14] = s.tw_inv, out[15] = s.tw_fwd, out[16] = plan::FK20_PASS_BYTES;
    return 1;
}
// pass p: out[2] = first, count
int fk20c_plan_pass(size_t n, size_t cell, size_t ext, size_t k, size_t forced, size_t p, size_t out[2]) {
    const plan::fk20_cells_sizes s = plan::fk20_cells_sizes_for(n, cell, ext, k, forced);
    if (!s.ok || p >= s.passes) return 0;
    plan::fk20_cells_pass(s, k, p, out[0], out[1]);
    return 1;
}
// the launches of a pass of `count` polynomials: out[9] = circ_grid, point_grid, inv_grid, pad_grid, fwd_grid, run, finish_grid, run_h,
// finish_h_grid; levels: the sum's levels, lanes[t] those of level t (room for 11)
int fk20c_plan_launch(size_t n, size_t cell, size_t ext, size_t count, uint32_t out[9], uint32_t* levels, uint64_t lanes[11]) {
    const plan::fk20_cells_sizes s = plan::fk20_cells_sizes_for(n, cell, ext, count, 0);
    if (!s.ok) return 0;
    const plan::fk20_cells_launch l = plan::fk20_cells_launch_for(s, count);
    out[0] = l.circ_grid, out[1] = l.point_grid, out[2] = l.inv_grid, out[3] = l.pad_grid, out[4] = l.fwd_grid, out[5] = l.run, out[6] = l.finish_grid;
    out[7] = l.run_h, out[8] = l.finish_h_grid;
    *levels = plan::fk20_cells_sum_levels(s);
    for (uint32_t t = 0; t < *levels && t < 11; t++) lanes[t] = plan::fk20_cells_sum_lanes(s, count, t);
    return 1;
}
// Walks what every launched lane addresses for a pass of `count` polynomials: -> 1 when the setup's layout reads every setup point but
// the last of each sub-setup once and its placing is a permutation of the 2n images; the call's layout reads every coefficient once and
// writes every scalar slot once; the product lanes read every scalar and write every product image once, and the l terms of a slot take
// the l images of that slot of the handle; the levels of the sum read every product once, write only first images of their groups and at
// last every slot of the count x 2q workspace places once; each inverse stage pairs those places once; the padding writes exactly entries
// q .. N-1; each forward stage pairs every one of the count x N places once; the finish (h != 0: the H form's) loads each of its places and
// stores each output slot once; and everything lies inside the plan's buffers.  want: a nonzero return is 1.
int fk20c_plan_walk(size_t n, size_t cell, size_t ext, size_t count, int permute, int h) {
    const plan::fk20_cells_sizes s = plan::fk20_cells_sizes_for(n, cell, ext, count, 0);
    if (!s.ok || s.per_pass != count) return 0;
    const plan::fk20_cells_launch l = plan::fk20_cells_launch_for(s, count);
    const uint32_t mq = s.log2q, c = s.log2cell, M = mq + 1, a = s.log2cells, w = s.log2w;
    const uint64_t q = (uint64_t)1 << mq, q2 = 2 * q, n2 = 2 * (uint64_t)n, big = (uint64_t)1 << a;
    const uint64_t terms = count * n2, slots = count * q2, places = (uint64_t)count << w, coeffs = count * (uint64_t)n, cells = count * big;
    if (places != s.ws / (plan::G1_WORDS * 4) || terms != s.prod / (plan::G1_WORDS * 4) || terms != s.scalars / 32 || coeffs != s.polys / 32 || cells != s.out / 96 ||
        count != s.status / 4 || q * 32 != s.tw_fr || q * 32 != s.tw_inv || big / 2 * 32 != s.tw_fwd || plan::fk20_setup_bytes(n) != n2 * 96)
        return 0;
    {   // the setup
        std::vector<uint8_t> rd(n, 0), at(n2, 0);
        for (uint64_t t = 0; t < n2; t++) {
            uint64_t i;
            if (fk20c_setup_src(mq, c, t, i)) {
                if (i >= n || rd[i]++) return 0;
                if ((i & (cell - 1)) != t / q2) return 0;                   // vector v holds the points l u + v
            }
            const uint64_t p = fk20c_setup_at(mq, c, t);
            if (p >= n2 || at[p]++) return 0;
            if (p != (t % q2) * cell + t / q2) return 0;
        }
        for (uint64_t i = 0; i < n; i++)
            if (rd[i] != (i / cell == q - 1 ? 0 : 1)) return 0;             // S^(v)_(q-1) takes no part
    }
    {   // the layout
        std::vector<uint8_t> rd(coeffs, 0), wr(terms, 0);
        const uint64_t per_vec = (q2 + FRNTT_RUN - 1) / FRNTT_RUN;
        if ((uint64_t)l.circ_grid * FRNTT_LANES < count * cell * per_vec) return 0;
        for (uint64_t run = 0; run < (uint64_t)l.circ_grid * FRNTT_LANES; run++) {
            const uint64_t vec = run / per_vec, poly = vec >> c, v = vec & (cell - 1);
            if (poly >= count) continue;
            const uint64_t lo = (run % per_vec) * FRNTT_RUN, hi = q2 - lo < FRNTT_RUN ? q2 : lo + FRNTT_RUN;
            for (uint64_t t = lo; t < hi; t++) {
                uint64_t j;
                if (fk20_circ_src(q, t, j)) {
                    const uint64_t e = poly * n + j * cell + v;
                    if (j >= q || e >= coeffs || rd[e]++) return 0;
                }
                if (vec * q2 + t >= terms || wr[vec * q2 + t]++) return 0;
            }
        }
        for (uint64_t e = 0; e < coeffs; e++)
            if (rd[e] != 1) return 0;
        for (uint64_t e = 0; e < terms; e++)
            if (wr[e] != 1) return 0;
    }
    {   // the products
        if ((uint64_t)l.point_grid * plan::WAVE < terms) return 0;
        std::vector<uint8_t> sc(terms, 0);
        for (uint64_t e = 0; e < terms; e++) {
            const fk20c_term_at t = fk20c_term(mq, c, e);
            const uint64_t v = e % cell, slot = e / cell % q2, g = e / cell / q2;
            if (t.scalar >= terms || sc[t.scalar]++ || t.scalar != (g * cell + v) * q2 + slot || t.setup != slot * cell + v || t.setup >= n2) return 0;
        }
    }
    std::vector<uint8_t> ws(places, 0);
    {   // the sum
        std::vector<uint8_t> live(terms, 1);                                    // a product or a partial that no level has consumed yet
        const uint32_t levels = plan::fk20_cells_sum_levels(s);
        uint32_t bits_done = 0;
        for (uint32_t t = 0; t < levels; t++) {
            const uint64_t lanes = plan::fk20_cells_sum_lanes(s, count, t);
            const uint32_t shift = t * FK20C_FAN_LOG2, bits = fk20c_level_bits(c, t);
            if (shift != bits_done || bits > FK20C_FAN_LOG2 || (c && bits == 0)) return 0;
            const bool last = t + 1 == levels;
            for (uint64_t o = 0; o < lanes; o++) {
                const uint64_t first = o << (shift + bits);
                for (uint64_t j = 0; j < ((uint64_t)1 << bits); j++) {
                    const uint64_t e = first + (j << shift);
                    if (e >= terms || !live[e]) return 0;
                    live[e] = 0;
                }
                if (last) {
                    const uint64_t p = fk20c_at(M, w, o);
                    if (o >= slots || p >= places || ws[p]++) return 0;
                } else {
                    live[first] = 1;
                }
            }
            bits_done += bits;
        }
        if (bits_done != c) return 0;
        for (uint64_t e = 0; e < terms; e++)
            if (live[e]) return 0;
        for (uint64_t o = 0; o < slots; o++)
            if (ws[fk20c_at(M, w, o)] != 1) return 0;
    }
    p1ntt_stage g{};
    g.k = count, g.m = M;
    for (uint32_t b = 0; b < M; b++) {
        g.b = b;
        std::vector<uint8_t> seen(places, 0);
        if ((uint64_t)l.inv_grid * plan::WAVE < p1ntt_lanes(g)) return 0;
        for (uint64_t lane = 0; lane < p1ntt_lanes(g); lane++) {
            const p1ntt_pair pr = p1ntt_pair_of(g, lane);
            const uint64_t a0 = fk20c_at(M, w, pr.i0), a1 = fk20c_at(M, w, pr.i1);
            if (a0 >= places || a1 >= places || pr.tw >= q || seen[a0]++ || seen[a1]++) return 0;
        }
        for (uint64_t e = 0; e < places; e++)
            if (seen[e] != ws[e]) return 0;                                     // exactly the places the sum wrote
    }
    if (!h) {
        if (a > mq) {
            if ((uint64_t)l.pad_grid * plan::WAVE < cells) return 0;
            for (uint64_t e = 0; e < cells; e++)
                if (fk20c_pad(mq, a, e)) {
                    const uint64_t p = fk20c_at(a, w, e);
                    if (p >= places || (e % big) < q) return 0;
                    ws[p] = 1;
                }
        } else if (l.pad_grid) {
            return 0;
        }
        g.m = a;
        for (uint32_t b = 0; b < a; b++) {
            g.b = b;
            std::vector<uint8_t> seen(places, 0);
            if ((uint64_t)l.fwd_grid * plan::WAVE < p1ntt_lanes(g)) return 0;
            for (uint64_t lane = 0; lane < p1ntt_lanes(g); lane++) {
                const p1ntt_pair pr = p1ntt_pair_of(g, lane);
                const uint64_t a0 = fk20c_at(a, w, pr.i0), a1 = fk20c_at(a, w, pr.i1);
                if (a0 >= places || a1 >= places || pr.tw >= big / 2 || seen[a0]++ || seen[a1]++ || !ws[a0] || !ws[a1]) return 0;
            }
            for (uint64_t e = 0; e < places; e++)
                if (seen[e] != ((e & (((uint64_t)1 << w) - 1)) < big ? 1 : 0)) return 0;
        }
    }
    const uint32_t fa = h ? mq : a;
    const uint64_t total = (uint64_t)count << fa;
    std::vector<uint8_t> loaded(places, 0), stored(total, 0);
    bool bad = false;
    for (uint64_t lane = 0; lane < (uint64_t)(h ? l.finish_h_grid : l.finish_grid) * plan::WAVE; lane++)
        p1ntt_finish_run<fp>(
            total, fa, permute != 0 && !h, h ? l.run_h : l.run, lane,
            [&](uint64_t e) {
                const uint64_t p = fk20c_at(fa, w, e);
                if (p >= places || !ws[p]) bad = true;
                else loaded[p]++;
                return jac_inf<fp>();
            },
            [&](uint64_t, const g1_aff&) { bad = true; },
            [&](uint64_t slot) {
                if (slot >= total) bad = true;
                else stored[slot]++;
            });
    for (uint64_t e = 0; e < places; e++)
        if (loaded[e] != ((e & (((uint64_t)1 << w) - 1)) < ((uint64_t)1 << fa) ? 2 : 0)) bad = true;      // to_affine_run loads a point twice
    for (uint64_t e = 0; e < total; e++)
        if (stored[e] != 1) bad = true;
    return !bad;
}
}
