// The numbers of csrc/plan.hpp p1ntt_sizes_for / p1ntt_slice / p1ntt_launch_for, and what the stages and the finish of csrc/p1ntt.hpp address
// under them, for tests/test_p1ntt_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <vector>

#include "fp.hpp"
#include "curve.hpp"
#include "p1ntt.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// -> 1 and out[7] = log2n, vecs, slices, twiddles, ws, staging, the slice bound in bytes | 0: refused
int p1ntt_plan_sizes(size_t n, size_t k, size_t forced_vecs, size_t out[7]) {
    const plan::p1ntt_sizes s = plan::p1ntt_sizes_for(n, k, forced_vecs);
    if (!s.ok) return 0;
    out[0] = s.log2n, out[1] = s.vecs, out[2] = s.slices, out[3] = s.twiddles, out[4] = s.ws, out[5] = s.staging, out[6] = plan::P1NTT_SLICE_BYTES;
    return 1;
}
// slice i: out[2] = first, count
int p1ntt_plan_slice(size_t n, size_t k, size_t forced_vecs, size_t i, size_t out[2]) {
    const plan::p1ntt_sizes s = plan::p1ntt_sizes_for(n, k, forced_vecs);
    if (!s.ok || i >= s.slices) return 0;
    plan::p1ntt_slice(s, k, i, out[0], out[1]);
    return 1;
}
// the launches of a slice of `count` vectors: out[3] = stage_grid, run, finish_grid
int p1ntt_plan_launch(size_t n, size_t count, uint32_t out[3]) {
    const plan::p1ntt_sizes s = plan::p1ntt_sizes_for(n, count, 0);
    if (!s.ok) return 0;
    const plan::p1ntt_launch l = plan::p1ntt_launch_for(s, count);
    out[0] = l.stage_grid, out[1] = l.run, out[2] = l.finish_grid;
    return 1;
}
// Walks the element indices every launched lane of every stage and of the finish addresses for a slice of `count` vectors of n points:
// -> 1 when each stage loads and stores every element of [0, count n) exactly once and nothing else, the finish loads each once and
// stores each slot once, and all of them lie inside the workspace (ws bytes / 192) and the staging (staging bytes / 96) of the plan.
int p1ntt_plan_walk(size_t n, size_t count, int permute) {
    const plan::p1ntt_sizes s = plan::p1ntt_sizes_for(n, count, 0);
    if (!s.ok || s.vecs != count) return 0;
    const plan::p1ntt_launch l = plan::p1ntt_launch_for(s, count);
    const uint64_t total = (uint64_t)count << s.log2n, ws_slots = s.ws / (plan::G1_WORDS * 4), io_slots = s.staging / 96;
    if (total > ws_slots || total > io_slots) return 0;
    p1ntt_stage g{};
    g.m = s.log2n, g.k = count;
    for (uint32_t b = 0; b < s.log2n; b++) {
        g.b = b;
        std::vector<uint8_t> seen(total, 0);
        if ((uint64_t)l.stage_grid * plan::WAVE < p1ntt_lanes(g)) return 0;
        for (uint64_t lane = 0; lane < (uint64_t)l.stage_grid * plan::WAVE; lane++) {
            if (lane >= p1ntt_lanes(g)) continue;
            const p1ntt_pair pr = p1ntt_pair_of(g, lane);
            if (pr.i0 >= total || pr.i1 >= total || pr.tw >= n / 2 || seen[pr.i0]++ || seen[pr.i1]++) return 0;
        }
        for (uint64_t e = 0; e < total; e++)
            if (seen[e] != 1) return 0;
    }
    std::vector<uint8_t> loaded(total, 0), stored(total, 0);
    bool bad = false;
    for (uint64_t lane = 0; lane < (uint64_t)l.finish_grid * plan::WAVE; lane++)
        p1ntt_finish_run<fp>(
            total, s.log2n, permute != 0, l.run, lane,
            [&](uint64_t e) {
                if (e >= total) bad = true;
                else loaded[e]++;
                return jac_inf<fp>();
            },
            [&](uint64_t, const g1_aff&) { bad = true; },
            [&](uint64_t slot) {
                if (slot >= total) bad = true;
                else stored[slot]++;
            });
    for (uint64_t e = 0; e < total; e++)
        if (loaded[e] != 2 || stored[e] != 1) bad = true;      // to_affine_run loads a point twice
    return !bad;
}
}
