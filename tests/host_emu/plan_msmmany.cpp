// The launch plan of k MSMs in one pass (csrc/plan.hpp msm_many_for / msm_many_next / msm_many_extents / msm_many_sizes_for) for
// tests/test_msm_many_plan.py and tests/test_gpu_msm_many.py: the product's own functions behind a C interface, 64-bit words out.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <initializer_list>

#include "plan.hpp"
using namespace plan;

namespace {
uint64_t* put(uint64_t* o, const msm_many_sizes& z) {
    for (size_t v : {z.pts_int, z.offs_dev, z.hist, z.chist, z.sorted, z.buckets, z.segout, z.part}) *o++ = v;
    return o;
}
}  // namespace

extern "C" {
enum { MANY_HEAD = 14 + 8 + 8, MANY_ROW = 14 + 8 };
void plan_manymsm_constants(uint64_t o[10]) {
    const uint64_t c[10] = {MSM_MANY_VWIN_MAX, MSM_MANY_BUCKETS_MAX, MSM_MANY_PAIRS_MAX, MSM_WINDOWS_MAX, MSM_TEAM_LANES_MAX, MSM_SEG, MSM_ORD_PER, WAVE, MANY_HEAD, MANY_ROW};
    for (int i = 0; i < 10; i++) o[i] = c[i];
}
// offsets: k + 1 values, or NULL for the shared form.  head: the window plan (14) | shared, n_ref, buckets_per_msm, segs_per_win, nsplit, tail_waves,
// tail_lanes, msms_max | msm_many_sizes_for (8).  rows: up to max_rows passes of MANY_ROW words: single, j0, j1, pair0, pairs, points, nv, total,
// nseg, pair_grid, order_grid, bucket_grid, team, segred_grid | msm_many_extents (8).  Returns the number of passes of the call.
size_t plan_manymsm_call(const size_t* offsets, size_t npoints, size_t k, size_t nbits, uint64_t* head, uint64_t* rows, size_t max_rows) {
    const msm_many_plan P = msm_many_for(k, npoints, offsets == nullptr, nbits);
    const uint32_t* w = &P.W.nwin;
    for (int j = 0; j < 14; j++) *head++ = w[j];
    for (uint64_t v : {(uint64_t)P.shared, (uint64_t)P.n_ref, (uint64_t)P.buckets_per_msm, (uint64_t)P.segs_per_win, (uint64_t)P.nsplit, (uint64_t)P.tail_waves,
                       (uint64_t)P.tail_lanes, (uint64_t)P.msms_max})
        *head++ = v;
    put(head, msm_many_sizes_for(P, offsets, npoints, k));
    size_t count = 0;
    for (size_t j = 0; j < k; count++) {
        const msm_many_pass s = msm_many_next(P, offsets, npoints, k, j);
        if (count < max_rows) {
            uint64_t* o = rows + count * MANY_ROW;
            for (uint64_t v : {(uint64_t)s.single, (uint64_t)s.j0, (uint64_t)s.j1, (uint64_t)s.pair0, (uint64_t)s.pairs, (uint64_t)s.points, (uint64_t)s.nv,
                               (uint64_t)s.total, (uint64_t)s.nseg, (uint64_t)s.pair_grid, (uint64_t)s.order_grid, (uint64_t)s.bucket_grid, (uint64_t)s.team,
                               (uint64_t)s.segred_grid})
                *o++ = v;
            put(o, msm_many_extents(P, s));
        }
        j = s.j1;
    }
    return count;
}
}
