// The launch plan of the fixed-base table MSM (csrc/plan.hpp fixed_win / fixed_wbits_for / fixed_for / fixed_next / fixed_extents /
// fixed_sizes_for) for tests/test_msm_table_plan.py and tests/test_gpu_msm_table.py: the product's own functions behind a C interface, 64-bit
// words out.  Built a second time as a program of its own (-DPLAN_MSMTABLE_MAIN, with sanitizers): main walks the tests' sweep and checks the
// same properties.  TEST INFRASTRUCTURE: never linked into the product library.
#include <cstdio>
#include <initializer_list>

#include "plan.hpp"
using namespace plan;

namespace {
uint64_t* put(uint64_t* o, const fixed_sizes& z) {
    for (size_t v : {z.hist, z.chist, z.sorted, z.buckets, z.segout, z.part, z.out}) *o++ = v;
    return o;
}
}  // namespace

extern "C" {
enum { FIXED_HEAD = 14 + 9 + 7, FIXED_ROW = 12 + 7 };
void plan_fixed_constants(uint64_t o[12]) {
    const uint64_t c[12] = {FIXED_ENTRIES_MAX, FIXED_ENTRY_BYTES, FIXED_PAIRS_MAX, MSM_MANY_VWIN_MAX, MSM_MANY_BUCKETS_MAX, MSM_TEAM_LANES_MAX,
                            MSM_SEG,           MSM_ORD_PER,       WAVE,            FIXED_HEAD,        FIXED_ROW,            FIXED_SCRATCH_BYTES};
    for (int i = 0; i < 12; i++) o[i] = c[i];
}
uint64_t plan_fixed_args_ok(size_t npoints, size_t wbits, size_t nbits) { return fixed_args_ok(npoints, wbits, nbits); }
uint64_t plan_fixed_table_bytes(size_t npoints, size_t wbits, size_t nbits) { return fixed_table_bytes(npoints, wbits, nbits); }
uint64_t plan_fixed_wbits_for(size_t npoints) { return fixed_wbits_for(npoints); }
uint64_t plan_fixed_rows_chunk(size_t npoints, uint32_t nwin) { return fixed_rows_chunk(npoints, nwin); }
// head: the window plan (14) | n, S, buckets_per_msm, segs_per_set, nsplit, tail_waves, tail_lanes, pairs_max, msms_max | fixed_sizes_for (7).
// rows: up to max_rows passes of FIXED_ROW words: j0, j1, pair0, pairs, nv, total, nseg, pair_grid, order_grid, bucket_grid, team, segred_grid |
// fixed_extents (7).  Returns the number of passes of the call.
size_t plan_fixed_call(size_t npoints, size_t wbits, size_t nbits, size_t k, uint32_t slots, uint32_t pairs_max, uint32_t force_S, uint64_t* head, uint64_t* rows,
                       size_t max_rows) {
    const fixed_plan P = fixed_for(npoints, fixed_win(wbits, nbits), k, slots, pairs_max ? pairs_max : FIXED_PAIRS_MAX, force_S);
    const uint32_t* w = &P.W.nwin;
    for (int j = 0; j < 14; j++) *head++ = w[j];
    for (uint64_t v : {(uint64_t)P.n, (uint64_t)P.S, (uint64_t)P.buckets_per_msm, (uint64_t)P.segs_per_set, (uint64_t)P.nsplit, (uint64_t)P.tail_waves,
                       (uint64_t)P.tail_lanes, (uint64_t)P.pairs_max, (uint64_t)P.msms_max})
        *head++ = v;
    put(head, fixed_sizes_for(P, k));
    size_t count = 0;
    for (size_t j = 0; j < k; count++) {
        const fixed_pass s = fixed_next(P, k, j);
        if (count < max_rows) {
            uint64_t* o = rows + count * FIXED_ROW;
            for (uint64_t v : {(uint64_t)s.j0, (uint64_t)s.j1, (uint64_t)s.pair0, (uint64_t)s.pairs, (uint64_t)s.nv, (uint64_t)s.total, (uint64_t)s.nseg,
                               (uint64_t)s.pair_grid, (uint64_t)s.order_grid, (uint64_t)s.bucket_grid, (uint64_t)s.team, (uint64_t)s.segred_grid})
                *o++ = v;
            put(o, fixed_extents(P, s));
        }
        j = s.j1;
    }
    return count;
}
}

#if defined(PLAN_MSMTABLE_MAIN)
#define NEED(cond)                                                                                                                   \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            std::printf("FAILED %s (npoints %zu wbits %zu nbits %zu k %zu)\n", #cond, npoints, wbits, nbits, k);                      \
            return 1;                                                                                                                \
        }                                                                                                                            \
    } while (0)
int main() {
    size_t cases = 0;
    for (size_t wbits = 5; wbits <= 16; wbits++)
        for (size_t nbits : {(size_t)1, (size_t)5, (size_t)64, (size_t)255, (size_t)256}) {
            const size_t Wn = (nbits + 1 + wbits - 1) / wbits, bound = (size_t)(FIXED_ENTRIES_MAX / Wn);
            for (size_t npoints : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)4096, (size_t)1 << 16, (size_t)1 << 20, bound, bound + 1})
                for (size_t k : {(size_t)1, (size_t)2, (size_t)9, (size_t)64, (size_t)512}) {
                    const bool ok = fixed_args_ok(npoints, wbits, nbits);
                    NEED(ok == (npoints <= bound));
                    NEED(fixed_table_bytes(npoints, wbits, nbits) == (ok ? Wn * npoints * 128 : 0));
                    if (!ok) continue;
                    const pip_win W = fixed_win(wbits, nbits);
                    NEED(W.nwin == Wn && W.wrem == 0 && W.wbase == wbits && W.cbk == wbits - 1);
                    const fixed_plan P = fixed_for(npoints, W, k, 1024);
                    NEED(P.S >= 1 && P.S <= W.nwin && P.msms_max >= 1);
                    const fixed_sizes m = fixed_sizes_for(P, k);
                    size_t at = 0;
                    while (at < k) {
                        const fixed_pass s = fixed_next(P, k, at);
                        NEED(s.j0 == at && s.j1 > at && s.j1 <= k && s.pair0 == at * npoints);
                        NEED((size_t)s.pairs == (s.j1 - s.j0) * npoints && (uint64_t)s.pairs * W.nwin <= FIXED_ENTRIES_MAX);
                        NEED(s.total <= MSM_MANY_BUCKETS_MAX && s.nv <= MSM_MANY_VWIN_MAX);
                        const fixed_sizes z = fixed_extents(P, s);
                        NEED(z.hist <= m.hist && z.chist <= m.chist && z.sorted <= m.sorted && z.buckets <= m.buckets && z.segout <= m.segout && z.part <= m.part &&
                             z.out <= m.out);
                        at = s.j1;
                    }
                    cases++;
                }
        }
    std::printf("plan_msmtable: %zu cases\n", cases);
    return 0;
}
#endif
