// The launch plan of k MSMs in one pass with its G2 flag (csrc/plan.hpp msm_many_for / msm_many_next / msm_many_extents / msm_many_sizes_for)
// and of the Jacobian-to-affine calls (to_affine_for / to_affine_next) for tests/test_msm_many_g2_plan.py, tests/test_gpu_msm_many_g2.py and
// tests/test_gpu_to_affine.py: the product's own functions behind a C interface, 64-bit words out.  With -DPLAN_MSMMANY_G2_MAIN a program of
// its own that walks the same plans over a sweep and checks them itself: what the sanitized build runs.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstdio>
#include <initializer_list>
#include <vector>

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
void plan_manymsm_g2_constants(uint64_t o[12]) {
    const uint64_t c[12] = {MSM_MANY_VWIN_MAX, MSM_MANY_BUCKETS_MAX, MSM_MANY_PAIRS_MAX, MSM_WINDOWS_MAX, MSM_MANY_G2_BUCKETS_MAX, MSM_MANY_G2_TAIL_WAVES,
                            G1_WORDS,          G2_WORDS,             MSM_SEG,            WAVE,            MANY_HEAD,               MANY_ROW};
    for (int i = 0; i < 12; i++) o[i] = c[i];
}
// plan_msmmany.cpp's plan_manymsm_call with the flag: the same words in the same order
size_t plan_manymsm_g2_call(const size_t* offsets, size_t npoints, size_t k, size_t nbits, int g2, uint64_t* head, uint64_t* rows, size_t max_rows) {
    const msm_many_plan P = msm_many_for(k, npoints, offsets == nullptr, nbits, g2 != 0);
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
// to_affine_for / to_affine_next: out[0] = run, out[1] = chunk, then per launch first, n, lanes, grid (up to max_rows) -> the number of launches
size_t plan_to_affine_call(size_t n, uint32_t force_run, uint64_t* out, size_t max_rows) {
    const to_affine_plan p = to_affine_for(n, force_run);
    out[0] = p.run, out[1] = p.chunk;
    size_t count = 0;
    for (size_t first = 0; first < n; count++) {
        const to_affine_launch l = to_affine_next(p, n, first);
        if (count < max_rows) {
            uint64_t* o = out + 2 + 4 * count;
            o[0] = l.first, o[1] = l.n, o[2] = l.lanes, o[3] = l.grid;
        }
        first += l.n;
    }
    return count;
}
void plan_to_affine_constants(uint64_t o[3]) { o[0] = TOAFF_DEVICE_LANES, o[1] = TOAFF_RUN_MAX, o[2] = TOAFF_CHUNK_POINTS; }
}

#ifdef PLAN_MSMMANY_G2_MAIN
// The sweep of tests/test_msm_many_g2_plan.py, checked here: every pass within the call's sizes and the G2 bounds, the passes tiling [0, k).
static int check_call(const size_t* offsets, size_t npoints, size_t k, size_t nbits, bool g2) {
    const msm_many_plan P = msm_many_for(k, npoints, offsets == nullptr, nbits, g2);
    const msm_many_sizes m = msm_many_sizes_for(P, offsets, npoints, k);
    const uint32_t bmax = g2 ? MSM_MANY_G2_BUCKETS_MAX : MSM_MANY_BUCKETS_MAX;
    size_t at = 0;
    for (size_t j = 0; j < k;) {
        const msm_many_pass s = msm_many_next(P, offsets, npoints, k, j);
        if (s.j0 != at || s.j1 <= s.j0 || s.j1 > k) return 1;
        at = j = s.j1;
        if (s.single) continue;
        const msm_many_sizes z = msm_many_extents(P, s);
        if (z.pts_int > m.pts_int || z.offs_dev > m.offs_dev || z.hist > m.hist || z.chist > m.chist || z.sorted > m.sorted || z.buckets > m.buckets ||
            z.segout > m.segout || z.part > m.part)
            return 2;
        if (s.pairs && (s.total > bmax || s.nv > MSM_MANY_VWIN_MAX || s.pairs > MSM_MANY_PAIRS_MAX || (g2 && s.team != 1))) return 3;
    }
    return at == k ? 0 : 4;
}
int main() {
    int bad = 0;
    size_t calls = 0;
    for (int g2 = 0; g2 < 2; g2++)
        for (size_t nbits : {1, 5, 64, 255, 256})
            for (size_t n : {1, 2, 33, 4096, 65536, 1 << 20, (1 << 20) + 1})
                for (size_t k : {1, 2, 5, 64, 1500, 70000}) {
                    if ((n > 65536 && k > 5) || (n >= 4096 && k > 1500)) continue;
                    bad |= check_call(nullptr, n, k, nbits, g2 != 0), calls++;      // shared
                    std::vector<size_t> offs(k + 1, 0);                              // ragged: lengths n, 0, 1, n, 0, 1, ...
                    for (size_t j = 0; j < k; j++) offs[j + 1] = offs[j] + (j % 3 == 0 ? n : j % 3 == 1 ? 0 : 1);
                    bad |= check_call(offs.data(), offs[k], k, nbits, g2 != 0), calls++;
                }
    for (size_t n : {1, 63, 64, 65, 65536, 65537, 1 << 20, (1 << 24) + 5, (1 << 25) + 1})
        for (uint32_t force : {0u, 1u, 8u, 100u}) {
            const to_affine_plan p = to_affine_for(n, force);
            if (p.run < 1 || p.run > TOAFF_RUN_MAX) bad |= 8;
            size_t first = 0;
            while (first < n) {
                const to_affine_launch l = to_affine_next(p, n, first);
                if (l.first != first || l.n == 0 || l.n > p.chunk || (size_t)l.lanes * p.run < l.n || (size_t)l.grid * WAVE < l.lanes) bad |= 16;
                first += l.n;
            }
            if (first != n) bad |= 32;
            calls++;
        }
    std::printf("plan_msmmany_g2: %zu calls walked, %s\n", calls, bad ? "VIOLATIONS" : "ok");
    return bad;
}
#endif
