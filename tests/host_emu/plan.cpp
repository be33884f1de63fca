// The product's launch plans (csrc/plan.hpp: plain C++, no device type) as a host library for ctypes - tests/util.py plan_lib().
// Structs go out as uint32 words in declaration order; tests/util.py names them.
#include <initializer_list>

#include "plan.hpp"
using namespace plan;

static uint32_t* put(uint32_t* o, const stage& s) {
    *o++ = s.team, *o++ = s.form, *o++ = s.grid;
    return o;
}
static uint32_t* put(uint32_t* o, const lines_plan& p) {
    *o++ = p.main_pairs;
    o = put(o, p.main);
    *o++ = p.extra_pairs;
    return put(o, p.extra);
}

static uint64_t* put(uint64_t* o, const msm_sizes& s) {
    for (size_t v : {s.d_pts, s.d_sc, s.pts_int, s.hist, s.chist, s.shist, s.part, s.sorted, s.buckets, s.segout, s.winout, s.out}) *o++ = v;
    return o;
}

extern "C" {
void plan_constants(uint32_t o[7]) {
    const uint32_t c[7] = {WAVE, N_LINES, SIG_SLOTS_MAX, (uint32_t)SIG_WIDE_MIN, FORK_ITEMS_PER_SLOT, TEAM_CLEAR_ITEMS_PER_SLOT, TEAM_LINES_ITEMS_PER_SLOT};
    for (int i = 0; i < 7; i++) o[i] = c[i];
}
uint32_t plan_team_rows_max(uint32_t slots) { return team_rows_max(slots); }
uint32_t plan_team_lines_max(uint32_t slots) { return team_lines_max(slots); }
uint32_t plan_team_form(uint32_t slots, uint32_t count) { return team_form_for(slots, count); }
void plan_lines(uint32_t slots, int coop, uint32_t npairs, uint32_t extra, uint32_t o[8]) { put(o, lines_for(slots, coop != 0, npairs, extra)); }
void plan_slice(uint32_t slots, int coop, int have_side, size_t n, uint32_t o[27]) {
    const slice_plan p = slice_for(slots, coop != 0, have_side != 0, n);
    *o++ = p.nb, *o++ = p.hash_map.form, *o++ = p.hash_map.grid;
    o = put(o, p.clear);
    *o++ = p.pkmul_spread, *o++ = p.side, *o++ = p.pk_stream, *o++ = p.sig_stream;
    *o++ = p.cw, *o++ = p.nwin, *o++ = p.total, *o++ = p.lshift, *o++ = p.bucket_grid, *o++ = p.extra_apart;
    put(put(o, p.extra_lines), p.lines);
}
void plan_lineprod(uint32_t slots, uint32_t nblk_cap, uint32_t stride, uint32_t npairs, int fold, uint32_t o[6]) {
    const lineprod_plan p = lineprod_for(slots, nblk_cap, stride, npairs, fold != 0);
    o[0] = p.nblk, o[1] = p.m, o[2] = (uint32_t)p.per_lane, o[3] = p.live, o[4] = p.per, o[5] = p.nb1;
}
size_t plan_aggv_cut(const uint32_t* msg_offsets, size_t n, size_t a, size_t cap) { return aggv_cut(msg_offsets, n, a, cap); }
int plan_aggv_all32(const uint32_t* offs, size_t n) { return aggv_all32(offs, n); }
size_t plan_shard_nslices(size_t n, size_t cap) { return shard_nslices(n, cap); }
int plan_shard_workspaces(size_t nslices) { return shard_workspaces(nslices); }
size_t plan_shard_slice_count(size_t n, size_t done, size_t nslices, uint32_t slice) { return shard_slice_count(n, done, nslices, slice); }
int plan_shard_workspace_of(size_t nslices, uint32_t slice, int nl) { return shard_workspace_of(nslices, slice, nl); }
uint32_t plan_chunk_of_tuple(size_t n_total, uint32_t B, size_t t) { return chunk_of_tuple(n_total, B, t); }
// the MSM, the point sums and the context's sizes: 64-bit words, tests/util.py names them
void plan_msm_constants(uint64_t o[14]) {
    const uint64_t c[14] = {MSM_SEG, MSM_ORD_PER, PIP_SLICES, PIP_SORT_THREADS, PIP_SORT_MAX_CBK, MSM_TEAM_LANES_MAX, MSM_TAIL_WAVES_MAX, MSM_WINDOWS_MAX,
                            MSM_NSPLIT_MAX, MSM_GROUPS_MAX, SUM_PARTS_BYTES, G1_WORDS, G2_WORDS, F12_WORDS};
    for (int i = 0; i < 14; i++) o[i] = c[i];
}
// `count` plans, MSM_ROW words each: the plan, then msm_extents of it, then msm_sizes_for what msm_reserve grows an empty workspace to for the call
enum { MSM_ROW = 14 + 13 + 2 * 12 + 2 * 12 };
size_t plan_msm_row(void) { return MSM_ROW; }
void plan_msm_many(const uint64_t* npoints, size_t count, size_t nbits, int g2, int allow_split, int have_side, uint64_t* o) {
    for (size_t i = 0; i < count; i++) {
        const msm_plan p = msm_for(npoints[i], nbits, g2 != 0, allow_split != 0, have_side != 0);
        const uint32_t* w = &p.W.nwin;
        for (int j = 0; j < 14; j++) *o++ = w[j];
        for (uint32_t v : {p.n, p.total, p.segs_per_win, p.nseg, p.nsplit, (uint32_t)p.lds_sort, p.per, p.point_grid, p.slice_scan_grid, p.ngroups, p.cut[0], p.cut[1], p.cut[2]}) *o++ = v;
        for (const msm_group& G : p.group)
            for (uint32_t v : {G.w0, G.w1, G.g0, G.gc, G.t0, G.tc, G.order_grid, G.bucket_grid, G.team, G.segred_grid, G.tail_waves, G.tail_lanes}) *o++ = v;
        o = put(o, msm_extents(p, g2 != 0));
        o = put(o, msm_sizes_for(npoints[i] * (g2 ? 192 : 96), p.total));
    }
}
// point sums of n[0 .. count): nblk, m each
void plan_sum_many(int g2, uint32_t slots, const uint32_t* n, size_t count, uint32_t* o) {
    for (size_t i = 0; i < count; i++) {
        const sum_plan p = g2 ? g2_sum_for(slots, n[i]) : g1_sum_for(slots, n[i]);
        *o++ = p.nblk, *o++ = p.m;
    }
}
// plan_lineprod for npairs = first .. first + count - 1: six words each
void plan_lineprod_many(uint32_t slots, uint32_t nblk_cap, uint32_t stride, uint32_t first, size_t count, int fold, uint32_t* o) {
    for (size_t i = 0; i < count; i++, o += 6) plan_lineprod(slots, nblk_cap, stride, first + (uint32_t)i, fold, o);
}
void plan_ctx(uint32_t slots, size_t max_sets, uint64_t o[6]) {
    const ctx_sizes s = ctx_for(slots, max_sets);
    o[0] = s.stride, o[1] = s.mstride, o[2] = s.nblk_cap, o[3] = s.lpart_words, o[4] = s.lpart_mid_words, o[5] = s.export_bytes;
}
}
