// The product's launch plans (csrc/plan.hpp: plain C++, no device type) as a host library for ctypes - tests/util.py plan_lib().
// Structs go out as uint32 words in declaration order; tests/util.py names them.
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
}
