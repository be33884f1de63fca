// The launch plan of batchVerify by message (csrc/plan.hpp slice_for_grouped) beside slice_for and the per-stage deciders it is built
// from, for tests/test_bymsg_plan.py: the product's own functions behind a C interface.  TEST INFRASTRUCTURE: never linked into the
// product library.
#include "plan.hpp"

namespace {
void put_stage(const plan::stage& s, unsigned* o) { o[0] = s.team, o[1] = s.form, o[2] = s.grid; }
void put_lines(const plan::lines_plan& l, unsigned* o) {
    o[0] = l.main_pairs, put_stage(l.main, o + 1), o[4] = l.extra_pairs;
    if (l.extra_pairs) put_stage(l.extra, o + 5);
    else o[5] = o[6] = o[7] = 0;
}
// hash_map (2) | clear (3) | extra_apart (1) | extra_lines (3) | lines (8)
void put_pairs(const plan::hash_map_plan& h, const plan::stage& clear, bool apart, const plan::stage& extra, const plan::lines_plan& lines, unsigned* o) {
    o[0] = h.form, o[1] = h.grid, put_stage(clear, o + 2), o[5] = apart, put_stage(extra, o + 6), put_lines(lines, o + 9);
}
// nb, pkmul_spread, side, pk_stream, sig_stream, cw, nwin, total, lshift, bucket_grid
void put_sets(const plan::slice_plan& p, unsigned* o) {
    o[0] = p.nb, o[1] = p.pkmul_spread, o[2] = p.side, o[3] = p.pk_stream, o[4] = p.sig_stream, o[5] = p.cw, o[6] = p.nwin, o[7] = p.total, o[8] = p.lshift,
    o[9] = p.bucket_grid;
}
}  // namespace

extern "C" {
size_t plan_bymsg_min_shared() { return plan::BYMSG_MIN_SHARED; }
// out: ordinary, table_slots, grid_n, grid_k | sets (10) | pairs (17)
void plan_slice_for_grouped(unsigned slots, int coop, int side_ok, size_t n, size_t k, unsigned out[31]) {
    const plan::grouped_plan g = plan::slice_for_grouped(slots, coop != 0, side_ok != 0, n, k);
    out[0] = g.ordinary, out[1] = g.table_slots, out[2] = g.grid_n, out[3] = g.grid_k;
    put_sets(g.sets, out + 4);
    put_pairs(g.hash_map, g.clear, g.extra_apart, g.extra_lines, g.lines, out + 14);
}
// slice_for(n) in the same words: sets (10) | pairs (17)
void plan_slice_for_words(unsigned slots, int coop, int side_ok, size_t n, unsigned out[27]) {
    const plan::slice_plan p = plan::slice_for(slots, coop != 0, side_ok != 0, n);
    put_sets(p, out);
    put_pairs(p.hash_map, p.clear, p.extra_apart, p.extra_lines, p.lines, out + 10);
}
// lines_for in put_lines' words
void plan_lines_for_words(unsigned slots, int coop, unsigned npairs, unsigned extra, unsigned out[8]) { put_lines(plan::lines_for(slots, coop != 0, npairs, extra), out); }
}
