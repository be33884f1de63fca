// The per-set verification plan of csrc/plan.hpp (each_for and its slice schedule) as a host library for ctypes - tests/test_vereach_plan.py.
#include "plan.hpp"
using namespace plan;

extern "C" {
size_t each_plan_slice_max(size_t cap) { return each_slice_max(cap); }
size_t each_plan_stride(size_t cap) { return each_stride(cap); }
size_t each_plan_nslices(size_t n, size_t slice_max) { return each_nslices(n, slice_max); }
size_t each_plan_slice_count(size_t n, size_t done, size_t nslices, uint32_t slice) { return each_slice_count(n, done, nslices, slice); }
uint32_t each_plan_team_clear_max(uint32_t slots) { return each_team_clear_max(slots); }
uint32_t each_plan_team_lines_max(uint32_t slots) { return each_team_lines_max(slots); }
uint32_t each_plan_engine_max(uint32_t slots) { return each_engine_max(slots); }
uint32_t each_plan_engine_grid_max(uint32_t slots) { return each_engine_grid_max(slots); }
// setup_grid | lines team, form, grid, pairs, extra pairs | tail_engine, tail_grid
void each_plan_for(uint32_t slots, int coop, uint32_t m, uint32_t o[8]) {
    const each_plan p = each_for(slots, coop != 0, m);
    o[0] = p.setup_grid;
    o[1] = p.lines.main.team, o[2] = p.lines.main.form, o[3] = p.lines.main.grid, o[4] = p.lines.main_pairs, o[5] = p.lines.extra_pairs;
    o[6] = p.tail_engine, o[7] = p.tail_grid;
}
}
