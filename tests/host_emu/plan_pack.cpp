// The staging layouts of the host forms (csrc/plan.hpp: pack_for for the grouped calls, the row columns for the per-row calls) behind a C
// interface, for tests/test_pack_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include "plan.hpp"

extern "C" {
size_t plan_pack_parts_max() { return plan::PACK_PARTS_MAX; }
// at: n offsets (written for n <= PACK_PARTS_MAX); returns the total to reserve, 0 for more parts than that
size_t plan_pack_for(const size_t* bytes, size_t n, size_t* at) {
    const plan::pack_layout p = plan::pack_for(bytes, n);
    for (size_t i = 0; i < n && i < plan::PACK_PARTS_MAX; i++) at[i] = p.at[i];
    return p.total;
}

size_t plan_row_bytes() { return plan::ROW_BYTES; }
size_t plan_row_column_count() { return plan::ROW_COLUMN_COUNT; }
// column i of the per-row staging: its call and name, the column of the same call it shares its bytes with (null: none), its buffer
// (0: d_comp, 1: d_sets), start and width; 0 for an i past the last column
int plan_row_column(size_t i, const char** call, const char** column, const char** shares, uint32_t* buf, uint32_t* start, uint32_t* width) {
    if (i >= plan::ROW_COLUMN_COUNT) return 0;
    const plan::row_col_entry& e = plan::ROW_COLUMNS[i];
    *call = e.call, *column = e.column, *shares = e.shares;
    *buf = e.col.buf == plan::ROW_SETS ? 1 : 0, *start = e.col.start, *width = e.col.width;
    return 1;
}
}
