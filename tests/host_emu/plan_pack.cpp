// The staging layout of the grouped calls' host inputs (csrc/plan.hpp pack_for) behind a C interface, for tests/test_pack_plan.py.
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
}
