// The launch plan of the same-message pre-aggregation (csrc/plan.hpp combsets_measure, combsets_chain_on_host) for tests/test_combsets_plan.py:
// the product's own functions behind a C interface.  TEST INFRASTRUCTURE: never linked into the product library.
#include "plan.hpp"

extern "C" {
unsigned plan_comb_chain_lane_max() { return plan::COMB_CHAIN_LANE_MAX; }
size_t plan_comb_mul_chunk() { return plan::COMB_MUL_CHUNK; }
size_t plan_comb_members_max() { return plan::COMB_MEMBERS_MAX; }
unsigned plan_comb_agg_c() { return plan::AGG_C; }
int plan_combsets_chain_on_host(size_t len) { return plan::combsets_chain_on_host(len) ? 1 : 0; }
// out: lo, members, chunks, chunk_cap, host_chains; returns ok
int plan_combsets_measure(const size_t* offsets, size_t k, size_t out[5]) {
    const plan::combsets_plan p = plan::combsets_measure(offsets, k);
    out[0] = p.lo, out[1] = p.members, out[2] = p.chunks, out[3] = p.chunk_cap, out[4] = p.host_chains;
    return p.ok ? 1 : 0;
}
}
