// The numbers of csrc/plan.hpp fropen_sizes_for / fropen_pass for tests/test_fropen_plan.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstddef>
#include <cstdint>

#include "plan.hpp"

extern "C" {
// -> 1 and out[8] = per_pass, passes, log2n, domain, scan, status, out_ys, out_quot | 0: refused
int fropen_plan_sizes(size_t n, size_t k, int eval, size_t forced, size_t out[8]) {
    const plan::fropen_sizes s = plan::fropen_sizes_for(n, k, eval != 0, forced);
    if (!s.ok) return 0;
    out[0] = s.per_pass, out[1] = s.passes, out[2] = s.log2n, out[3] = s.domain, out[4] = s.scan, out[5] = s.status, out[6] = s.out_ys, out[7] = s.out_quot;
    return 1;
}
// pass p: out[2] = first, count
int fropen_plan_pass(size_t n, size_t k, int eval, size_t forced, size_t p, size_t out[2]) {
    const plan::fropen_sizes s = plan::fropen_sizes_for(n, k, eval != 0, forced);
    if (!s.ok || p >= s.passes) return 0;
    plan::fropen_pass(s, k, p, out[0], out[1]);
    return 1;
}
size_t fropen_plan_polys_pass(void) { return plan::FROPEN_POLYS_PASS; }
size_t fropen_plan_scan_bytes(void) { return plan::FROPEN_SCAN_BYTES; }
}
