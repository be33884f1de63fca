// CPU execution of the shared-inversion body of the Jacobian-to-affine calls (csrc/toaffine.hpp to_affine_run, what one lane of k_to_affine
// carries) under the bounds tracker, lane by lane as the kernel cuts n points into runs, for tests/test_to_affine_emu.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>

#include "toaffine.hpp"
using namespace bls;

namespace {
void store_aff(uint8_t* o, const g1_aff& a) { fp_store_le(o, a.x), fp_store_le(o + 48, a.y); }
void store_aff(uint8_t* o, const g2_aff& a) { fp2_store_le(o, a.x), fp2_store_le(o + 96, a.y); }
g1_jac load_jac(const uint8_t* p, const g1_jac*) { return g1_jac_load(p); }
g2_jac load_jac(const uint8_t* p, const g2_jac*) { return g2_jac_load(p); }

template <class F>
int run_all(const uint8_t* in, size_t n, uint32_t run, uint8_t* out) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192, JACB = AFFB / 2 * 3;
    if (run < 1 || run > plan::TOAFF_RUN_MAX) return -1;
    int inversions = 0;
    for (size_t first = 0; first < n; first += run) {
        const uint32_t count = (uint32_t)(n - first < run ? n - first : run);
        bool any = false;
        to_affine_run<F>(
            count,
            [&](uint32_t i) {
                const jac<F> p = load_jac(in + (first + i) * JACB, (const jac<F>*)nullptr);
                any |= !f_is_zero(p.z);
                return p;
            },
            [&](uint32_t i, const aff<F>& a) { store_aff(out + (first + i) * AFFB, a); }, [&](uint32_t i) { memset(out + (first + i) * AFFB, 0, AFFB); });
        inversions += any;
    }
    return inversions;
}
}  // namespace

extern "C" {
// n Jacobian images -> n affine images, in runs of `run` points per lane.  Returns the number of runs that held a finite point (the
// inversions a kernel makes), or -1 for a run length the plan never gives.
int emu_to_affine_g1(const uint8_t* in144, size_t n, uint32_t run, uint8_t* out96) { return run_all<fp>(in144, n, run, out96); }
int emu_to_affine_g2(const uint8_t* in288, size_t n, uint32_t run, uint8_t* out192) { return run_all<fp2>(in288, n, run, out192); }
}
