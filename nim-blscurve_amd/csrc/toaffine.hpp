// Jacobian images to affine images for MANY points (mi355_bls_p1s_to_affine / mi355_bls_p2s_to_affine: blst_p1s_to_affine / blst_p2s_to_affine,
// blst_abi.nim:323, :345) - the body one lane of k_to_affine carries, written so that the host can run it (tests/host_emu/toaffine.cpp).
// A lane takes a RUN of consecutive points and shares ONE inversion among them (Montgomery's trick):
//   forward    pre[i] = the product of the non-zero Z of points 0 .. i of the run (a point with Z == 0 leaves the product as it is)
//   invert     inv = 1 / pre[last], once - and not at all for a run of nothing but infinities
//   backward   point i, from the last down: Z_i^-1 = inv x pre[i - 1], then inv = inv x Z_i; x = X Z^-2, y = Y Z^-3
// Three products per point beside the one inversion.  A point with Z == 0 is written as the all-zero image, the library's affine infinity.
// Where the points live is the caller's business: it hands in a loader and two stores.
#pragma once
#include "curve.hpp"
#include "plan.hpp"

namespace bls {

BLS_HD fp f_inv(const fp& a) { return fp_inv(fp_reduce(a)); }
BLS_HD fp2 f_inv(const fp2& a) { return fp2_inv(fp2_reduce(a)); }

// count <= plan::TOAFF_RUN_MAX points; load(i) -> jac<F> of point i of the run (called twice per point), store(i, aff<F>) and
// store_inf(i) write its image
template <class F, class Load, class Store, class StoreInf>
BLS_HD void to_affine_run(uint32_t count, Load&& load, Store&& store, StoreInf&& store_inf) {
    F pre[plan::TOAFF_RUN_MAX];
    F acc = f_one<F>();
    bool any = false;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0; i < count; i++) {
        const F z = load(i).z;
        if (!f_is_zero(z)) {
            acc = f_mul(acc, z);
            any = true;
        }
        pre[i] = acc;
    }
    F inv = any ? f_inv(acc) : f_zero<F>();
#pragma clang loop unroll(disable)
    for (uint32_t i = count; i-- > 0;) {
        const jac<F> p = load(i);
        if (f_is_zero(p.z)) {
            store_inf(i);
            continue;
        }
        const F zi = i ? f_mul(inv, pre[i - 1]) : inv;      // (pre is 1 in front of the run's first finite point)
        inv = f_mul(inv, p.z);
        const F zi2 = f_sqr(zi);
        store(i, aff<F>{f_mul(p.x, zi2), f_mul(p.y, f_mul(zi2, zi))});
    }
}

}  // namespace bls
