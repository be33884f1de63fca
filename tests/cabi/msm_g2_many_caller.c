/* A plain-C caller of the G2 many-MSM and Jacobian-to-affine entry points, built from include/blscurve_mi355x.h alone
 * (tests/test_cabi_msm_g2_many.py).  It makes only calls that are decided before a device is looked at, so it runs without a GPU; every line it
 * prints is `name value`. */
#include <stdio.h>
#include <string.h>

#include "blscurve_mi355x.h"

int main(void) {
    uint8_t out[288 * 2], pts[192 * 2], sc[32 * 2];
    size_t offs[3] = {0, 1, 2};
    memset(out, 0xaa, sizeof out);
    memset(pts, 0, sizeof pts);
    memset(sc, 0, sizeof sc);
    printf("many_null_ctx %d\n", mi355_bls_p2s_mult_pippenger_many(NULL, out, pts, 2, sc, offs, 2, 255));
    printf("many_null_ctx_k0 %d\n", mi355_bls_p2s_mult_pippenger_many(NULL, out, pts, 2, sc, offs, 0, 255));
    printf("many_device_null_ctx %d\n", mi355_bls_p2s_mult_pippenger_many_device(NULL, out, NULL, pts, 2, sc, NULL, 1, 255, NULL));
    printf("p1s_to_affine_null_ctx %d\n", mi355_bls_p1s_to_affine(NULL, pts, 1, out));
    printf("p1s_to_affine_null_ctx_n0 %d\n", mi355_bls_p1s_to_affine(NULL, pts, 0, out));
    printf("p1s_to_affine_device_null_ctx %d\n", mi355_bls_p1s_to_affine_device(NULL, pts, 1, out, NULL));
    printf("p2s_to_affine_null_ctx %d\n", mi355_bls_p2s_to_affine(NULL, pts, 1, out));
    printf("p2s_to_affine_device_null_ctx %d\n", mi355_bls_p2s_to_affine_device(NULL, pts, 1, out, NULL));
    printf("set_run_null_ctx %d\n", mi355_bls_debug_to_affine_set_run(NULL, 8));
    printf("out_untouched %d\n", out[0] == 0xaa && out[575] == 0xaa);
    printf("err_arg %d\n", MI355_BLS_ERR_ARG);
    return 0;
}
