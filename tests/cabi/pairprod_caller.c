/* A plain-C caller of the pairing-product entry points, built from include/blscurve_mi355x.h alone (tests/test_cabi_pairprod.py).  It makes only
 * calls that are decided before a device is looked at, so it runs without a GPU; every line it prints is `name value`. */
#include <stdio.h>
#include <string.h>

#include "blscurve_mi355x.h"

int main(void) {
    uint8_t p1[96 * 2], q2[192 * 2], out[2], status[2], gt[576 * 2], rnd[32];
    uint64_t r[2] = {3, 5};
    size_t offs[3] = {0, 1, 2};
    memset(p1, 0, sizeof p1);
    memset(q2, 0, sizeof q2);
    memset(rnd, 7, sizeof rnd);
    memset(out, 0xaa, sizeof out);
    memset(status, 0xaa, sizeof status);
    memset(gt, 0xaa, sizeof gt);
    printf("each_null_ctx %d\n", mi355_bls_pairing_check_each(NULL, p1, q2, offs, 2, 0, out, status));
    printf("each_device_null_ctx %d\n", mi355_bls_pairing_check_each_device(NULL, p1, q2, offs, 2, 0, out, status, NULL));
    printf("products_null_ctx %d\n", mi355_bls_pairing_products(NULL, p1, q2, offs, 2, MI355_BLS_PAIR_VALIDATE, out, status, gt));
    printf("products_device_null_ctx %d\n", mi355_bls_pairing_products_device(NULL, p1, q2, offs, 2, 0, out, status, gt, NULL));
    printf("batch_null_ctx %d\n", mi355_bls_batch_pairing_check(NULL, p1, q2, offs, 2, 0, rnd, status));
    printf("batch_device_null_ctx %d\n", mi355_bls_batch_pairing_check_device(NULL, p1, q2, offs, 2, 0, rnd, status, NULL));
    printf("locate_null_ctx %d\n", mi355_bls_batch_pairing_check_locate(NULL, p1, q2, offs, 2, 0, rnd, status, out));
    printf("locate_device_null_ctx %d\n", mi355_bls_batch_pairing_check_locate_device(NULL, p1, q2, offs, 2, 0, rnd, status, out, NULL));
    printf("scalars_null_ctx %d\n", mi355_bls_debug_batch_pairing_check_scalars(NULL, p1, q2, offs, 2, 0, r, status, gt));
    printf("null_ctx_k0 %d\n", mi355_bls_pairing_check_each(NULL, p1, q2, offs, 0, 0, out, status));      /* the NULL context comes first */
    printf("untouched %d\n", out[0] == 0xaa && out[1] == 0xaa && status[0] == 0xaa && gt[0] == 0xaa && gt[1151] == 0xaa);
    printf("codes %d%d%d%d%d\n", MI355_BLS_PAIR_OK, MI355_BLS_PAIR_P_OFF_CURVE, MI355_BLS_PAIR_P_NOT_IN_G1, MI355_BLS_PAIR_Q_OFF_CURVE,
           MI355_BLS_PAIR_Q_NOT_IN_G2);
    printf("validate_bit %u\n", MI355_BLS_PAIR_VALIDATE);
    printf("err_arg %d\n", MI355_BLS_ERR_ARG);
    return 0;
}
