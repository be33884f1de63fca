/* A plain-C caller of the fixed-base table MSM entry points, built from include/blscurve_mi355x.h alone (tests/test_cabi_msm_table.py).  It makes
 * only calls that are decided before a device is looked at, so it runs without a GPU; every line it prints is `name value`. */
#include <stdio.h>
#include <string.h>

#include "blscurve_mi355x.h"

int main(void) {
    mi355_bls_p1s_table* tab = NULL;
    uint8_t out[144 * 2], pts[96 * 2], sc[32 * 2];
    uint32_t plan[3] = {7, 7, 7};
    memset(out, 0xaa, sizeof out);
    memset(pts, 0, sizeof pts);
    memset(sc, 0, sizeof sc);
    printf("sizeof_4096_12_255 %lu\n", (unsigned long)mi355_bls_p1s_table_sizeof(4096, 12, 255));
    printf("sizeof_rule_4096 %lu\n", (unsigned long)mi355_bls_p1s_table_sizeof(4096, 0, 255));
    printf("sizeof_refused %lu\n", (unsigned long)(mi355_bls_p1s_table_sizeof(0, 12, 255) + mi355_bls_p1s_table_sizeof(5, 4, 255) +
                                                   mi355_bls_p1s_table_sizeof(5, 17, 255) + mi355_bls_p1s_table_sizeof(5, 8, 257)));
    printf("create_null_ctx %d\n", mi355_bls_p1s_table_create(NULL, &tab, pts, 2, 8, 255));
    printf("create_device_null_ctx %d\n", mi355_bls_p1s_table_create_device(NULL, &tab, pts, 2, 8, 255, NULL));
    printf("table_still_null %d\n", tab == NULL);
    mi355_bls_p1s_table_destroy(NULL);
    printf("mult_null_ctx %d\n", mi355_bls_p1s_mult_table(NULL, out, tab, sc, 255));
    printf("mult_device_null_ctx %d\n", mi355_bls_p1s_mult_table_device(NULL, out, tab, sc, 255, NULL));
    printf("many_null_ctx %d\n", mi355_bls_p1s_mult_table_many(NULL, out, tab, sc, 0, 255));
    printf("many_device_null_ctx %d\n", mi355_bls_p1s_mult_table_many_device(NULL, out, NULL, tab, sc, 2, 255, NULL));
    printf("rows_null_table %d\n", mi355_bls_debug_p1s_table_rows(NULL, 0, 1, 0, 1, out));
    printf("last_plan_null_ctx %d\n", mi355_bls_debug_p1s_table_last_plan(NULL, plan));
    printf("set_plan_null_ctx %d\n", mi355_bls_debug_p1s_table_set_plan(NULL, 1, 64));
    printf("out_untouched %d\n", out[0] == 0xaa && out[287] == 0xaa && plan[0] == 7);
    printf("err_arg %d\n", MI355_BLS_ERR_ARG);
    return 0;
}
