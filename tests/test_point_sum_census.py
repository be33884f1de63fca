"""A guard on the INPUTS of tests/test_gpu_point_sums.py, not on the kernels: the drawn lists of small multiples (tests/small_multiples.py),
replayed on integers in the order the kernels combine them (tests/reduction_model.py), must meet every exceptional addition at every level:
equal partial sums and opposite partial sums (of at least two elements each, reached by different additions, so that their Z differ),
infinity on the left and infinity on the right.  If a kernel's reduction changes shape, the counts move and the inputs have to be redrawn.

The counts with the seeds as committed (equal, opposite, infinity left, infinity right, of all additions):

    k_jac_sum_blst, G1 (7 lambdas)   lane loop   15   20   57   56  of 2038      fold  11  18  79   73  of 1206
    k_jac_sum_blst, G2 (9 lambdas)   lane loop   16   21   57   56  of 2038      fold  13  17  79   73  of 1206
    k_g1_sum / k_g2_sum              lane loop  115  128  271  320  of 7468      fold  44  47  86  107  of 3024
    k_g1_sum2 / k_g2_sum2                         2    2    2    2  of 2316      (513 points are two blocks, 1025 three)
    k_aggsets_l0                                 55   71   88   93  of 2448
    k_aggsets_ln                                  6   10   26   19  of 296

These additions are exceptional as POINTS; with the device's nearly canonical products their H is still literally zero almost every time.  The
additions whose H is a non-zero multiple of p are the searched pairs of small_multiples.HARD_PAIRS, held by tests/test_host_emu.py.

k_*_sum2's own lane loop only ever adds a block's partial to an empty accumulator below 64 blocks (32 768 points); its fold is where partials
of different blocks meet.  The model is the same for both curves: G2 differs in the cap on the number of blocks alone, far above these sizes."""
import reduction_model as rm
import small_multiples as sm

REDRAW = "the reduction's shape changed: redraw the inputs of tests/small_multiples.py (seeds) until every class is met again; missing: %s\n%s"


def _check(c, levels):
    assert not c.missing(levels), REDRAW % (c.missing(levels), c.table(levels))


def test_jacobian_sum_inputs_meet_every_class():
    for nlam in (len(sm.LAMBDAS_FP), len(sm.LAMBDAS_FP2)):
        c = rm.Census()
        for label, ks, lams in sm.jac_cases(nlam):
            assert rm.jac_sum(c, ks, [l != 0 for l in lams]).v == sum(ks), label      # lambda index 0 is Z = 1
        _check(c, ("jac.lane", "jac.fold"))


def test_aggregate_inputs_meet_every_class():
    for g2 in (False, True):
        c = rm.Census()
        for label, ks in sm.agg_cases():
            assert rm.affine_sum(c, ks, g2=g2).v == sum(ks), label
        _check(c, ("sum.lane", "sum.fold", "sum2"))
    assert [rm.sum_grid(n) for n in (512, 513, 1024, 1025)] == [(1, 8), (2, 5), (2, 8), (3, 6)]      # 1025: m = 6 > 1, three blocks


def test_aggregate_sets_inputs_meet_every_class():
    from test_aggsets_plan import plan_aggsets_lib
    C = plan_aggsets_lib().aggsets_plan_c()
    lists = sm.aggsets_lists(C)
    c = rm.Census()
    assert rm.aggsets_sum(c, [ks for _, ks in lists]) == [sum(ks) for _, ks in lists]
    _check(c, ("agg.l0", "agg.ln"))
    assert any(sum(ks) == 0 for _, ks in lists) and {len(ks) for _, ks in lists} >= {1, 2, C - 1, C, C + 1, C * C + 1}
