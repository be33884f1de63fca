"""The chosen operands of tests/fp_operands.py through the bounds-tracked CPU build of the device arithmetic (tests/host_emu): every (operation,
family) pairing that tests/test_gpu_fp_ops.py sends to the device, with each operand tagged by the bounds its family declares.

  (a) no BLS_REQUIRE fires (the tracker aborts the process): every chosen operand is inside the contract of the operation it is paired with - a
      member that is not is a mistake in the family, not a finding;
  (b) every result is congruent to the big-integer model;
  (c) the documented output shape holds: limbs 0..12 in [0, 2^28) and |value| < 2p for the multipliers and the exponentiation, |value| < 0.51 p
      for fp_reduce (and for the row exponentiations, which reduce what they hand back), a carry of at most 16 on the limbs of a row product.

This is the reference side of the GPU test, validated without a GPU: the same check functions run there with the device behind `run`."""
import ctypes

import pytest

import fp_operands as F

FPOP = {"fp_mul": 0, "fp_sqr": 1, "fp_sqr_n1": 2, "fp_sqr_n4": 3, "fp_dot2": 4, "fp_reduce": 5, "fp_inv": 6, "fp_pow": 7, "pred": 8,
        "row_mul": 16, "row_sqr": 17, "pow_per_row": 18, "pow_two_rows": 19}


@pytest.fixture(scope="module")
def run(emu):
    def run(op, a, b, fam_a, fam_b):
        per = 2 if op == "fp_dot2" else 1
        assert len(a) == len(b) and len(a) % per == 0
        n = len(a) // per
        out = ctypes.create_string_buffer(n * 56)
        (vba, lba), (vbb, lbb) = F.BOUNDS[fam_a], F.BOUNDS[fam_b]
        assert emu.emu_fp_op(FPOP[op], F.words(a), F.words(b), n, vba, lba, vbb, lbb, out) == 0
        return F.unwords(out.raw)
    return run


def test_op_codes_are_the_headers():
    import re
    import __graft_entry__ as ge
    hdr = open(ge.ROOT + "/include/blscurve_mi355x.h").read()
    codes = {k.lower(): int(v) for k, v in re.findall(r"MI355_BLS_FPOP_([A-Z0-9_]+) = (\d+)", hdr)}
    assert codes == FPOP


def test_families_are_what_they_declare():
    """seeded and deterministic; about 60 images each; the value model round-trips"""
    assert {k: len(v) for k, v in F.FAMILIES.items()} == {"canon": 70, "noncanon": 60, "lazy": 60, "pow_corner": 34}
    for fam, members in F.FAMILIES.items():
        assert len({n for n, _ in members}) == len(members), fam
        assert F.unwords(F.words([i for _, i in members])) == [i for _, i in members]
    assert F.val(F.carried(-1)) == -1 and F.val(F.carried(F.P)) == F.P and F.limbs(F.carried(-1))[13] == -1
    assert F._families() == F.FAMILIES


@pytest.mark.parametrize("pairing", F.PAIRINGS, ids=lambda p: "%s-%s" % p)
def test_multipliers(run, pairing):
    F.check_multipliers(run, pairing)


def test_reduce_inverse_predicates(run):
    F.check_reduce(run)
    F.check_inv(run)
    F.check_predicates(run)


def test_exponentiation_in_its_three_forms(run):
    F.check_pow(run)


def test_sswu_list_meets_its_conditions_and_maps_right(emu):
    """fp_operands.sswu_cases() asserts the branch tallies of the u list (both values of is_sq and of qr at least 50 times, the tv2 = 0 arm once,
    g.c1 = 0 for the whole real-ratio family, its d = 0 arm taken and left at least twice); the list then goes through the CPU build's map."""
    def map_fn(pairs, fam):
        flat = [c for pr in pairs for c in pr]
        if len(pairs) % 2:
            flat += list(pairs[0])                       # the hook maps pairs of u: pad to an even count
        n = len(flat) // 4
        out = ctypes.create_string_buffer(2 * n * 288)
        vb, lb = F.BOUNDS[fam]
        emu.emu_map_to_g2(F.words(flat), n, vb, lb, out)
        return [out.raw[288 * k:288 * k + 288] for k in range(len(pairs))]
    F.check_sswu(map_fn)
