"""The shared-inversion body of the Jacobian-to-affine calls (csrc/toaffine.hpp to_affine_run, what one lane of k_to_affine carries) executed on
the host under the bounds tracker (tests/host_emu/toaffine.cpp), both fields, runs of 1, 2 and 8 points: infinity at the first, a middle and
the last place of a run, a run of infinities only (no inversion of zero), Z == 1, Z scaled by random lambda - byte for byte the oracle's
affine images."""
import ctypes

import pytest

import g2many_helpers as h


def run_emu(g2, images, n, run):
    out = ctypes.create_string_buffer((192 if g2 else 96) * n)
    L = h.toaffine_lib()
    inv = (L.emu_to_affine_g2 if g2 else L.emu_to_affine_g1)(images, n, run, out)
    return out.raw, inv


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("run", [1, 2, 8])
def test_runs_with_infinities_at_every_place(g2, run):
    for n in (run, 3 * run + 1):
        for inf_at in h.infinity_placements(n, run):
            images, want = h.to_affine_case(g2, n, inf_at, seed=run, unit_z_at=(0, n - 1))
            got, inversions = run_emu(g2, images, n, run)
            assert got == want, (g2, run, n, inf_at)
            runs_with_a_point = sum(1 for f in range(0, n, run) if any(i not in inf_at for i in range(f, min(f + run, n))))
            assert inversions == runs_with_a_point                                    # one inversion per run, none for a run of infinities


@pytest.mark.parametrize("g2", [False, True])
def test_a_run_length_the_plan_never_gives_is_refused(g2):
    images, _ = h.to_affine_case(g2, 2)
    assert run_emu(g2, images, 2, 0)[1] == -1 and run_emu(g2, images, 2, 9)[1] == -1
