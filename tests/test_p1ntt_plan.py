"""csrc/plan.hpp's entry for the transforms over G1 (p1ntt_sizes_for / p1ntt_slice / p1ntt_launch_for, through tests/host_emu/plan_p1ntt.cpp):
slices are whole vectors and cover [0, k) exactly once, one vector always fits, the hook only shortens, the launches hold a lane for every
butterfly and every run, the workspace sizes match what the stages and the finish address, and the sizes of large calls stay inside 64 bits."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32
CAP = 256 << 20
JAC, AFF = 192, 96                     # bytes of an internal Jacobian image and of an affine image


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_p1ntt.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_p1ntt.so"))
    L.p1ntt_plan_sizes.argtypes = [SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.p1ntt_plan_slice.argtypes = [SZ, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.p1ntt_plan_launch.argtypes = [SZ, SZ, ctypes.POINTER(U32)]
    L.p1ntt_plan_walk.argtypes = [SZ, SZ, ctypes.c_int]
    return L


def sizes(lib, n, k, vecs=0):
    out = (SZ * 7)()
    if not lib.p1ntt_plan_sizes(n, k, vecs, out):
        return None
    return dict(zip(("log2n", "vecs", "slices", "twiddles", "ws", "staging", "cap"), out))


@pytest.mark.parametrize("forced", [0, 1, 2, 100])
def test_slices_hold_whole_vectors_and_cover_every_one_once(lib, forced):
    rule = lambda n: max(1, CAP // (JAC * n))          # noqa: E731
    for n in (1, 2, 256, 4096, 1 << 16, 1 << 20, 1 << 21, 1 << 24):
        for k in (1, 2, 5, 257, 2048, 2049):
            s = sizes(lib, n, k, forced)
            per = min(rule(n), forced or rule(n), k)
            assert s["cap"] == CAP and s["log2n"] == n.bit_length() - 1 and s["twiddles"] == n // 2 * 32
            assert s["vecs"] == per and s["slices"] == -(-k // per) and s["ws"] == per * n * JAC and s["staging"] == per * n * AFF
            assert s["ws"] <= CAP or per == 1                              # one vector always forms a slice, whatever its size
            out, got = (SZ * 2)(), []
            for i in range(s["slices"]):
                assert lib.p1ntt_plan_slice(n, k, forced, i, out) == 1
                got.append((out[0], out[1]))
            assert lib.p1ntt_plan_slice(n, k, forced, s["slices"], out) == 0
            assert got[0][0] == 0 and sum(c for _, c in got) == k and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:]))
            assert all(c == per for _, c in got[:-1]) and 1 <= got[-1][1] <= per


def test_the_hook_only_shortens(lib):
    assert sizes(lib, 1 << 20, 64, 1000)["vecs"] == 1                       # 192 MiB a vector: the hook cannot lengthen a slice
    assert sizes(lib, 1 << 12, 1 << 20, 1 << 30)["vecs"] == CAP // (JAC << 12) == 341
    assert sizes(lib, 8, 5, 2)["vecs"] == 2 and sizes(lib, 8, 5, 7)["vecs"] == 5


def test_launches_hold_a_lane_for_every_butterfly_and_every_run(lib):
    out = (U32 * 3)()
    for n, count in ((1, 1), (1, 1000), (2, 1), (2, 257), (16, 257), (128, 64), (4096, 8), (1 << 16, 1), (1 << 20, 1), (1 << 32, 1)):
        assert lib.p1ntt_plan_launch(n, count, out) == 1
        stage_grid, run, finish_grid = out
        total = n * count
        assert stage_grid == -(-(total // 2) // 64) and 1 <= run <= 8
        assert finish_grid == -(-(-(-total // run)) // 64) and finish_grid * 64 * run >= total
        assert run == min(8, max(1, -(-total // (256 * 4 * 64))))            # to_affine's rule
    assert lib.p1ntt_plan_launch(1 << 32, 1, out) == 1 and out[0] == 1 << 25


@pytest.mark.parametrize("permute", [0, 1])
def test_workspace_sizes_match_what_the_lanes_address(lib, permute):
    for n, count in ((1, 1), (1, 70), (2, 1), (2, 257), (4, 3), (16, 257), (64, 5), (128, 3), (1024, 1), (4096, 2), (1 << 17, 1)):
        assert lib.p1ntt_plan_walk(n, count, permute) == 1, (n, count)


def test_large_calls_stay_inside_64_bits(lib):
    s = sizes(lib, 1 << 32, 1 << 20)
    assert s["vecs"] == 1 and s["slices"] == 1 << 20 and s["ws"] == JAC << 32 and s["staging"] == AFF << 32 and s["twiddles"] == 1 << 36 and s["log2n"] == 32


def test_refused_sizes(lib):
    for n in (0, 3, 6, 255, (1 << 32) + 1, 1 << 33):
        assert sizes(lib, n, 1) is None, n
    assert sizes(lib, 1 << 32, 1) is not None and sizes(lib, 1, 1)["log2n"] == 0
    assert sizes(lib, 4, 0)["slices"] == 0
