"""csrc/plan.hpp's entry for the cell-proof call (fk20_cells_sizes_for / fk20_cells_pass / fk20_cells_launch_for, through
tests/host_emu/plan_fk20cells.cpp): passes are whole polynomials under the stated budget of 2n scalars, 2n product images and max(2q, N)
workspace images each and cover [0, k) exactly once, one polynomial always fits, the hook only shortens, the launches hold a lane for every
run, term, group, butterfly and element at both sides of every hand-over (N = q, 2q, 4q), the buffer sizes match what the lanes address, the
largest legal n and ext stay inside 64 bits, and every size the call refuses is refused here."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32
U64 = ctypes.c_uint64
CAP = 256 << 20
JAC, AFF, FR = 192, 96, 32             # bytes of an internal Jacobian image, of an affine image and of a scalar
FAN_LOG2 = 3
KEYS = ("log2n", "log2cell", "log2q", "log2cells", "log2w", "per_pass", "passes", "scalars", "prod", "ws", "polys", "out", "status", "tw_fr", "tw_inv", "tw_fwd", "cap")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_fk20cells.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_fk20cells.so"))
    L.fk20c_plan_sizes.argtypes = [SZ, SZ, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.fk20c_plan_pass.argtypes = [SZ, SZ, SZ, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.fk20c_plan_launch.argtypes = [SZ, SZ, SZ, SZ, ctypes.POINTER(U32), ctypes.POINTER(U32), ctypes.POINTER(U64)]
    L.fk20c_plan_walk.argtypes = [SZ, SZ, SZ, SZ, ctypes.c_int, ctypes.c_int]
    return L


def sizes(lib, n, cell, ext, k, forced=0):
    out = (SZ * 17)()
    if not lib.fk20c_plan_sizes(n, cell, ext, k, forced, out):
        return None
    return dict(zip(KEYS, out))


def per_poly(n, cell, ext):
    q = n // cell
    return 2 * n * (JAC + FR) + max(2 * q, q << ext) * JAC


@pytest.mark.parametrize("forced", [0, 1, 2, 100])
def test_passes_hold_whole_polynomials_and_cover_every_one_once(lib, forced):
    for n, cell, ext in ((1, 1, 0), (16, 4, 1), (128, 8, 1), (4096, 64, 1), (4096, 1, 0), (4096, 64, 6), (1 << 16, 64, 1), (1 << 20, 64, 1), (1 << 24, 1 << 24, 3)):
        rule = max(1, CAP // per_poly(n, cell, ext))
        for k in (1, 2, 5, 257, 2049):
            s = sizes(lib, n, cell, ext, k, forced)
            per = min(rule, forced or rule, k)
            q = n // cell
            big, w = q << ext, max(2 * q, q << ext)
            assert s["cap"] == CAP and (1 << s["log2n"], 1 << s["log2cell"], 1 << s["log2q"], 1 << s["log2cells"], 1 << s["log2w"]) == (n, cell, q, big, w)
            assert (s["tw_fr"], s["tw_inv"], s["tw_fwd"]) == (q * 32, q * 32, big // 2 * 32)
            assert s["per_pass"] == per and s["passes"] == -(-k // per) and s["status"] == 4 * per
            assert (s["scalars"], s["prod"], s["ws"]) == (per * 2 * n * FR, per * 2 * n * JAC, per * w * JAC)
            assert (s["polys"], s["out"]) == (per * n * FR, per * big * AFF)
            assert s["ws"] + s["prod"] + s["scalars"] <= CAP or per == 1          # one polynomial always forms a pass, whatever its size
            out, got = (SZ * 2)(), []
            for i in range(s["passes"]):
                assert lib.fk20c_plan_pass(n, cell, ext, k, forced, i, out) == 1
                got.append((out[0], out[1]))
            assert lib.fk20c_plan_pass(n, cell, ext, k, forced, s["passes"], out) == 0
            assert got[0][0] == 0 and sum(c for _, c in got) == k and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:]))
            assert all(c == per for _, c in got[:-1]) and 1 <= got[-1][1] <= per


def test_the_hook_only_shortens(lib):
    assert sizes(lib, 1 << 20, 64, 1, 64, 1000)["per_pass"] == 1                  # 448 MiB and more a polynomial: the hook cannot lengthen a pass
    assert sizes(lib, 4096, 64, 1, 1 << 20, 1 << 30)["per_pass"] == CAP // per_poly(4096, 64, 1) == 144
    assert sizes(lib, 16, 4, 1, 5, 2)["per_pass"] == 2 and sizes(lib, 16, 4, 1, 5, 7)["per_pass"] == 5
    assert sizes(lib, 16, 4, 1, 5, 2)["passes"] == 3 and sizes(lib, 16, 4, 1, 3, 1)["passes"] == 3
    assert sizes(lib, 16, 4, 1, 0)["passes"] == 0


def test_launches_hold_a_lane_for_everything_at_both_sides_of_every_hand_over(lib):
    out, levels, lanes = (U32 * 9)(), U32(), (U64 * 11)()
    shapes = [(n, cell, ext, count) for n, cell in ((16, 4), (128, 8), (4096, 64), (4096, 1), (4096, 512), (1 << 16, 64)) for ext in (0, 1, 2) for count in (1, 3, 64)]
    shapes += [(1, 1, 0, 1), (1, 1, 5, 1000), (2, 2, 0, 257), (16, 16, 1, 3), (1 << 20, 64, 1, 1), (1 << 31, 1, 1, 1), (1 << 31, 1 << 31, 1, 1), (1 << 16, 2, 16, 1)]
    for n, cell, ext, count in shapes:
        assert lib.fk20c_plan_launch(n, cell, ext, count, out, ctypes.byref(levels), lanes) == 1
        circ, point, inv, pad, fwd, run, finish, run_h, finish_h = out
        q = n // cell
        big = q << ext
        c = cell.bit_length() - 1
        assert circ == -(-(count * cell * -(-2 * q // 16)) // 256) and point == -(-2 * n * count // 64) and inv == -(-q * count // 64)
        assert pad == (0 if ext == 0 else -(-big * count // 64)) and fwd == -(-(big * count // 2) // 64)
        for total, r, grid in ((big * count, run, finish), (q * count, run_h, finish_h)):
            assert 1 <= r <= 8 and r == min(8, max(1, -(-total // (256 * 4 * 64))))     # to_affine's rule
            assert grid == -(-(-(-total // r)) // 64)
        assert levels.value == max(1, -(-c // FAN_LOG2))
        assert [lanes[t] for t in range(levels.value)] == [count * 2 * q << max(0, c - FAN_LOG2 * (t + 1)) for t in range(levels.value)]
        assert lanes[levels.value - 1] == count * 2 * q
    assert lib.fk20c_plan_launch(1 << 31, 1, 1, 1, out, ctypes.byref(levels), lanes) == 1 and out[1] == 1 << 26 and out[4] == 1 << 25


@pytest.mark.parametrize("permute", [0, 1])
def test_buffer_sizes_match_what_the_lanes_address(lib, permute):
    shapes = [(16, cell, ext, 3) for cell in (1, 2, 4, 8, 16) for ext in (0, 1, 2, 3)]              # N = q, 2q, 4q, 8q for every cell size
    shapes += [(1, 1, 0, 1), (1, 1, 2, 70), (2, 1, 0, 257), (2, 2, 1, 5), (64, 8, 1, 2), (128, 8, 1, 3), (128, 64, 0, 3), (128, 128, 1, 2), (1024, 16, 2, 1),
               (4096, 64, 1, 2), (4096, 64, 0, 1), (4096, 64, 2, 1), (4096, 512, 1, 1), (4096, 1, 0, 2), (1 << 14, 4096, 1, 1)]
    for n, cell, ext, count in shapes:
        for h in (0, 1):
            if h and permute:
                continue
            assert lib.fk20c_plan_walk(n, cell, ext, count, permute, h) == 1, (n, cell, ext, count, h)


def test_the_largest_legal_sizes_stay_inside_64_bits(lib):
    s = sizes(lib, 1 << 31, 1, 1, 1 << 20)
    assert s["per_pass"] == 1 and s["passes"] == 1 << 20 and (s["log2n"], s["log2q"], s["log2cells"], s["log2w"]) == (31, 31, 32, 32)
    assert (s["scalars"], s["prod"], s["ws"], s["out"], s["tw_fwd"]) == (FR << 32, JAC << 32, JAC << 32, AFF << 32, FR << 31)
    s = sizes(lib, 1 << 31, 1 << 31, 1, 3)
    assert (s["log2q"], s["log2cells"], s["log2w"], s["ws"]) == (0, 1, 1, 2 * JAC) and s["prod"] == JAC << 32
    s = sizes(lib, 1, 1, 32, 1)
    assert (s["log2cells"], s["log2w"], s["ws"], s["out"]) == (32, 32, JAC << 32, AFF << 32)
    s = sizes(lib, 4096, 64, 20, 2)
    assert (s["log2cells"], s["log2w"]) == (26, 26) and s["per_pass"] == 1


def test_refused_sizes(lib):
    for n in (0, 3, 6, 255, (1 << 31) + 1, 1 << 32, 1 << 33):
        assert sizes(lib, n, 1, 0, 1) is None, n
    for cell in (0, 3, 6, 32, 1 << 40):
        assert sizes(lib, 16, cell, 0, 1) is None, cell
    assert sizes(lib, 16, 16, 0, 1) is not None and sizes(lib, 1, 1, 0, 1) is not None and sizes(lib, 1, 2, 0, 1) is None
    for n, ext in ((16, 29), (1 << 31, 2), (1, 33), (16, 1 << 40), (16, (1 << 64) - 1), (4096, 21)):
        assert sizes(lib, n, 4 if n > 4 else 1, ext, 1) is None, (n, ext)
    for n, ext in ((16, 28), (1 << 31, 1), (1, 32), (4096, 20)):
        assert sizes(lib, n, 1, ext, 1) is not None, (n, ext)
