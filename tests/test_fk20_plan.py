"""csrc/plan.hpp's entry for the all-openings call (fk20_sizes_for / fk20_pass / fk20_launch_for, through tests/host_emu/plan_fk20.cpp): passes
are whole polynomials under the stated budget of 2n Jacobian images and 2n scalars each and cover [0, k) exactly once, one polynomial always
fits, the hook only shortens, the launches hold a lane for every slot, butterfly and run, the buffer sizes match what the lanes address, the
sizes of large calls stay inside 64 bits, and n = 0, 3 and 2^32 are refused."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32
CAP = 256 << 20
JAC, AFF, FR = 192, 96, 32             # bytes of an internal Jacobian image, of an affine image and of a scalar
PER_COEFF = 2 * (JAC + FR)             # 2n images and 2n scalars per polynomial
KEYS = ("log2n", "per_pass", "passes", "ws", "scalars", "polys", "out", "status", "tw_fr", "tw_inv", "tw_fwd", "cap")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_fk20.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_fk20.so"))
    L.fk20_plan_sizes.argtypes = [SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.fk20_plan_setup_bytes.argtypes = [SZ]
    L.fk20_plan_setup_bytes.restype = SZ
    L.fk20_plan_pass.argtypes = [SZ, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.fk20_plan_launch.argtypes = [SZ, SZ, ctypes.POINTER(U32)]
    L.fk20_plan_walk.argtypes = [SZ, SZ, ctypes.c_int]
    return L


def sizes(lib, n, k, forced=0):
    out = (SZ * 12)()
    if not lib.fk20_plan_sizes(n, k, forced, out):
        return None
    return dict(zip(KEYS, out))


@pytest.mark.parametrize("forced", [0, 1, 2, 100])
def test_passes_hold_whole_polynomials_and_cover_every_one_once(lib, forced):
    rule = lambda n: max(1, CAP // (PER_COEFF * n))          # noqa: E731
    for n in (1, 2, 128, 4096, 1 << 16, 1 << 19, 1 << 20, 1 << 24):
        for k in (1, 2, 5, 257, 2048, 2049):
            s = sizes(lib, n, k, forced)
            per = min(rule(n), forced or rule(n), k)
            assert s["cap"] == CAP and s["log2n"] == n.bit_length() - 1
            assert (s["tw_fr"], s["tw_inv"], s["tw_fwd"]) == (n * 32, n * 32, n // 2 * 32)
            assert s["per_pass"] == per and s["passes"] == -(-k // per) and s["status"] == 4 * per
            assert s["ws"] == per * 2 * n * JAC and s["scalars"] == per * 2 * n * FR and s["polys"] == per * n * FR and s["out"] == per * n * AFF
            assert s["ws"] + s["scalars"] <= CAP or per == 1                     # one polynomial always forms a pass, whatever its size
            out, got = (SZ * 2)(), []
            for i in range(s["passes"]):
                assert lib.fk20_plan_pass(n, k, forced, i, out) == 1
                got.append((out[0], out[1]))
            assert lib.fk20_plan_pass(n, k, forced, s["passes"], out) == 0
            assert got[0][0] == 0 and sum(c for _, c in got) == k and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:]))
            assert all(c == per for _, c in got[:-1]) and 1 <= got[-1][1] <= per


def test_the_hook_only_shortens(lib):
    assert sizes(lib, 1 << 20, 64, 1000)["per_pass"] == 1                    # 448 MiB a polynomial: the hook cannot lengthen a pass
    assert sizes(lib, 1 << 12, 1 << 20, 1 << 30)["per_pass"] == CAP // (PER_COEFF << 12) == 146
    assert sizes(lib, 8, 5, 2)["per_pass"] == 2 and sizes(lib, 8, 5, 7)["per_pass"] == 5
    assert sizes(lib, 8, 3, 1)["passes"] == 3 and sizes(lib, 8, 3, 2)["passes"] == 2


def test_launches_hold_a_lane_for_every_slot_butterfly_and_run(lib):
    out = (U32 * 6)()
    for n, count in ((1, 1), (1, 1000), (2, 1), (2, 257), (16, 257), (128, 64), (4096, 16), (1 << 16, 1), (1 << 20, 1), (1 << 31, 1)):
        assert lib.fk20_plan_launch(n, count, out) == 1
        circ, point, inv, fwd, run, finish = out
        half = n * count
        assert circ == -(-(count * -(-2 * n // 16)) // 256) and point == -(-2 * half // 64) and inv == -(-half // 64) and fwd == -(-(half // 2) // 64)
        assert 1 <= run <= 8 and run == min(8, max(1, -(-half // (256 * 4 * 64))))     # to_affine's rule
        assert finish == -(-(-(-half // run)) // 64)
    assert lib.fk20_plan_launch(1 << 31, 1, out) == 1 and out[1] == 1 << 26


@pytest.mark.parametrize("permute", [0, 1])
def test_buffer_sizes_match_what_the_lanes_address(lib, permute):
    for n, count in ((1, 1), (1, 70), (2, 1), (2, 257), (4, 3), (8, 3), (16, 257), (64, 2), (128, 3), (1024, 1), (4096, 2), (1 << 16, 1)):
        assert lib.fk20_plan_walk(n, count, permute) == 1, (n, count)


def test_large_calls_stay_inside_64_bits(lib):
    s = sizes(lib, 1 << 31, 1 << 20)
    assert s["per_pass"] == 1 and s["passes"] == 1 << 20 and s["ws"] == JAC << 32 and s["scalars"] == FR << 32 and s["out"] == AFF << 31 and s["log2n"] == 31


def test_refused_sizes(lib):
    for n in (0, 3, 6, 255, (1 << 31) + 1, 1 << 32, 1 << 33):
        assert sizes(lib, n, 1) is None and lib.fk20_plan_setup_bytes(n) == 0, n
    assert sizes(lib, 1 << 31, 1) is not None and sizes(lib, 1, 1)["log2n"] == 0
    assert sizes(lib, 4, 0)["passes"] == 0
    assert [lib.fk20_plan_setup_bytes(n) for n in (1, 2, 64, 1 << 31)] == [192, 384, 64 * 192, 192 << 31]
