"""csrc/plan.hpp's entry for the openings over Fr (fropen_sizes_for / fropen_pass, through tests/host_emu/plan_fropen.cpp): passes are whole
polynomials and cover [0, k) exactly once, the hook's pass size is honoured, the workspace is sized by a pass, and the sizes of large calls stay
inside 64 bits."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_fropen.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libfropen.so"))
    P = ctypes.POINTER(SZ)
    L.fropen_plan_sizes.argtypes = [SZ, SZ, ctypes.c_int, SZ, P]
    L.fropen_plan_pass.argtypes = [SZ, SZ, ctypes.c_int, SZ, SZ, P]
    L.fropen_plan_polys_pass.restype = SZ
    L.fropen_plan_scan_bytes.restype = SZ
    return L


def sizes(lib, n, k, ev, forced=0):
    out = (SZ * 8)()
    if not lib.fropen_plan_sizes(n, k, ev, forced, out):
        return None
    return dict(zip(("per_pass", "passes", "log2n", "domain", "scan", "status", "out_ys", "out_quot"), out))


def passes(lib, n, k, ev, forced=0):
    s, out, got = sizes(lib, n, k, ev, forced), (SZ * 2)(), []
    for p in range(s["passes"]):
        assert lib.fropen_plan_pass(n, k, ev, forced, p, out) == 1
        got.append((out[0], out[1]))
    assert lib.fropen_plan_pass(n, k, ev, forced, s["passes"], out) == 0
    return s, got


def test_the_constants(lib):
    assert lib.fropen_plan_polys_pass() == 65536 and lib.fropen_plan_scan_bytes() == 256 << 20


@pytest.mark.parametrize("ev", [0, 1])
@pytest.mark.parametrize("forced", [0, 1, 2, 100])
def test_passes_hold_whole_polynomials_and_cover_every_one_once(lib, ev, forced):
    rule = lambda n: max(1, min(65536, (256 << 20) // (32 * n)))          # noqa: E731
    for n in (1, 2, 256, 4096, 1 << 16, 1 << 20, 1 << 23, 1 << 24) + (() if ev else (3, 255, 257, 5000)):
        for k in (1, 2, 5, 257, 2048, 2049) + ((65536, 65537, 200001) if not forced and n <= 4096 else ()):
            s, got = passes(lib, n, k, ev, forced)
            per = min(rule(n), forced or rule(n), k)
            assert s["per_pass"] == per and s["passes"] == len(got) == -(-k // per), (n, k)
            assert got[0][0] == 0 and sum(c for _, c in got) == k                      # [0, k) ...
            assert all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:]))              # ... exactly once, in order
            assert all(c == per for _, c in got[:-1]) and 1 <= got[-1][1] <= per       # counts of polynomials: never a part of one
            assert s["status"] == per and s["out_ys"] == per * 32 and s["out_quot"] == per * n * 32
            assert (s["domain"], s["scan"]) == ((n * 32, per * n * 32) if ev else (0, 0))
            assert s["log2n"] == (n.bit_length() - 1 if ev else 0)


def test_the_forced_pass_is_honoured_and_only_shortens(lib):
    assert sizes(lib, 8, 5, 0, 2)["per_pass"] == 2 and passes(lib, 8, 5, 1, 2)[1] == [(0, 2), (2, 2), (4, 1)]
    assert sizes(lib, 1 << 20, 64, 1, 1000)["per_pass"] == 8                          # 256 MiB of scan: the hook cannot lengthen a pass
    assert sizes(lib, 1, 1 << 20, 0, 1 << 19)["per_pass"] == 65536


def test_large_calls_stay_inside_64_bits(lib):
    for ev in (0, 1):
        s = sizes(lib, 1 << 26, 1 << 20, ev)
        assert s["per_pass"] == 1 and s["passes"] == 1 << 20 and s["out_quot"] == 1 << 31 and s["scan"] == (ev << 31) and s["domain"] == (ev << 31)
        s = sizes(lib, 1 << 12, 1 << 20, ev)
        assert s["per_pass"] == 2048 and s["passes"] == 512 and s["out_quot"] == 256 << 20
    s = sizes(lib, 1 << 32, 3, 1)                                                      # the longest domain: a pass of one, 128 GiB of scan asked for
    assert s["per_pass"] == 1 and s["scan"] == 1 << 37 and s["log2n"] == 32


def test_refused_sizes(lib):
    assert sizes(lib, 0, 1, 0) is None and sizes(lib, 0, 1, 1) is None
    for n in (3, 255, 257, 6, (1 << 32) + 1, 1 << 33):
        assert sizes(lib, n, 1, 1) is None and sizes(lib, n, 1, 0) is not None
    assert sizes(lib, 1 << 32, 1, 1) is not None and sizes(lib, 1, 1, 1)["log2n"] == 0
    assert sizes(lib, 4, 0, 1)["passes"] == 0                                          # k == 0: nothing to walk
