"""csrc/plan.hpp's entry for the transforms over Fr (frntt_sizes_for / frntt_slice / frntt_geo_for, through tests/host_emu/frntt.cpp): the
passes' stages sum to log2 n and none exceeds the tile, slices are whole vectors and cover [0, k) exactly once, the hooks only shrink, the
shape of a pass covers every element once, and the sizes of large calls stay inside 64 bits."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32
CAP = 256 << 20


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_frntt.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libfrntt.so"))
    L.frntt_plan_sizes.argtypes = [SZ, SZ, U32, SZ, ctypes.POINTER(SZ), ctypes.POINTER(ctypes.c_uint8)]
    L.frntt_plan_slice.argtypes = [SZ, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    L.frntt_plan_geo.argtypes = [U32, U32, U32, U32, SZ, ctypes.POINTER(ctypes.c_uint64)]
    L.frntt_plan_geo.restype = None
    L.frntt_plan_tile.restype = U32
    L.frntt_plan_tile_max.restype = U32
    return L


def sizes(lib, n, k, tile=0, vecs=0):
    out, stages = (SZ * 8)(), (ctypes.c_uint8 * 32)()
    if not lib.frntt_plan_sizes(n, k, tile, vecs, out, stages):
        return None
    s = dict(zip(("log2n", "tile", "passes", "vecs", "slices", "twiddles", "status", "staging"), out))
    s["stages"] = list(stages)[:s["passes"]]
    return s


def test_the_constants(lib):
    assert lib.frntt_plan_tile() in (10, 12) and lib.frntt_plan_tile_max() == 12


@pytest.mark.parametrize("tile", [0, 2, 3, 10, 12])
def test_the_stages_of_the_passes(lib, tile):
    t = tile or lib.frntt_plan_tile()
    for m in range(0, 33):
        s = sizes(lib, 1 << m, 3, tile)
        assert s["log2n"] == m and s["tile"] == t and s["passes"] == -(-m // t) == len(s["stages"])
        assert sum(s["stages"]) == m and all(1 <= x <= t for x in s["stages"])
        assert s["stages"] == sorted(s["stages"], reverse=True) and (not s["stages"] or s["stages"][0] - s["stages"][-1] <= 1)
        assert s["twiddles"] == (1 << m) // 2 * 32
    assert [sizes(lib, n, 1, 2)["stages"] for n in (4, 8, 16, 64)] == [[2], [2, 1], [2, 2], [2, 2, 2]]
    d = lib.frntt_plan_tile()
    assert [sizes(lib, n, 1)["passes"] for n in (1, 2, 4, 256, 512, 1 << d, 2 << d)] == [0, 1, 1, 1, 1, 1, 2]


@pytest.mark.parametrize("forced", [0, 1, 2, 100])
def test_slices_hold_whole_vectors_and_cover_every_one_once(lib, forced):
    rule = lambda n: max(1, min(1 << 20, CAP // (32 * n)))          # noqa: E731
    for n in (1, 2, 256, 4096, 1 << 16, 1 << 20, 1 << 23, 1 << 24):
        for k in (1, 2, 5, 257, 2048, 2049):
            s = sizes(lib, n, k, 0, forced)
            per = min(rule(n), forced or rule(n), k)
            assert s["vecs"] == per and s["slices"] == -(-k // per) and s["status"] == per * 4 and s["staging"] == per * n * 32
            out, got = (SZ * 2)(), []
            for i in range(s["slices"]):
                assert lib.frntt_plan_slice(n, k, forced, i, out) == 1
                got.append((out[0], out[1]))
            assert lib.frntt_plan_slice(n, k, forced, s["slices"], out) == 0
            assert got[0][0] == 0 and sum(c for _, c in got) == k and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:]))
            assert all(c == per for _, c in got[:-1]) and 1 <= got[-1][1] <= per


def test_the_hooks_only_shrink(lib):
    assert sizes(lib, 1 << 20, 1, 13)["tile"] == sizes(lib, 1 << 20, 1, 200)["tile"] == lib.frntt_plan_tile_max()      # never above what the LDS holds
    assert sizes(lib, 1 << 20, 1, 2)["tile"] == 2 and sizes(lib, 1 << 20, 1, 1)["passes"] == 20
    assert sizes(lib, 1 << 20, 64, 0, 1000)["vecs"] == 8                                                              # 256 MiB a slice: the hook cannot lengthen it
    assert sizes(lib, 8, 5, 0, 2)["vecs"] == 2 and sizes(lib, 1, 1 << 21, 0, 1 << 30)["vecs"] == 1 << 20


def test_large_calls_stay_inside_64_bits(lib):
    s = sizes(lib, 1 << 32, 1 << 20)
    assert s["vecs"] == 1 and s["slices"] == 1 << 20 and s["staging"] == 1 << 37 and s["twiddles"] == 1 << 36 and s["log2n"] == 32
    assert sum(s["stages"]) == 32
    s = sizes(lib, 1 << 12, 1 << 20)
    assert s["vecs"] == 2048 and s["slices"] == 512 and s["staging"] == CAP


def test_refused_sizes(lib):
    for n in (0, 3, 6, 255, (1 << 32) + 1, 1 << 33):
        assert sizes(lib, n, 1) is None, n
    assert sizes(lib, 1 << 32, 1) is not None and sizes(lib, 1, 1)["passes"] == 0
    assert sizes(lib, 4, 0)["slices"] == 0


def test_the_shape_of_a_pass(lib):
    out = (ctypes.c_uint64 * 4)()
    for m, tile, sigma, tp, vecs in ((16, 10, 8, 8, 1), (16, 10, 0, 8, 1), (20, 10, 10, 10, 3), (3, 2, 1, 2, 3), (3, 2, 0, 1, 3), (1, 10, 0, 1, 257), (8, 10, 0, 8, 3),
                                     (32, 10, 24, 8, 1)):
        lib.frntt_plan_geo(m, tile, sigma, tp, vecs, out)
        clo, chi, L, wgs = out
        blocks = vecs << (m - sigma - tp)
        assert clo == min(tile - tp, sigma) and L == clo + tp + chi <= tile and chi <= tile - tp - clo
        assert (1 << chi) >= min(blocks, 1 << (tile - tp - clo))                      # no room left unused while blocks wait
        assert wgs == -(-blocks // (1 << chi)) << (sigma - clo) and wgs << L >= vecs << m      # every element has a slot
