"""csrc/plan.hpp's entry for the short linear combinations (lincomb_measure / lincomb_chunk_end / lincomb_sizes_for, through
tests/host_emu/lincomb.cpp): the chunk rule never splits a group and covers every group once, and the workspace is sized by a chunk."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t
G1_JAC, G2_JAC = 3 * 16 * 4, 6 * 16 * 4      # bytes of an internal Jacobian image (kernels.hip G1W, G2W words)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_lincomb.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "liblincomb.so"))
    P = ctypes.POINTER(SZ)
    L.lincomb_plan_measure.argtypes = [P, SZ, SZ, P]
    L.lincomb_plan_chunk_end.argtypes = [P, SZ, SZ, SZ]
    L.lincomb_plan_chunk_end.restype = SZ
    L.lincomb_plan_chunk.argtypes = [SZ]
    L.lincomb_plan_chunk.restype = SZ
    L.lincomb_plan_sizes.argtypes = [P, SZ, SZ, ctypes.c_int, P, P]
    return L


def offsets_of(lens, first=0):
    o = [first]
    for n in lens:
        o.append(o[-1] + n)
    return o


def walk(lib, offsets, forced):
    k = len(offsets) - 1
    arr = (SZ * (k + 1))(*offsets)
    chunks, g0 = [], 0
    while g0 < k:
        g1 = lib.lincomb_plan_chunk_end(arr, k, g0, forced)
        chunks.append((g0, g1))
        g0 = g1
    return chunks


def test_the_constant_and_the_hook(lib):
    assert lib.lincomb_plan_chunk(0) == 65536 and lib.lincomb_plan_chunk(16) == 16 and lib.lincomb_plan_chunk(1) == 1


@pytest.mark.parametrize("forced", [0, 1, 16, 100])
def test_chunks_hold_whole_groups_and_cover_every_group_once(lib, forced):
    rng = random.Random(forced)
    cases = [[0, 1, 2, 3, 8, 9, 64, 65], [65, 64, 0, 0, 1], [0] * 40, [1] * 70, [16, 16, 17, 15, 1], [200000], [70000, 3, 70000], [2] * 40000]
    cases += [[rng.choice((0, 1, 2, 3, 5, 17, 64)) for _ in range(rng.randrange(1, 60))] for _ in range(20)]
    chunk = lib.lincomb_plan_chunk(forced)
    for lens in cases:
        offsets = offsets_of(lens, first=rng.randrange(4))
        k = len(lens)
        chunks = walk(lib, offsets, forced)
        assert chunks[0][0] == 0 and chunks[-1][1] == k and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))      # every group once, in order
        out = (SZ * 5)()
        assert lib.lincomb_plan_measure((SZ * (k + 1))(*offsets), k, forced, out) == 1
        assert list(out)[:3] == [offsets[0], offsets[-1] - offsets[0], len(chunks)]
        for g0, g1 in chunks:
            terms, groups = offsets[g1] - offsets[g0], g1 - g0
            assert groups >= 1 and groups <= max(chunk, 1)
            assert terms <= chunk or groups == 1                                    # a group longer than a chunk is a chunk of its own, never split
            assert terms <= out[3] and groups <= out[4]                             # the workspace is the largest chunk's
            if g1 < k:                                                              # greedy: the next group did not fit
                assert groups == chunk or offsets[g1 + 1] - offsets[g0] > chunk
        assert out[3] == max(offsets[b] - offsets[a] for a, b in chunks) and out[4] == max(b - a for a, b in chunks)


def test_workspace_of_a_chunk(lib):
    lens = [0, 1, 2, 3, 8, 9, 64, 65]
    offsets = offsets_of(lens, first=5)
    arr = (SZ * len(offsets))(*offsets)
    sizes, items = (SZ * 6)(), SZ()
    for g2, jac, row in ((0, G1_JAC, 96), (1, G2_JAC, 192)):
        assert lib.lincomb_plan_sizes(arr, 0, len(lens), g2, sizes, ctypes.byref(items)) == 1
        n_items = sum((n + 7) // 8 for n in lens) + (1 + 1 + 2) + 1                  # level 0; 9, 64 and 65 terms have a level 1, 65 a level 2
        assert items.value == n_items
        assert list(sizes) == [152 * jac, n_items * jac, ((152 + n_items) * 4 + 2 * 8) * 4, 8 * 4, 8, 8 * row]
        assert lib.lincomb_plan_sizes(arr, 0, 1, g2, sizes, ctypes.byref(items)) == 1     # an empty chunk keeps one product and one partial
        assert items.value == 0 and list(sizes) == [jac, jac, 2 * 4, 4, 1, row]


def test_refused_offsets(lib):
    out = (SZ * 5)()
    assert lib.lincomb_plan_measure((SZ * 3)(0, 2, 1), 2, 0, out) == 0
    assert lib.lincomb_plan_measure((SZ * 2)(0, (1 << 32) - 1), 1, 0, out) == 0
    assert lib.lincomb_plan_measure((SZ * 2)(0, (1 << 32) - 2), 1, 0, out) == 1 and out[2] == 1
