"""The launch plan of batchVerify by message (csrc/plan.hpp slice_for_grouped), called from the product's header through
tests/host_emu/plan_bymsg.cpp: k == n names the ordinary path, the per-pair stages are what the batch path's deciders choose for k, the
per-set stages what slice_for chooses for n, and the table is a power of two of at least 2 n slots."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
SETS = ("nb", "pkmul_spread", "side", "pk_stream", "sig_stream", "cw", "nwin", "total", "lshift", "bucket_grid")
SIDE_NONE, SIDE_FORK, SIDE_FORK_SIG = 0, 1, 2


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_bymsg.sh"), "plan"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_bymsg.so"))
        u, sz, up = ctypes.c_uint, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint)
        L.plan_bymsg_min_shared.restype = sz
        L.plan_slice_for_grouped.argtypes = [u, ctypes.c_int, ctypes.c_int, sz, sz, up]
        L.plan_slice_for_words.argtypes = [u, ctypes.c_int, ctypes.c_int, sz, up]
        L.plan_lines_for_words.argtypes = [u, ctypes.c_int, u, u, up]
        L.plan_slice_for_grouped.restype = L.plan_slice_for_words.restype = L.plan_lines_for_words.restype = None
        _lib = L
    return _lib


def grouped(S, coop, side, n, k):
    out = (ctypes.c_uint * 31)()
    lib().plan_slice_for_grouped(S, coop, side, n, k, out)
    o = list(out)
    return {"ordinary": bool(o[0]), "table_slots": o[1], "grid_n": o[2], "grid_k": o[3], "sets": o[4:14], "hash_map": o[14:16], "clear": o[16:19],
            "extra_apart": o[19], "extra_lines": o[20:23], "lines": o[23:31]}


def ordinary(S, coop, side, n):
    out = (ctypes.c_uint * 27)()
    lib().plan_slice_for_words(S, coop, side, n, out)
    o = list(out)
    return {"sets": o[0:10], "hash_map": o[10:12], "clear": o[12:15], "extra_apart": o[15], "extra_lines": o[16:19], "lines": o[19:27]}


def lines_for(S, coop, npairs, extra):
    out = (ctypes.c_uint * 8)()
    lib().plan_lines_for_words(S, coop, npairs, extra, out)
    return list(out)


SLOTS = (1024, 416)                # the MI355X's wave slots at one wave per SIMD, and a smaller device
NS = (1, 2, 3, 64, 65, 130, 1000, 4096, 16384, 16385, 39999, 40000, 65536)


def ks_for(n):
    return sorted({k for k in (1, 2, 3, 7, 64, 65, 448, 449, n // 16, n // 2, n - 1, n) if 1 <= k <= n})


def test_the_threshold_hook_is_unset():
    assert lib().plan_bymsg_min_shared() == 0


@pytest.mark.parametrize("S", SLOTS)
@pytest.mark.parametrize("coop", [0, 1])
def test_grid_of_n_and_k(S, coop):
    for side in ((0, 1) if coop else (0,)):
        for n in NS:
            base_n = ordinary(S, coop, side, n)
            for k in ks_for(n):
                g = grouped(S, coop, side, n, k)
                assert g["ordinary"] == (k == n), (n, k)                         # nothing shared: run_pairs as it stands; anything shared: grouped
                t = g["table_slots"]
                assert t >= 2 * n and t & (t - 1) == 0, n
                assert g["grid_n"] == -(-n // 64) and g["grid_k"] == -(-k // 64)
                # the per-set stages: slice_for's for n, word for word
                assert g["sets"] == base_n["sets"], (n, k)
                total = dict(zip(SETS, g["sets"]))["total"]
                # the per-pair stages: what the batch path chooses for a batch of k
                base_k = ordinary(S, coop, side, k)
                assert g["hash_map"] == base_k["hash_map"] and g["clear"] == base_k["clear"], (n, k)
                # ... its lines too, wherever a batch of k has the same extra pairs on the same streams (the extra pairs and the fork are
                # decided by n: they belong to the signature side, which runs over all n sets)
                if base_k["sets"][2:8] == base_n["sets"][2:8]:
                    assert (g["extra_apart"], g["extra_lines"], g["lines"]) == (base_k["extra_apart"], base_k["extra_lines"], base_k["lines"]), (n, k)
                # ... and always lines_for's own answer for k tuple pairs in front of n's extra pairs
                assert g["extra_apart"] == base_n["extra_apart"] and g["extra_lines"] == base_n["extra_lines"], (n, k)
                want = lines_for(S, coop, k, 0) if g["extra_apart"] else lines_for(S, coop, k + total, total)
                assert g["lines"] == want, (n, k)


def test_small_k_takes_the_latency_forms():
    """65 536 sets of 128 messages on one caller's device: the hashing and the lines of the group pairs run on the lane-team engine, which a
    batch of 65 536 pairs is far too large for"""
    S = 1024
    big, g = ordinary(S, 1, 1, 65536), grouped(S, 1, 1, 65536, 128)
    assert big["clear"][0] == 0 and big["lines"][1] == 0                         # one lane per item
    assert g["clear"][0] == 1 and g["lines"][1] == 1 and g["lines"][0] == 128    # the engine
    assert g["hash_map"][0] == 0                                                 # HASH_MAP_ROWS
    assert g["sets"] == big["sets"]
