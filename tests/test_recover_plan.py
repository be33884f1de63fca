"""The plan of the threshold-signature recovery (csrc/plan.hpp recover_measure / recover_chunk_end / recover_fill / recover_sizes_for, through
tests/host_emu/recover.cpp): member range, chunks that end at group boundaries and never hold more than the chunk constant unless one group
alone does, a workspace that holds every product, partial and table entry of a chunk, and the refusals."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def L():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_recover.sh")])
    lib = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "librecover.so"))
    lib.recover_plan_measure.argtypes = [ctypes.POINTER(SZ), SZ, SZ, ctypes.POINTER(SZ)]
    lib.recover_plan_chunk_end.argtypes = [ctypes.POINTER(SZ), SZ, SZ, SZ]
    lib.recover_plan_chunk_end.restype = SZ
    lib.recover_plan_chunk.restype = SZ
    lib.recover_plan_sizes.argtypes = [ctypes.POINTER(SZ), SZ, SZ, ctypes.POINTER(SZ), ctypes.POINTER(SZ)]
    return lib


def offsets_of(lengths, first=0):
    offs = [first]
    for n in lengths:
        offs.append(offs[-1] + n)
    return offs


def measure(L, offs, chunk=0):
    out = (SZ * 5)()
    if L.recover_plan_measure((SZ * len(offs))(*offs), len(offs) - 1, chunk, out) != 1:
        return None
    return dict(zip(("lo", "members", "chunks", "max_members", "max_groups"), out))


def chunks_of(L, offs, chunk=0):
    arr, k, g0, out = (SZ * len(offs))(*offs), len(offs) - 1, 0, []
    while g0 < k:
        g1 = L.recover_plan_chunk_end(arr, k, g0, chunk)
        assert g0 < g1 <= k
        out.append((g0, g1))
        g0 = g1
    return out


def check(L, lengths, chunk=0, first=0):
    offs = offsets_of(lengths, first)
    cap = chunk or L.recover_plan_chunk()
    m = measure(L, offs, chunk)
    ch = chunks_of(L, offs, chunk)
    assert m["lo"] == (first if lengths else 0) and m["members"] == sum(lengths) and m["chunks"] == len(ch)
    for g0, g1 in ch:
        n = offs[g1] - offs[g0]
        assert n <= cap or g1 - g0 == 1                              # over the bound only as one group alone
        assert g1 - g0 <= cap
        if g1 < len(lengths):                                        # greedy: the next group did not fit
            assert offs[g1 + 1] - offs[g0] > cap or g1 - g0 == cap
    assert m["max_members"] == max([offs[b] - offs[a] for a, b in ch], default=0)
    assert m["max_groups"] == max([b - a for a, b in ch], default=0)
    return m, ch


def test_constant_is_a_memory_bound(L):
    assert L.recover_plan_chunk() == 65536                           # 24 MiB of 384-byte products


def test_sizes_and_chunking(L):
    cap = L.recover_plan_chunk()
    assert check(L, [3] * 300)[0] == {"lo": 0, "members": 900, "chunks": 1, "max_members": 900, "max_groups": 300}
    assert check(L, [3, 0, 10, 1], first=5)[0]["lo"] == 5
    m, ch = check(L, [3] * 21900)                                    # 65 700 members: the second chunk starts at a group boundary
    assert ch == [(0, 21845), (21845, 21900)] and m["max_members"] == 65535
    m, ch = check(L, [cap, 1])                                       # a total just over the chunk
    assert ch == [(0, 1), (1, 2)]
    m, ch = check(L, [cap - 1, 1, 1])
    assert ch == [(0, 2), (2, 3)]
    m, ch = check(L, [5, cap + 7, 5])                                # one group longer than the chunk is a chunk of its own
    assert ch == [(0, 1), (1, 2), (2, 3)] and m["max_members"] == cap + 7
    m, ch = check(L, [1 << 20])
    assert ch == [(0, 1)] and m["max_members"] == 1 << 20
    for chunk in (1, 2, 7, 16):                                      # small chunks, as the emulation walks them
        check(L, [3, 0, 0, 9, 1, 16, 17, 2, 2, 2, 0, 33], chunk)


def test_zero_groups_and_all_empty_groups(L):
    assert measure(L, [0]) == {"lo": 0, "members": 0, "chunks": 0, "max_members": 0, "max_groups": 0}
    m, ch = check(L, [0] * 10)
    assert m["members"] == 0 and ch == [(0, 10)]
    m, ch = check(L, [0] * 9, chunk=4)                               # empty groups have no members to count: the group count bounds a chunk
    assert ch == [(0, 4), (4, 8), (8, 9)]


def test_refusals(L):
    assert measure(L, [0, 5, 4]) is None                             # decreasing offsets
    assert measure(L, [0, (1 << 32) - 1]) is None                    # a position the 32-bit tables cannot address
    assert measure(L, [0, (1 << 32) - 2]) is not None                # nothing is refused for its size alone


def test_workspace_holds_a_chunk(L):
    lengths = [3, 0, 8, 9, 64, 65, 1, 2]
    offs = offsets_of(lengths, first=4)
    arr = (SZ * len(offs))(*offs)
    for g0, g1 in [(0, len(lengths)), (2, 6), (1, 2)]:
        sizes, items = (SZ * 7)(), SZ()
        assert L.recover_plan_sizes(arr, g0, g1, sizes, ctypes.byref(items)) == 1
        s = dict(zip(("prod", "part", "tab", "flags", "status", "out192", "out96"), sizes))
        m, kc = offs[g1] - offs[g0], g1 - g0
        want_items = 0
        for n in lengths[g0:g1]:
            while n > 0:
                n = (n + 7) // 8
                want_items += n
                if n == 1:
                    break
        assert items.value == want_items
        assert s == {"prod": max(m, 1) * 384, "part": max(want_items, 1) * 384, "tab": ((m + want_items) * 4 + 2 * kc) * 4, "flags": 4 * kc, "status": kc,
                     "out192": 192 * kc, "out96": 96 * kc}
