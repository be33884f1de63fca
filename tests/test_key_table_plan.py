"""The two host decisions of key admission (csrc/plan.hpp admit_survivors / admit_merge), executed through tests/host_emu/plan_keytable.cpp:
the survivor list is exactly the rows both decoders accepted, in row order; the merged status is the key's failure before the proof's before
a refused proof (8); the rows to zero are exactly the refused ones whose key decoded - for all rows surviving, none, alternating, 63 / 64 / 65 survivors and a
table one row above a slice."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SLICE = 64


@pytest.fixture(scope="module")
def pl():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_keytable.sh"), "plan"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_keytable.so"))
    cp, sz, u32p = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)
    for f in (L.keytable_plan_bad_proof, L.keytable_plan_gather_threads, L.keytable_plan_record_blocks, L.keytable_plan_zero_blocks):
        f.restype = ctypes.c_uint32
    L.keytable_plan_record_blocks.argtypes = L.keytable_plan_zero_blocks.argtypes = [sz]
    L.keytable_plan_survivors.argtypes = [cp, cp, sz, u32p]
    L.keytable_plan_survivors.restype = sz
    L.keytable_plan_merge.argtypes = [cp, cp, sz, u32p, cp, sz, cp, u32p]
    L.keytable_plan_merge.restype = sz
    return L


def survivors(L, key_st, proof_st):
    n = len(key_st)
    lst = (ctypes.c_uint32 * (n + 1))(*([0xdeadbeef] * (n + 1)))
    m = L.keytable_plan_survivors(bytes(key_st), bytes(proof_st), n, lst)
    assert list(lst)[m:] == [0xdeadbeef] * (n + 1 - m)                       # nothing written past the survivors
    return list(lst)[:m]


def merge(L, key_st, proof_st, lst, verdicts):
    n, m = len(key_st), len(lst)
    status, zero = ctypes.create_string_buffer(n + 1), (ctypes.c_uint32 * (n + 1))(*([0xdeadbeef] * (n + 1)))
    status.raw = b"\xee" * (n + 1)
    nz = L.keytable_plan_merge(bytes(key_st), bytes(proof_st), n, (ctypes.c_uint32 * max(m, 1))(*lst), bytes(verdicts), m, status, zero)
    assert status.raw[n] == 0xee and list(zero)[nz:] == [0xdeadbeef] * (n + 1 - nz)
    return status.raw[:n], list(zero)[:nz]


def check(L, key_st, proof_st, verdict_of):
    """verdict_of(row) for the surviving rows -> the merged status, checked against the contract written out"""
    n = len(key_st)
    lst = survivors(L, key_st, proof_st)
    assert lst == [i for i in range(n) if key_st[i] == 0 and proof_st[i] == 0]
    verdicts = [verdict_of(i) for i in lst]
    status, bad = merge(L, key_st, proof_st, lst, verdicts)
    want = [key_st[i] if key_st[i] else proof_st[i] if proof_st[i] else (0 if verdict_of(i) == 1 else 8) for i in range(n)]
    assert list(status) == want
    assert bad == [i for i in range(n) if want[i] != 0 and key_st[i] == 0]     # the rows the key decoder left an image in
    return lst, status, bad


def test_constants_and_grids(pl):
    assert pl.keytable_plan_bad_proof() == 8 and pl.keytable_plan_gather_threads() == 256
    for m in (0, 1, 3, 4, 63, 64, 65, 4097, 1 << 20, 1 << 30):
        assert pl.keytable_plan_record_blocks(m) == -(-m * 80 // 256)          # a thread per word of m 80-word records, none short
        assert pl.keytable_plan_zero_blocks(m) == -(-m * 24 // 256)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, SLICE + 1, 150))
def test_all_none_alternating(pl, n):
    ok, one = [0] * n, lambda i: 1
    lst, status, bad = check(pl, ok, ok, one)
    assert lst == list(range(n)) and status == bytes(n) and bad == []
    lst, status, bad = check(pl, [1] * n, ok, one)                               # no survivors
    assert lst == [] and status == b"\x01" * n and bad == []
    lst, status, bad = check(pl, ok, [5] * n, one)
    assert lst == [] and status == b"\x05" * n and bad == list(range(n))       # the keys decoded: every row is zeroed
    for phase in (0, 1):
        ks = [0 if i % 2 == phase else 3 for i in range(n)]
        lst, status, bad = check(pl, ks, ok, one)
        assert lst == list(range(phase, n, 2)) and bad == []
        lst, status, bad = check(pl, ks, ok, lambda i: 0)                        # every survivor refused
        assert bad == lst and all(status[i] == 8 for i in lst)


@pytest.mark.parametrize("m", (63, 64, 65))
def test_survivor_counts_around_a_wave(pl, m):
    n = 200
    ks = [0 if 7 <= i < 7 + m else 1 + i % 3 for i in range(n)]
    ps = [0 if i % 5 else 4 for i in range(n)]
    lst, status, bad = check(pl, ks, ps, lambda i: i % 7 != 0)
    assert len(lst) == m - len([i for i in range(7, 7 + m) if i % 5 == 0])
    ps = [0] * n
    lst, status, bad = check(pl, ks, ps, lambda i: 1)
    assert len(lst) == m and lst[0] == 7 and lst[-1] == 6 + m


def test_precedence(pl):
    """a key failure hides a proof failure, which hides a bad verdict"""
    ks = [0, 1, 2, 3, 0, 0, 1, 2, 3, 0]
    ps = [0, 0, 0, 0, 4, 5, 4, 5, 4, 0]
    lst, status, bad = check(pl, ks, ps, lambda i: 0)                            # every verdict there is is bad
    assert lst == [0, 9] and list(status) == [8, 1, 2, 3, 4, 5, 1, 2, 3, 8] and bad == [0, 4, 5, 9]
    # a verdict byte other than 1 is a refusal (the per-pair pass writes 0 or 1)
    status, bad = merge(pl, [0, 0], [0, 0], [0, 1], [1, 2])
    assert list(status) == [0, 8] and bad == [1]
    # rows that did not survive are never touched by a verdict
    status, bad = merge(pl, [1, 0, 0], [4, 5, 0], [2], [0])
    assert list(status) == [1, 5, 8] and bad == [1, 2]

