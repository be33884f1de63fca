"""The device grouping of batchVerify by message (csrc/bymsg.hpp: insert, representative, ranking, offsets, scatter) executed on the CPU
through tests/host_emu/bymsg.cpp, against mi355_bls_group_by_message on the same records: the same groups in the same order, the members
of a group compared as sets.  Only the 32 message bytes of a record matter to either."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def emu():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_bymsg.sh"), "emu"])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libbymsg.so"))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L.emu_bymsg_table_slots.argtypes = [ctypes.c_size_t]
        L.emu_bymsg_table_slots.restype = ctypes.c_uint
        L.emu_bymsg_hash.argtypes = [ctypes.c_char_p]
        L.emu_bymsg_hash.restype = ctypes.c_uint
        L.emu_bymsg_group.argtypes = [ctypes.c_char_p, ctypes.c_size_t, u32p] + [u32p] * 6
        _lib = L
    return _lib


@pytest.fixture(scope="module")
def product():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package().lib()


def records(msgs):
    return b"".join(bytes(96) + m + bytes(192) for m in msgs)


def msg(tag):
    return hashlib.sha256(b"bymsg-%d" % tag).digest()


def device_groups(msgs, order=None):
    n = len(msgs)
    arr = lambda m: (ctypes.c_uint32 * max(m, 1))()
    slot_of, rep, gid, offsets, members, reps = arr(n), arr(n), arr(n), arr(n + 1), arr(n), arr(n)
    k = emu().emu_bymsg_group(records(msgs), n, (ctypes.c_uint32 * n)(*order) if order else None, slot_of, rep, gid, offsets, members, reps)
    assert k >= 1, "an index left its array"
    return k, list(rep[:n]), list(gid[:n]), list(offsets[:k + 1]), list(members[:n]), list(reps[:k]), list(slot_of[:n])


def host_groups(product, msgs):
    n = len(msgs)
    idx, offs, k = (ctypes.c_uint32 * n)(), (ctypes.c_size_t * (n + 1))(), ctypes.c_size_t()
    product.mi355_bls_group_by_message.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t),
                                                   ctypes.POINTER(ctypes.c_size_t)]
    assert product.mi355_bls_group_by_message(records(msgs), n, idx, offs, ctypes.byref(k)) == 0
    return [list(idx[offs[g]:offs[g + 1]]) for g in range(k.value)]


def check(product, msgs, order=None):
    n = len(msgs)
    want = host_groups(product, msgs)
    k, rep, gid, offsets, members, reps, slot_of = device_groups(msgs, order)
    assert k == len(want)
    assert offsets[0] == 0 and offsets[k] == n
    assert sorted(members) == list(range(n))                                   # the scatter is a permutation
    for g, grp in enumerate(want):
        assert offsets[g + 1] - offsets[g] == len(grp), g
        assert sorted(members[offsets[g]:offsets[g + 1]]) == grp, g               # as sets; the host's members are in input order
        assert reps[g] == grp[0] == min(grp), g                                   # the representative is the smallest index: first appearance
        for i in grp:
            assert rep[i] == grp[0] and gid[i] == g, i
    slots = emu().emu_bymsg_table_slots(n)
    assert all(s < slots for s in slot_of)
    return k


def test_table_size_is_a_power_of_two_of_at_least_2n():
    L = emu()
    assert L.emu_bymsg_table_slots(1) == 2                                       # the minimum
    for n in list(range(1, 300)) + [1100, 2200, 65536, 65537, (1 << 30)]:
        s = L.emu_bymsg_table_slots(n)
        assert s >= 2 * n and s & (s - 1) == 0 and (s < 4 * n or n == 1), n


def test_the_probe_hash_reads_every_word():
    """a message that differs from another in ONE byte, whichever, starts its probe elsewhere (no clustering by a shared prefix or suffix)"""
    L = emu()
    base = bytearray(msg(0))
    h0 = L.emu_bymsg_hash(bytes(base))
    seen = {h0 & 0xffff}
    for byte in range(32):
        m = bytearray(base)
        m[byte] ^= 1
        h = L.emu_bymsg_hash(bytes(m))
        assert h != h0, byte
        seen.add(h & 0xffff)
    assert len(seen) >= 30                                                      # 33 messages, a 65 536-slot table: a collision or two at the most


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 130])
def test_all_equal_and_all_distinct(product, n):
    assert check(product, [msg(7)] * n) == 1
    assert check(product, [msg(i) for i in range(n)]) == n


@pytest.mark.parametrize("byte", [0, 31])
def test_messages_that_differ_in_one_byte_only(product, byte):
    base = bytearray(msg(3))
    msgs = []
    for v in range(40):
        m = bytearray(base)
        m[byte] = v
        msgs += [bytes(m)] * (1 + v % 3)
    random.Random(byte).shuffle(msgs)
    assert check(product, msgs) == 40


def test_either_side_of_every_table_size_step_below_300(product):
    """the table doubles when 2 n passes a power of two: n = 2^j and 2^j + 1, with repeats so that both claims and joins happen"""
    L = emu()
    steps = [n for n in range(1, 300) if L.emu_bymsg_table_slots(n) != L.emu_bymsg_table_slots(n + 1)]
    assert steps == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    for s in steps:
        for n in (s, s + 1):
            rng = random.Random(n)
            assert check(product, [msg(i) for i in range(n)]) == n               # the table at its fullest: half the slots
            msgs = [msg(rng.randrange(max(1, n // 3))) for _ in range(n)]
            check(product, msgs)


def test_the_order_of_the_lanes_does_not_matter(product):
    """lanes insert in any order on the device: the groups, their order and their representatives are the same for every order"""
    rng = random.Random(5)
    msgs = [msg(rng.randrange(23)) for _ in range(200)]
    first = device_groups(msgs)
    for seed in range(4):
        order = list(range(200))
        random.Random(seed).shuffle(order)
        check(product, msgs, order)
        got = device_groups(msgs, order)
        assert got[:4] == first[:4] and got[5] == first[5]                        # k, rep, gid, offsets, reps: not the member order, not the slots
    check(product, msgs, list(reversed(range(200))))


def test_interleaved_group_sizes(product):
    sizes = [1, 2, 7, 8, 9]
    msgs = []
    for j in range(9):
        for g, s in enumerate(sizes):
            if j < s:
                msgs.append(msg(100 + g))
    assert check(product, msgs) == 5
