"""mi355_bls_group_by_message (host only, no GPU): the records of a flat batch grouped by their 32-byte message - stable, groups in the order
their message first appears, members in input order."""
import ctypes
import hashlib
import random

import pytest


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def records(msg_ids):
    """records that differ in every part, message = a function of the id"""
    return b"".join(hashlib.sha256(b"pk %d" % i).digest() * 3 + hashlib.sha256(b"m %d" % g).digest() + hashlib.sha256(b"sig %d" % i).digest() * 6
                    for i, g in enumerate(msg_ids))


def reference(msg_ids):
    order, members = [], {}
    for i, g in enumerate(msg_ids):
        if g not in members:
            order.append(g)
            members[g] = []
        members[g].append(i)
    idx, offsets = [], [0]
    for g in order:
        idx += members[g]
        offsets.append(len(idx))
    return idx, offsets


def test_stable_and_in_order_of_first_appearance(m):
    rng = random.Random(11)
    ids = [rng.randrange(40) for _ in range(1000)]
    assert m.groupByMessage(records(ids)) == reference(ids)
    assert m.groupByMessage(records([3, 1, 3, 2, 1, 3])) == ([0, 2, 5, 1, 4, 3], [0, 3, 5, 6])


def test_all_distinct_all_equal_and_empty(m):
    assert m.groupByMessage(records(list(range(50)))) == (list(range(50)), list(range(51)))
    assert m.groupByMessage(records([7] * 50)) == (list(range(50)), [0, 50])
    assert m.groupByMessage(b"") == ([], [0])


def test_only_the_message_bytes_count(m):
    a = bytearray(records([0, 0, 0]))
    a[95] ^= 1          # last byte of a key
    a[320 + 128] ^= 1   # first byte of a signature
    assert m.groupByMessage(bytes(a)) == ([0, 1, 2], [0, 3])
    a[640 + 96 + 31] ^= 1                                            # last byte of a message
    assert m.groupByMessage(bytes(a)) == ([0, 1, 2], [0, 2, 3])


def test_argument_errors(m):
    L = m.lib()
    sz = ctypes.c_size_t
    idx, offs, k = (ctypes.c_uint32 * 2)(), (sz * 3)(), sz(9)
    rec = records([0, 1])
    assert L.mi355_bls_group_by_message(rec, 2, idx, offs, ctypes.byref(k)) == 0 and k.value == 2
    assert L.mi355_bls_group_by_message(None, 2, idx, offs, ctypes.byref(k)) == -3
    assert L.mi355_bls_group_by_message(rec, 2, None, offs, ctypes.byref(k)) == -3
    assert L.mi355_bls_group_by_message(rec, 2, idx, None, ctypes.byref(k)) == -3
    assert L.mi355_bls_group_by_message(rec, 2, idx, offs, None) == -3
    assert L.mi355_bls_group_by_message(None, 0, None, offs, ctypes.byref(k)) == 0 and k.value == 0 and offs[0] == 0
