"""The staging layout of the grouped calls' host inputs (csrc/plan.hpp pack_for), called from the product's header through
tests/host_emu/plan_pack.cpp: every part starts on a multiple of 4 bytes, the parts keep their order and do not overlap, the total covers the
last one, and for the part lists the host forms pass (every length a multiple of 4 except the last) the offsets are the running sums the
entry points used to add up by hand.  And the per-row calls' staging (csrc/plan.hpp cols, ROW_COLUMNS): every column where the entry points
used to write it as a bare number, no two columns of a call overlapping but for the one declared sharing, every column inside its 320-byte row."""
import ctypes
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_pack.sh")])
        L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libplan_pack.so"))
        sz, szp = ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)
        L.plan_pack_parts_max.restype = sz
        L.plan_pack_for.restype, L.plan_pack_for.argtypes = sz, [szp, sz, szp]
        L.plan_row_bytes.restype = L.plan_row_column_count.restype = sz
        strp, u32p = ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint32)
        L.plan_row_column.restype, L.plan_row_column.argtypes = ctypes.c_int, [sz, strp, strp, strp, u32p, u32p, u32p]
        _lib = L
    return _lib


def pack(lengths):
    n = len(lengths)
    at = (ctypes.c_size_t * max(n, 1))()
    total = lib().plan_pack_for((ctypes.c_size_t * max(n, 1))(*lengths), n, at)
    return list(at)[:n], total


def check(lengths):
    at, total = pack(lengths)
    end = 0
    for a, ln in zip(at, lengths):
        assert a % 4 == 0, (lengths, at)
        assert a >= end, (lengths, at)                   # in order, no overlap
        assert a - end < 4, (lengths, at)                # and no more room lost than the alignment takes
        end = a + ln
    assert total >= end, (lengths, at, total)
    return at, total


LENGTHS = (0, 1, 3, 4, 5, 96, 192)


def test_the_aggregate_bits_call_fits():
    assert lib().plan_pack_parts_max() >= 6              # keys | signatures | messages | indices | committee aggregates | bits


@pytest.mark.parametrize("n", [1, 2, 3])
def test_every_list_of_the_edge_lengths(n):
    for lengths in itertools.product(LENGTHS, repeat=n):
        check(lengths)


def test_an_odd_part_in_the_middle():
    for odd in (1, 3, 5):
        for first, last in itertools.product(LENGTHS, repeat=2):
            at, _ = check((first, 96, odd, 192, last, 4))
            assert at[3] == at[2] + 4 * -(-odd // 4)     # the part behind the odd one starts on the next word
    assert pack((96, 5, 192)) == ([0, 96, 104], 300)
    assert pack((0, 1, 0, 3, 4, 5)) == ([0, 0, 4, 4, 8, 12], 21)


def test_no_parts():
    assert pack(()) == ([], 4)


def test_more_parts_than_the_layout_names_are_refused():
    most = lib().plan_pack_parts_max()
    assert pack((4,) * most)[1] == 4 * most + 4
    assert pack((4,) * (most + 1))[1] == 0               # total 0: no layout with parts has it


def running_sums(lengths):
    at, s = [], 0
    for ln in lengths:
        at.append(s)
        s += ln
    return at, s + 4                                     # what the entry points reserved: the parts and a word


def test_the_host_forms_part_lists_land_where_they_did():
    """the part lists of the six host forms, as each entry point listed them before there was a layout function"""
    n_table, k, n_idx, m, bits = 80, 3, 10, 5, 7
    cases = {
        # aggregate_sets: keys | signatures | messages | indices
        "aggregate_sets": ((n_table * 96, k * 192, k * 32, n_idx * 4), [0, 7680, 8256, 8352], 8396),
        "aggregate_sets, no indices": ((n_table * 96, k * 192, k * 32, 0), [0, 7680, 8256, 8352], 8356),
        "aggregate_sets, empty table": ((0, k * 192, k * 32, n_idx * 4), [0, 0, 576, 672], 716),
        # aggregate_sets_bits: ... | committee aggregates, packed | bits (byte-aligned, last)
        "aggregate_sets_bits": ((n_table * 96, k * 192, k * 32, n_idx * 4, m * 96, bits), [0, 7680, 8256, 8352, 8392, 8872], 8883),
        "aggregate_sets_bits, no aggregates": ((n_table * 96, k * 192, k * 32, 0, 0, bits), [0, 7680, 8256, 8352, 8352, 8352], 8363),
        # aggregate_verify_each: keys | signatures | messages by position | indices
        "aggregate_verify_each": ((n_table * 96, k * 192, n_idx * 32, n_idx * 4), [0, 7680, 8256, 8576], 8620),
        # aggregate_signature_sets: signatures | indices
        "aggregate_signature_sets": ((n_table * 192, n_idx * 4), [0, 15360], 15404),
        # recover_signature_sets: signatures | ids | indices
        "recover_signature_sets": ((n_table * 192, n_idx * 32, n_idx * 4), [0, 15360, 15680], 15724),
        # combine_sets: records | indices
        "combine_sets": ((n_table * 320, n_idx * 4), [0, 25600], 25644),
    }
    for name, (lengths, want_at, want_total) in cases.items():
        assert running_sums(lengths) == (want_at, want_total), name      # the figures written out above are the old sums
        assert pack(lengths) == (want_at, want_total), name


# ---- the per-row calls' staging columns

def row_columns():
    """[(call, buffer, column, start, width, shares)] as csrc/plan.hpp lists them"""
    out = []
    for i in range(lib().plan_row_column_count()):
        call, column, shares = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_char_p()
        buf, start, width = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert lib().plan_row_column(i, call, column, shares, buf, start, width) == 1
        out.append((call.value.decode(), ("d_comp", "d_sets")[buf.value], column.value.decode(), start.value, width.value,
                    shares.value.decode() if shares.value else None))
    return out


# (call, buffer, column): (start, width) - the figures the entry points carried as `cap_io * K` and `n * W` before there was a table
ROW_COLUMNS = {
    ("compress_public_keys", "d_comp", "keys in"): (0, 96),
    ("compress_public_keys", "d_comp", "out"): (96, 48),
    ("compress_signatures", "d_comp", "signatures in"): (0, 192),
    ("compress_signatures", "d_comp", "out"): (192, 96),
    ("deserialize_signatures", "d_comp", "wire"): (0, 192),
    ("deserialize_public_keys", "d_comp", "wire"): (0, 96),
    ("pop_verify", "d_comp", "keys"): (0, 96),
    ("pop_verify", "d_comp", "proofs"): (96, 192),
    ("admit_keys", "d_comp", "decoded keys"): (0, 96),
    ("admit_keys", "d_comp", "decoded proofs"): (96, 192),
    ("admit_keys", "d_comp", "row list"): (288, 4),
    ("admit_keys", "d_comp", "proof status"): (292, 1),
    ("admit_keys", "d_sets", "wire keys"): (0, 96),
    ("admit_keys", "d_sets", "wire proofs"): (96, 192),
    ("deserialize_sets", "d_comp", "keys"): (0, 96),
    ("deserialize_sets", "d_comp", "messages"): (96, 32),
    ("deserialize_sets", "d_comp", "signatures"): (128, 192),
    ("sign_sets", "d_comp", "scalars"): (0, 32),
    ("sign_sets", "d_comp", "messages"): (48, 32),
    ("pop_prove", "d_comp", "keys out"): (0, 96),
    ("pop_prove", "d_comp", "proofs out"): (96, 192),
    ("pop_prove", "d_comp", "scalars"): (288, 32),
    ("pop_prove", "d_comp", "zero messages"): (96, 32),           # the device form's: they share the proofs' column
}
ROW_SHARINGS = {("pop_prove", "d_comp", frozenset(("zero messages", "proofs out")))}


def test_the_row_is_320_bytes():
    assert lib().plan_row_bytes() == 320
    assert lib().plan_row_column(lib().plan_row_column_count(), *([None] * 6)) == 0


def test_every_row_column_lands_where_it_did():
    got = {(call, buf, column): (start, width) for call, buf, column, start, width, _ in row_columns()}
    assert len(got) == lib().plan_row_column_count()         # no (call, buffer, column) twice
    assert got == ROW_COLUMNS


def test_row_columns_of_a_call_do_not_overlap():
    cols = row_columns()
    declared = set()
    for call, buf, column, _, _, shares in cols:
        if shares is not None:
            assert any(c == call and b == buf and name == shares for c, b, name, _, _, _ in cols), (call, column, shares)
            declared.add((call, buf, frozenset((column, shares))))
    assert declared == ROW_SHARINGS
    overlapping = set()
    for (c1, b1, n1, s1, w1, _), (c2, b2, n2, s2, w2, _) in itertools.combinations(cols, 2):
        if (c1, b1) == (c2, b2) and s1 < s2 + w2 and s2 < s1 + w1:
            overlapping.add((c1, b1, frozenset((n1, n2))))
    assert overlapping == ROW_SHARINGS                       # the declared sharing is a real one, and the only overlap


def test_every_row_column_ends_inside_the_row():
    for call, buf, column, start, width, _ in row_columns():
        assert width > 0 and start + width <= 320, (call, buf, column)
    # the two that end exactly at the row's end
    assert sum(ROW_COLUMNS[("pop_prove", "d_comp", "scalars")]) == 320 and sum(ROW_COLUMNS[("deserialize_sets", "d_comp", "signatures")]) == 320
