"""The item bodies of the key aggregation by participation bits (csrc/aggbits.hpp: the mode of a set, the level-0 sums of the keys its bits
select or leave out, the subtraction from the committee's aggregate) executed on the CPU under the bounds tracker
(tests/host_emu/aggbits.cpp), over the tables of the product's own plan, for every set of tests/golden/aggregate_bits.json: records, status
bytes and route counts equal to the fixture with the committee aggregates at a stride of 96 and of 320 and without them, and the keys equal
to the C restatement's sum of the participants."""
import ctypes
import os
import subprocess

import pytest

import c_oracle as co
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture_inputs(fx=None, which_sets=None):
    """-> dict of the fixture's call: table, idx, c_offsets, aggs (packed, 96 bytes apart), which, bits, msgs, sigs, and the expected
    records, status bytes, verdicts and routes; which_sets: only these sets, in this order"""
    fx = fx or golden("aggregate_bits")
    sets = fx["sets"] if which_sets is None else [fx["sets"][i] for i in which_sets]
    return {"table": bytes.fromhex(fx["table"]), "idx": list(fx["idx"]), "c_offsets": list(fx["c_offsets"]),
            "aggs": b"".join(bytes.fromhex(c["aggregate"]) for c in fx["committees"]),
            "which": [s["committee"] for s in sets], "bits": [bytes.fromhex(s["bits"]) for s in sets],
            "msgs": b"".join(bytes.fromhex(s["message"]) for s in sets), "sigs": b"".join(bytes.fromhex(s["signature"]) for s in sets),
            "want": b"".join(bytes.fromhex(s["aggregate"] + s["message"] + s["signature"]) for s in sets),
            "status": bytes(s["status"] for s in sets), "verdicts": [bool(s["verdict"]) for s in sets], "routes": [s["route"] for s in sets]}


def as_records(aggs):
    """the packed aggregates as the keys of 320-byte records with something else behind each key"""
    return b"".join(aggs[96 * c:96 * c + 96] + bytes([0xa5]) * 224 for c in range(len(aggs) // 96))


def participants(fx, s):
    """the table indices of the set's participants, in committee order"""
    a, b = fx["c_offsets"][s["committee"]], fx["c_offsets"][s["committee"] + 1]
    bits = bytes.fromhex(s["bits"])
    return [fx["idx"][a + i] for i in range(b - a) if bits[i // 8] >> (i % 8) & 1]


@pytest.fixture(scope="module")
def emu_bits():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggbits.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libaggbits.so"))
    cp, sz, pu32 = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)
    L.emu_aggregate_sets_bits.argtypes = [cp, sz, pu32, ctypes.POINTER(sz), sz, cp, sz, pu32, cp, sz, cp, cp, cp, cp, pu32]

    def run(table, idx, c_offsets, aggs, stride, which, bits, msgs, sigs):
        m, k = len(c_offsets) - 1, len(which)
        rec, st, routes = ctypes.create_string_buffer(320 * k), ctypes.create_string_buffer(k), (ctypes.c_uint32 * 2)(7, 7)
        iarr = (ctypes.c_uint32 * len(idx))(*idx) if idx is not None else None
        rc = L.emu_aggregate_sets_bits(table, len(table) // 96, iarr, (sz * (m + 1))(*c_offsets), m, aggs, stride, (ctypes.c_uint32 * max(k, 1))(*which),
                                       b"".join(bits) + b"\0", k, msgs, sigs, rec, st, routes)
        return rc, rec.raw, st.raw, tuple(routes)
    return run


def test_fixture_has_every_kind():
    fx = golden("aggregate_bits")
    by = {s["kind"]: s for s in fx["sets"]}
    lens = [b - a for a, b in zip(fx["c_offsets"], fx["c_offsets"][1:])]
    assert {1, 7, 8, 9, 64, 65} <= set(lens)
    for s in fx["sets"]:
        L, bits = lens[s["committee"]], bytes.fromhex(s["bits"])
        assert len(bits) == (L + 7) // 8
        pop = sum(bits[i // 8] >> (i % 8) & 1 for i in range(L))
        assert pop == s["popcount"]
        base_zero = fx["committees"][s["committee"]]["aggregate"] == bytes(96).hex()
        assert s["route"] == int(not base_zero and 2 * pop > L), s["kind"]
        assert (s["aggregate"] == bytes(96).hex()) == (s["status"] != 0)
        assert s["verdict"] == int(s["status"] == 0 and not s["kind"].startswith("wrong"))
        assert (s["status"] == 1) == (pop == 0)
    assert by["none_set"]["popcount"] == 0 and by["all_set"]["popcount"] == 9 and by["all_set"]["route"] == 1
    assert (by["half"]["popcount"], by["half"]["route"], by["half_plus_1"]["popcount"], by["half_plus_1"]["route"]) == (4, 0, 5, 1)
    assert by["only_last"]["bits"] == "00" * 7 + "80" and by["only_first"]["bits"] == "01" + "00" * 7
    assert by["only_last"]["committee"] == by["only_first"]["committee"]                      # two sets on one committee
    for kind in ("all_set_unused_bits_set", "none_set_unused_bits_set", "len_65_most", "len_7_all_and_delimiter", "len_1_delimiter_only"):
        s = by[kind]
        L, last = lens[s["committee"]], bytes.fromhex(s["bits"])[-1]
        assert L % 8 and last >> (L % 8) == 0xff >> (L % 8), kind                              # every unused bit of the last byte
    assert by["all_set_unused_bits_set"]["aggregate"] == by["all_set"]["aggregate"]
    assert (by["p_negp_direct"]["status"], by["p_negp_direct"]["route"]) == (2, 0)
    assert (by["p_negp_tie_direct"]["status"], by["p_negp_tie_direct"]["route"]) == (2, 0)
    assert (by["p_negp_r_110"]["status"], by["p_negp_r_110"]["route"], by["p_negp_r_110"]["bits"]) == (2, 1, "03")
    assert (by["p_p_negp_110"]["status"], by["p_p_negp_110"]["route"], by["p_p_negp_110"]["bits"]) == (0, 1, "03")
    assert (by["infinity_base_forces_direct"]["status"], by["infinity_base_forces_direct"]["route"], by["infinity_base_forces_direct"]["popcount"]) == (0, 0, 3)
    assert (by["oor_participating"]["status"], by["oor_absent"]["status"], by["oor_absent"]["route"]) == (3, 0, 0)
    assert fx["oor_value"] >= len(fx["table"]) // 192 and fx["oor_value"] in participants(fx, by["oor_participating"])
    assert fx["oor_value"] not in participants(fx, by["oor_absent"])
    rep = participants(fx, by["repeated_index_most"])
    assert len(set(rep)) < len(rep) and by["repeated_index_most"]["route"] == 1 and by["repeated_index_few"]["route"] == 0
    assert sum(s["route"] for s in fx["sets"]) >= 8 and sum(1 - s["route"] for s in fx["sets"]) >= 8


def test_bodies_equal_fixture_three_ways(emu_bits):
    f = fixture_inputs()
    k, excl = len(f["which"]), sum(f["routes"])
    args = (f["which"], f["bits"], f["msgs"], f["sigs"])
    got96 = emu_bits(f["table"], f["idx"], f["c_offsets"], f["aggs"], 96, *args)
    got320 = emu_bits(f["table"], f["idx"], f["c_offsets"], as_records(f["aggs"]), 320, *args)
    none = emu_bits(f["table"], f["idx"], f["c_offsets"], None, 0, *args)
    for got, routes in ((got96, (k - excl, excl)), (got320, (k - excl, excl)), (none, (k, 0))):
        rc, rec, st, r = got
        assert st == f["status"] and rc == 0 and r == routes
        for s in range(k):
            assert rec[320 * s:320 * s + 320] == f["want"][320 * s:320 * s + 320], s
    assert 0 < excl < k


def test_every_set_alone_and_in_reverse(emu_bits):
    fx = golden("aggregate_bits")
    n = len(fx["sets"])
    for order in [[s] for s in range(n)] + [list(range(n))[::-1]]:
        f = fixture_inputs(fx, order)
        rc, rec, st, r = emu_bits(f["table"], f["idx"], f["c_offsets"], f["aggs"], 96, f["which"], f["bits"], f["msgs"], f["sigs"])
        assert (rec, st, r[1]) == (f["want"], f["status"], sum(f["routes"])), order
        assert rc == int(all(x == 0 for x in f["status"]))


def test_bodies_equal_c_oracle(emu_bits):
    fx = golden("aggregate_bits")
    f = fixture_inputs(fx)
    for aggs, stride in ((f["aggs"], 96), (None, 0)):
        _, rec, st, _ = emu_bits(f["table"], f["idx"], f["c_offsets"], aggs, stride, f["which"], f["bits"], f["msgs"], f["sigs"])
        for s, d in enumerate(fx["sets"]):
            if st[s] == 0:
                keys = b"".join(f["table"][96 * t:96 * t + 96] for t in participants(fx, d))
                assert rec[320 * s:320 * s + 96] == co.g1_sum(keys), d["kind"]


def test_contiguous_committees_without_indices(emu_bits):
    """the committees as stretches of the table itself: committee c = keys [3 c, 3 c + 5) is not expressible, so consecutive stretches"""
    fx = golden("aggregate_bits")
    table = bytes.fromhex(fx["table"])[:96 * 40]
    c_offsets = [0, 9, 9, 26, 40]
    which, bits = [0, 2, 3, 1, 2], [b"\xff\x01", b"\xfe\xff\xff", b"\x03\x00", b"", b"\x01\x00\x01"]
    msgs, sigs = bytes(32 * 5), bytes(192 * 5)
    aggs = b"".join(co.g1_sum(table[96 * a:96 * b]) if b > a else bytes(96) for a, b in zip(c_offsets, c_offsets[1:]))
    for ag, stride, routes in ((aggs, 96, (3, 2)), (None, 0, (5, 0))):
        rc, rec, st, r = emu_bits(table, None, c_offsets, ag, stride, which, bits, msgs, sigs)
        assert st == bytes([0, 0, 0, 1, 0]) and rc == 0 and r == routes
        for s, (c, b) in enumerate(zip(which, bits)):
            keys = b"".join(table[96 * (c_offsets[c] + i):96 * (c_offsets[c] + i) + 96] for i in range(c_offsets[c + 1] - c_offsets[c]) if b[i // 8] >> (i % 8) & 1)
            assert rec[320 * s:320 * s + 96] == (co.g1_sum(keys) if keys else bytes(96)), s


def test_refused_arguments(emu_bits):
    f = fixture_inputs()
    one = ([0], [f["bits"][0][:1]], f["msgs"][:32], f["sigs"][:192])
    assert emu_bits(f["table"], f["idx"], [0, 2, 1], None, 0, *one)[0] == -3                    # decreasing offsets
    assert emu_bits(f["table"], f["idx"], [0, 1], None, 0, [1], *one[1:])[0] == -3              # which >= m
    assert emu_bits(f["table"][:96], None, [0, 2], None, 0, *one)[0] == -3                      # c_offsets[m] past the table without indices
    assert emu_bits(f["table"], f["idx"], [0, 1], f["aggs"], 95, *one)[0] == -3
    assert emu_bits(f["table"], f["idx"], [0, 1], f["aggs"], 98, *one)[0] == -3
