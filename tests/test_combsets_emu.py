"""The bodies of the same-message pre-aggregation (csrc/combsets.hpp: the scalar chain, the windowed 64-bit multiplications with their tables
outside the lane, the sums of Jacobian points, the member checks, the conversion to the record and the status byte) executed on the CPU
under the bounds tracker (tests/host_emu/combsets.cpp), over the tables of the product's own plan, for every segment of
tests/golden/combine_sets.json: records and status bytes byte-equal to the fixture, in the contiguous and in the indexed form, and against
the C restatement's combine."""
import ctypes
import os
import subprocess

import pytest

import c_oracle as co
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))


def table_records(fx=None):
    fx = fx or golden("combine_sets")
    t = bytes.fromhex(fx["table"])
    return [t[320 * i:320 * i + 320] for i in range(len(t) // 320)]


def fixture_inputs(fx=None):
    """-> (member records laid end to end, offsets, rnds, expected records, expected status bytes) of the fixture's segments"""
    fx = fx or golden("combine_sets")
    tab, segs = table_records(fx), fx["segments"]
    sets = b"".join(tab[j] for s in segs for j in s["members"])
    offsets = [0]
    for s in segs:
        offsets.append(offsets[-1] + len(s["members"]))
    return (sets, offsets, b"".join(bytes.fromhex(s["rnd"]) for s in segs), b"".join(bytes.fromhex(s["record"]) for s in segs),
            bytes(s["status"] for s in segs))


def indexed_inputs(bad=False, fx=None):
    """-> (table, idx, offsets, rnds, expected records, expected status) of the indexed form; bad: with the out-of-range index in place"""
    fx = fx or golden("combine_sets")
    _, offsets, rnds, want, status = fixture_inputs(fx)
    idx = [j for s in fx["segments"] for j in s["members"]]
    if bad:
        b = fx["bad_index"]
        s = b["segment"]
        idx[offsets[s] + b["position"]] = b["value"]
        want = want[:320 * s] + bytes.fromhex(b["record"]) + want[320 * s + 320:]
        status = status[:s] + bytes([b["status"]]) + status[s + 1:]
    return bytes.fromhex(fx["table"]), idx, offsets, rnds, want, status


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_combsets.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libcombsets.so"))
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    L.emu_combine_sets.argtypes = [cp, sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(sz), sz, cp, cp, cp]
    L.emu_combsets_chain.argtypes = [cp, sz, ctypes.POINTER(ctypes.c_uint64)]

    def run(sets, idx, offsets, rnds):
        k = len(offsets) - 1
        rec, st = ctypes.create_string_buffer(320 * k), ctypes.create_string_buffer(k)
        iarr = (ctypes.c_uint32 * max(len(idx), 1))(*idx) if idx is not None else None
        rc = L.emu_combine_sets(sets or b"\0", len(sets) // 320, iarr, (sz * (k + 1))(*offsets), k, rnds, rec, st)
        return rc, rec.raw, st.raw

    def chain(rnd, n):
        out = (ctypes.c_uint64 * n)()
        L.emu_combsets_chain(rnd, n, out)
        return list(out)
    run.chain = chain
    return run


def test_fixture_has_every_kind():
    fx = golden("combine_sets")
    C = fx["C"]
    by = {s["kind"]: s for s in fx["segments"]}
    for n in (1, 2, 3, 4, 5, C - 1, C, C + 1, C * C + 1, 64, 65):
        assert len(by["len_%d" % n]["members"]) == n and by["len_%d" % n]["status"] == 0 and by["len_%d" % n]["verdict"] == 1
    want = {"twice": (0, 1), "inf_sig": (0, 0), "equal_terms": (0, 1), "cancel": (2, 0), "wrong_signature": (0, 0), "empty": (1, 0), "mixed": (4, 0),
            "inf_key": (5, 0)}
    for kind, sv in want.items():
        assert (by[kind]["status"], by[kind]["verdict"]) == sv, kind
    tab = table_records(fx)
    assert len(set(by["twice"]["members"])) == 1 and len(by["twice"]["members"]) == 2
    assert any(tab[j][128:] == bytes(192) for j in by["inf_sig"]["members"])
    assert any(tab[j][:96] == bytes(96) for j in by["inf_key"]["members"])
    assert len({tab[j][96:128] for j in by["mixed"]["members"]}) == 2
    assert len(by["wrong_signature"]["members"]) == C + 1 and by["empty"]["members"] == []
    for s in fx["segments"]:
        rec = bytes.fromhex(s["record"])
        assert (rec[:96] == bytes(96)) == (s["status"] != 0), s["kind"]
        if s["status"]:
            assert rec[128:] == bytes(192) and rec[96:128] == (tab[s["members"][0]][96:128] if s["members"] else bytes(32))
    assert bytes.fromhex(by["len_1"]["record"]) == tab[by["len_1"]["members"][0]]                    # the passthrough
    assert bytes.fromhex(by["cancel"]["record"])[128:] == bytes(192)
    b = fx["bad_index"]
    assert b["value"] >= len(tab) and b["status"] == 3 and fx["segments"][b["segment"]]["kind"] == "len_%d" % (C + 1)
    flat = [j for s in fx["segments"] for j in s["members"]]
    assert flat != sorted(flat) and len(set(flat)) < len(flat)


def test_chain_equals_c_oracle(emu):
    fx = golden("combine_sets")
    tab = table_records(fx)
    for s in fx["segments"]:
        n = len(s["members"])
        if n >= 2:
            rnd = bytes.fromhex(s["rnd"])
            ms = [tab[j] for j in s["members"]]
            assert emu.chain(rnd, n) == co.combine(rnd, b"".join(r[:96] for r in ms), b"".join(r[128:] for r in ms))[2], s["kind"]
    rnd = bytes(range(32))
    assert emu.chain(rnd, 1030) == co.combine(rnd, bytes(96 * 1030), bytes(192 * 1030))[2]           # 258 digests


def test_bodies_equal_fixture(emu):
    sets, offsets, rnds, want, status = fixture_inputs()
    rc, rec, st = emu(sets, None, offsets, rnds)
    assert st == status and rc == 0
    for s in range(len(st)):
        assert rec[320 * s:320 * s + 320] == want[320 * s:320 * s + 320], s


def test_indexed_form_and_bad_index(emu):
    for bad in (False, True):
        table, idx, offsets, rnds, want, status = indexed_inputs(bad)
        rc, rec, st = emu(table, idx, offsets, rnds)
        assert (rc, st) == (0, status), bad
        for s in range(len(st)):
            assert rec[320 * s:320 * s + 320] == want[320 * s:320 * s + 320], (bad, s)
    assert 3 in indexed_inputs(True)[5]


def test_only_good_segments_return_one_and_range_may_start_late(emu):
    sets, offsets, rnds, want, status = fixture_inputs()
    n = next(i for i, b in enumerate(status) if b)                   # the segments in front of the first refused one
    assert n >= 10
    rc, rec, st = emu(sets, None, offsets[:n + 1], rnds[:32 * n])
    assert rc == 1 and st == bytes(n) and rec == want[:320 * n]
    rc, rec, st = emu(sets, None, offsets[3:n + 1], rnds[32 * 3:32 * n])                             # offsets[0] > 0
    assert rc == 1 and rec == want[320 * 3:320 * n]


def test_bodies_equal_c_oracle(emu):
    fx = golden("combine_sets")
    tab = table_records(fx)
    sets, offsets, rnds, _, _ = fixture_inputs(fx)
    _, rec, st = emu(sets, None, offsets, rnds)
    for i, s in enumerate(fx["segments"]):
        if st[i] == 0 and len(s["members"]) >= 2:
            ms = [tab[j] for j in s["members"]]
            pk, sg, _ = co.combine(bytes.fromhex(s["rnd"]), b"".join(r[:96] for r in ms), b"".join(r[128:] for r in ms))
            assert rec[320 * i:320 * i + 320] == pk + ms[0][96:128] + sg, s["kind"]


def test_refused_offsets(emu):
    sets, offsets, rnds, _, _ = fixture_inputs()
    assert emu(sets, None, [0, 2, 1], rnds[:64])[0] == -3
    assert emu(sets[:320], None, [0, 2], rnds[:32])[0] == -3         # offsets[k] past the table without indices
