"""The item bodies of the per-set key aggregation (csrc/aggsets.hpp: level-0 sums of affine keys, sums of partials, the conversion to the affine
record and the status byte) executed on the CPU under the bounds tracker (tests/host_emu/aggsets.cpp), over the tables of the product's own plan,
for every segment of tests/golden/aggregate_sets.json: records and status bytes byte-equal to the fixture, in the contiguous and in the
indexed form, and against the C restatement's key sum."""
import ctypes
import os
import subprocess

import pytest

import c_oracle as co
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture_inputs(fx=None):
    """-> (keys, offsets, messages, signatures, expected records, expected status bytes) of the fixture's segments, laid end to end"""
    fx = fx or golden("aggregate_sets")
    segs = fx["segments"]
    keys = b"".join(bytes.fromhex(s["keys"]) for s in segs)
    offsets = [0]
    for s in segs:
        offsets.append(offsets[-1] + len(s["keys"]) // 192)
    msgs = b"".join(bytes.fromhex(s["message"]) for s in segs)
    sigs = b"".join(bytes.fromhex(s["signature"]) for s in segs)
    want = b"".join(bytes.fromhex(s["aggregate"] + s["message"] + s["signature"]) for s in segs)
    return keys, offsets, msgs, sigs, want, bytes(s["status"] for s in segs)


def indexed_inputs(bad=False, fx=None):
    """-> (table, idx, offsets, expected records, expected status) of the indexed form; bad: with the out-of-range index in place"""
    fx = fx or golden("aggregate_sets")
    ix = fx["indexed"]
    _, _, _, _, want, status = fixture_inputs(fx)
    idx = list(ix["idx"])
    if bad:
        b = ix["bad_index"]
        idx[b["position"]] = b["value"]
        s = b["segment"]
        want = want[:320 * s] + bytes(96) + want[320 * s + 96:]
        status = status[:s] + bytes([b["status"]]) + status[s + 1:]
    return bytes.fromhex(ix["table"]), idx, list(ix["offsets"]), want, status


@pytest.fixture(scope="module")
def emu_agg():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggsets.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libaggsets.so"))
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    L.emu_aggregate_sets.argtypes = [cp, sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(sz), sz, cp, cp, cp, cp]

    def run(keys, idx, offsets, msgs, sigs):
        k = len(offsets) - 1
        rec, st = ctypes.create_string_buffer(320 * k), ctypes.create_string_buffer(k)
        iarr = (ctypes.c_uint32 * len(idx))(*idx) if idx is not None else None
        rc = L.emu_aggregate_sets(keys, len(keys) // 96, iarr, (sz * (k + 1))(*offsets), k, msgs, sigs, rec, st)
        return rc, rec.raw, st.raw
    return run


def test_fixture_has_every_kind():
    fx = golden("aggregate_sets")
    C = fx["C"]
    kinds = [s["kind"] for s in fx["segments"]]
    for n in (1, 2, C - 1, C, C + 1, C * C + 1, 64, 65):
        assert "len_%d" % n in kinds
    for k in ("empty", "p_p", "p_negp", "c_p_c_p", "p_q_negp_negq_r", "wrong_signature", "wrong_message"):
        assert k in kinds
    by = {s["kind"]: s for s in fx["segments"]}
    assert by["empty"]["status"] == 1 and by["p_negp"]["status"] == 2 and all(s["status"] == 0 for s in fx["segments"] if s["kind"] not in ("empty", "p_negp"))
    assert all(s["verdict"] == int(s["status"] == 0 and not s["kind"].startswith("wrong")) for s in fx["segments"])
    assert all((s["aggregate"] == bytes(96).hex()) == (s["status"] != 0) for s in fx["segments"])
    assert len(by["c_p_c_p"]["keys"]) == 2 * C * 192 and len(set(by["c_p_c_p"]["keys"][192 * j:192 * j + 192] for j in range(2 * C))) == 1
    ix = fx["indexed"]
    assert len(set(ix["idx"])) < len(ix["idx"]) and ix["bad_index"]["value"] >= len(ix["table"]) // 192
    assert ix["idx"] != sorted(ix["idx"])                        # a shuffled table


def test_bodies_equal_fixture(emu_agg):
    keys, offsets, msgs, sigs, want, status = fixture_inputs()
    rc, rec, st = emu_agg(keys, None, offsets, msgs, sigs)
    assert st == status and rc == 0
    for s in range(len(st)):
        assert rec[320 * s:320 * s + 320] == want[320 * s:320 * s + 320], s


def test_indexed_form_and_bad_index(emu_agg):
    _, _, msgs, sigs, _, _ = fixture_inputs()
    for bad in (False, True):
        table, idx, offsets, want, status = indexed_inputs(bad)
        rc, rec, st = emu_agg(table, idx, offsets, msgs, sigs)
        assert (rc, st, rec) == (0, status, want), bad
    assert 3 in indexed_inputs(True)[4]


def test_only_good_segments_return_one(emu_agg):
    keys, offsets, msgs, sigs, want, status = fixture_inputs()
    n = status.index(1)                                          # the segments in front of the empty one
    rc, rec, st = emu_agg(keys, None, offsets[:n + 1], msgs[:32 * n], sigs[:192 * n])
    assert rc == 1 and st == bytes(n) and rec == want[:320 * n]


def test_bodies_equal_c_oracle(emu_agg):
    keys, offsets, msgs, sigs, _, _ = fixture_inputs()
    _, rec, st = emu_agg(keys, None, offsets, msgs, sigs)
    for s in range(len(st)):
        seg = keys[96 * offsets[s]:96 * offsets[s + 1]]
        if seg:
            assert rec[320 * s:320 * s + 96] == co.g1_sum(seg), s


def test_refused_offsets(emu_agg):
    keys, offsets, msgs, sigs, _, _ = fixture_inputs()
    assert emu_agg(keys, None, [0, 2, 1], msgs[:64], sigs[:384])[0] == -3
    assert emu_agg(keys[:96], None, [0, 2], msgs[:32], sigs[:192])[0] == -3      # offsets[k] past the table without indices
