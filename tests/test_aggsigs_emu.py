"""The item bodies of the per-group signature aggregation (csrc/aggsigs.hpp: level-0 sums of affine signatures, csrc/combsets.hpp's sums of G2
partials, the conversion to the affine image, its compressed wire form and the status byte) executed on the CPU under the bounds tracker
(tests/host_emu/aggsigs.cpp), over the tables of the product's own plan, for every group of tests/golden/aggregate_signatures.json: images, wire
forms and status bytes byte-equal to the fixture, in the contiguous and in the indexed form, and against the C restatement's g2_sum and
compress_sets.  Beside them g2_compress and the signature-only decoder on the adversarial signature encodings."""
import ctypes
import os
import subprocess

import pytest

import aggsigs_cases as ac
import bls12381_py as o
import c_oracle as co
import deser_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_aggsigs.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libaggsigs.so"))
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    L.emu_aggregate_signature_sets.argtypes = [cp, sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(sz), sz, cp, cp, cp]
    L.emu_compress_signatures.argtypes = [cp, sz, cp]
    L.emu_deserialize_signatures.argtypes = [cp, sz, ctypes.c_uint32, cp, cp]
    return L


@pytest.fixture(scope="module")
def emu(lib):
    def run(sigs, idx, offsets, want192=True, want96=True):
        k = len(offsets) - 1
        o192 = ctypes.create_string_buffer(192 * k) if want192 else None
        o96 = ctypes.create_string_buffer(96 * k) if want96 else None
        st = ctypes.create_string_buffer(k)
        iarr = (ctypes.c_uint32 * len(idx))(*idx) if idx is not None else None
        rc = lib.emu_aggregate_signature_sets(sigs, len(sigs) // 192, iarr, (ctypes.c_size_t * (k + 1))(*offsets), k, o192, o96, st)
        return rc, o192.raw if want192 else None, o96.raw if want96 else None, st.raw
    return run


def test_fixture_has_every_kind():
    fx = ac.fixture()
    C = fx["C"]
    assert C == 8 and len(open(os.path.join(HERE, "golden", "aggregate_signatures.json")).read()) <= len(open(os.path.join(HERE, "golden", "aggregate_sets.json")).read())
    by = {}
    for g in fx["groups"]:
        by.setdefault(g["kind"], []).append(g)
    for n in (1, 2, C - 1, C, C + 1, C * C + 1, 64, 65):
        assert any(len(g["members"]) == n for g in by["len_%d" % n])
    tab = ac.table_of(fx)
    assert tab[0] == bytes(192) and len(set(tab)) == len(tab)
    assert by["empty"][0]["members"] == [] and by["empty"][0]["status"] == 1
    a, b = by["s_s"][0]["members"]
    assert a == b and by["s_s"][0]["status"] == 0
    a, b = (o.g2_from_blst_affine(tab[i]) for i in by["s_negs"][0]["members"])
    assert a == o.g2_neg(b) and by["s_negs"][0]["status"] == 2
    assert len(by["c_s_c_s"][0]["members"]) == 2 * C and len(set(by["c_s_c_s"][0]["members"])) == 1
    assert 0 in by["with_zero"][0]["members"] and by["with_zero"][0]["status"] == 0 and len(set(by["with_zero"][0]["members"])) == 3
    assert set(by["only_zero"][0]["members"]) == {0} and by["only_zero"][0]["status"] == 2
    for g in fx["groups"]:
        assert (g["status"] != 0) == (g["out192"] == ac.INF192.hex()) == (g["out96"] == ac.INF96.hex()), g["kind"]
        assert g["status"] == (1 if not g["members"] else 2 if g["out192"] == ac.INF192.hex() else 0)
    ix = fx["indexed"]
    assert len(set(ix["idx"])) < len(ix["idx"]) and ix["idx"] != sorted(ix["idx"]) and ix["bad_index"]["value"] >= len(tab)
    assert ix["offsets"][ix["bad_index"]["group"]] <= ix["bad_index"]["position"] < ix["offsets"][ix["bad_index"]["group"] + 1]


def test_bodies_equal_fixture(emu):
    sigs, offsets, w192, w96, status = ac.contiguous_inputs()
    rc, o192, o96, st = emu(sigs, None, offsets)
    assert st == status and rc == 0
    for g in range(len(st)):
        assert o192[192 * g:192 * g + 192] == w192[192 * g:192 * g + 192], g
        assert o96[96 * g:96 * g + 96] == w96[96 * g:96 * g + 96], g
    assert emu(sigs, None, offsets, want96=False)[1:] == (w192, None, status)
    assert emu(sigs, None, offsets, want192=False)[1:] == (None, w96, status)


def test_indexed_form_and_bad_index(emu):
    for bad in (False, True):
        table, idx, offsets, w192, w96, status = ac.indexed_inputs(bad)
        assert emu(table, idx, offsets) == (0, w192, w96, status), bad
    assert 3 in ac.indexed_inputs(True)[5]


def test_only_good_groups_return_one(emu):
    sigs, offsets, w192, w96, status = ac.contiguous_inputs()
    n = status.index(1)                                          # the groups in front of the empty one
    assert n >= 8 and emu(sigs, None, offsets[:n + 1]) == (1, w192[:192 * n], w96[:96 * n], bytes(n))


def test_bodies_equal_c_oracle(emu):
    sigs, offsets, _, _, _ = ac.contiguous_inputs()
    _, o192, o96, st = emu(sigs, None, offsets)
    for g in range(len(st)):
        seg = sigs[192 * offsets[g]:192 * offsets[g + 1]]
        if seg:
            want = co.g2_sum(seg)
            assert o192[192 * g:192 * g + 192] == want, g
            assert o96[96 * g:96 * g + 96] == co.compress_sets(bytes(128) + want)[2], g


def test_refused_offsets(emu):
    sigs, _, _, _, _ = ac.contiguous_inputs()
    assert emu(sigs, None, [0, 2, 1])[0] == -3
    assert emu(sigs[:192], None, [0, 2])[0] == -3                # offsets[k] past the table without indices
    assert emu(sigs[:192], [0, 0], [0, 2])[0] == 1               # the same offsets are fine through indices


def _decodable(unc):
    """[(name, wire bytes, point)] of the adversarial signature encodings that decode (any subgroup, infinity included)"""
    out = []
    for nm, b in ac.adversarial_signatures(unc):
        ok, pt = dc.decode("sig", b, unc)
        if ok:
            out.append((nm, b, pt))
    return out


def test_compress_on_adversarial_points(lib):
    pts = _decodable(False) + _decodable(True)
    names = {nm for nm, _, _ in pts}
    assert any("c0zero" in nm for nm in names) and any("c1zero" in nm for nm in names) and any("ord13" in nm for nm in names) and "g2_inf" in names
    imgs = b"".join(o.g2_to_blst_affine(pt) for _, _, pt in pts)
    out = ctypes.create_string_buffer(96 * len(pts))
    assert lib.emu_compress_signatures(imgs, len(pts), out) == 0
    for k, (nm, _, pt) in enumerate(pts):
        assert out.raw[96 * k:96 * k + 96] == o.g2_compress(pt), nm
    assert out.raw == b"".join(co.compress_sets(bytes(128) + imgs[192 * k:192 * k + 192])[2] for k in range(len(pts)))


@pytest.mark.parametrize("unc", (False, True))
@pytest.mark.parametrize("known", (False, True))
def test_decoder_on_adversarial_encodings(lib, unc, known):
    encs = ac.adversarial_signatures(unc)
    n, unit = len(encs), (192 if unc else 96)
    assert n >= 40
    flags = (dc.SIG_UNCOMPRESSED if unc else 0) | (dc.KNOWN_ON_CURVE if known else 0)
    sg = b"".join(b for _, b in encs)
    out, st = ctypes.create_string_buffer(192 * n), ctypes.create_string_buffer(n)
    rc = lib.emu_deserialize_signatures(sg, n, flags, out, st)
    pk48 = co.compress_sets(co.make_batch(1, seed=7))[0]
    _, rec, st_c = co.deserialize_sets_ex(pk48 * n, bytes(32 * n), sg, flags)
    assert st.raw == st_c and set(st.raw) <= {0, 4, 5} and rc == int(not any(st.raw))
    if not known:
        assert {0, 4, 5} <= set(st.raw)
    for k, (nm, b) in enumerate(encs):
        assert out.raw[192 * k:192 * k + 192] == rec[320 * k + 128:320 * k + 320], nm
        ok, pt = dc.decode("sig", b, unc)
        want = 4 if not ok else 5 if (not known and pt is not None and not dc.in_subgroup("sig", pt)) else 0
        assert st.raw[k] == want, nm
        assert out.raw[192 * k:192 * k + 192] == (o.g2_to_blst_affine(pt) if want == 0 else bytes(192)), nm
    assert len(sg) == unit * n
