"""fromBytes on the encodings an attacker would pick (tests/golden/deser_adversarial.json: small-order and torsion points, G2 points whose y has
a zero component, coordinates at and around p, flag-bit edges, bad key with bad signature), through the CPU build of the device code
(tests/host_emu, bounds tracked) against the big-integer oracle computed here and the statuses the fixture records.  The GPU half is
tests/test_gpu_deser_adversarial.py."""
import ctypes
import os
import subprocess

import pytest

import bls12381_py as o
import deser_cases as dc
from util import buf

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dc.fixture()


@pytest.fixture(scope="module")
def live(fx):
    """{(row, keys uncompressed, signatures uncompressed): [status with KNOWN_ON_CURVE off, on]} by the oracle, computed once"""
    return {(i, pku, sgu): [dc.oracle_status(pkb, pku, sgb, sgu, known) for known in (False, True)]
            for pku, sgu in dc.COMBOS for i, pkb, sgb in dc.rows_for(fx, pku, sgu)}


def test_fixture_has_every_family(fx):
    rows, enc = fx["rows"], fx["enc"]
    assert len(rows) < 200 and {r["family"] for r in rows} == {"valid", "g1_torsion", "g2_torsion", "fp2_sign", "range", "precedence"}
    for l in (3, 11, 10177, 859267, 52437899, 33):
        assert "g1_ord%d_0_pos" % l in enc and "g1_ord%d_0_neg" % l in enc
    for l in (11, 10177, 859267, 52437899):
        assert "g1_ord%d_1_pos" % l in enc                                   # the second, independent point of the rank-2 torsion
    for l in (13, 23, 2713, 11953, 262069, 299, "c448"):
        assert "g2_ord%s_0_pos" % l in enc
    assert "g2_ord13_1_pos" in enc and "g2_ord23_1_pos" in enc
    assert enc["g1_ord3_0_pos"]["c"] == "80" + "00" * 47 and enc["g1_ord3_0_neg"]["c"] == "a0" + "00" * 47
    assert sum(1 for k in enc if k.startswith("g2_y_c1zero")) == 6 and sum(1 for k in enc if k.startswith("g2_y_c0zero")) == 6
    prec = [r for r in rows if r["family"] == "precedence"]
    assert sorted(r["st"][0] for r in prec) == [1, 1, 2, 2, 3, 3]
    assert {r["st"][0] for r in rows} == {0, 1, 2, 3, 4, 5}


def test_fixture_statuses_equal_the_oracle(fx, live):
    """the recorded statuses, under every wire form a row applies to, against decode-by-square-root and [r]P == infinity computed now"""
    seen = set()
    for (i, pku, sgu), st in live.items():
        assert st == fx["rows"][i]["st"], (fx["rows"][i], pku, sgu, st)
        seen.add(i)
    assert seen == set(range(len(fx["rows"])))
    for i, r in enumerate(fx["rows"]):                                        # the points behind the invariant of the GPU test
        nonmember = False
        for side, name in (("pk", r["pk"]), ("sig", r["sig"])):
            for unc in (False, True):
                b = dc.wire(fx["enc"][name], side, unc)
                if b is not None:
                    ok, pt = dc.decode(side, b, unc)
                    nonmember |= ok and pt is not None and not dc.in_subgroup(side, pt)
        assert nonmember == r["nonmember"], r
        if nonmember and r["family"] != "precedence":
            assert r["st"][0] in (2, 5)


def test_tuples_through_the_device_code(emu, fx, live):
    """deserialize_tuple as k_deser calls it, for every row, wire-form combination and both settings of KNOWN_ON_CURVE"""
    for (i, pku, sgu), want in live.items():
        r = fx["rows"][i]
        pkb, sgb = dc.wire(fx["enc"][r["pk"]], "pk", pku), dc.wire(fx["enc"][r["sig"]], "sig", sgu)
        flags = (dc.PK_UNCOMPRESSED if pku else 0) | (dc.SIG_UNCOMPRESSED if sgu else 0)
        got = [emu.emu_deserialize_tuple_ex(pkb, sgb, flags), emu.emu_deserialize_tuple_ex(pkb, sgb, flags | dc.KNOWN_ON_CURVE)]
        assert got == want == r["st"], (r, pku, sgu, got)
        if r["nonmember"]:
            assert got[0] != 0, r                                             # no point outside the subgroup gets through fromBytes


def test_decode_and_membership_of_every_encoding(emu, fx):
    """each encoding on its own: uncompress / deserialize give the oracle's verdict, infinity flag and point image, and the endomorphism
    membership tests agree with [r]P == infinity on every point that decodes"""
    inf = ctypes.c_int()
    members = {"pk": set(), "sig": set()}
    for name, e in fx["enc"].items():
        side = "pk" if name.startswith(("g1_", "good_pk")) else "sig"
        n = 96 if side == "pk" else 192
        for unc in (False, True):
            b = dc.wire(e, side, unc)
            if b is None:
                continue
            fn = {("pk", False): emu.emu_g1_uncompress, ("pk", True): emu.emu_g1_deserialize,
                  ("sig", False): emu.emu_g2_uncompress, ("sig", True): emu.emu_g2_deserialize}[side, unc]
            out = buf(n)
            ok, pt = dc.decode(side, b, unc)
            assert fn(b, out, ctypes.byref(inf)) == int(ok), (name, unc)
            if not ok:
                continue
            assert inf.value == int(pt is None), (name, unc)
            assert out.raw == (o.g1_to_blst_affine(pt) if side == "pk" else o.g2_to_blst_affine(pt)), (name, unc)
            if pt is not None and pt not in members[side]:
                members[side].add(pt)
                got = emu.emu_g1_in_subgroup(out.raw) if side == "pk" else emu.emu_g2_in_subgroup(out.raw)
                assert got == int(dc.in_subgroup(side, pt)), name
    assert len(members["pk"]) > 20 and len(members["sig"]) > 30


def test_compress_on_boundary_images():
    """g1_compress (shared by popVerify's message and mi355_bls_compress_public_keys) takes images without validating them: for y at
    1, (p - 1) / 2, (p + 1) / 2, p - 1 the sign bit is the integer rule y > p - y and the x bytes are canonical.  No curve point has
    y = (p +- 1) / 2 (y^2 - 4 is not a cube for either), so the boundary of fp_is_lex_largest is reached only this way."""
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_pop.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libpop.so"))
    L.emu_g1_compress.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.emu_g1_compress.restype = None
    for x, y in dc.compress_boundary_images():
        out = buf(48)
        L.emu_g1_compress(o.g1_to_blst_affine((x, y)), out)
        assert out.raw == dc.compress_boundary_expect(x, y), (hex(x), hex(y))
