"""CPU-only checks of the fk20 entry points: exported and declared, prototypes bound as the header has them, the flags, setup_sizeof, loud
failure without a context (before the k == 0 rule), destroy of NULL, argument validation of the Python mirror, and the contract's words in
the header."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_fk20_setup_sizeof", "mi355_bls_fk20_setup_create", "mi355_bls_fk20_setup_create_device", "mi355_bls_fk20_setup_destroy",
         "mi355_bls_fk20_open_all_many", "mi355_bls_fk20_open_all_many_device", "mi355_bls_debug_fk20_set_pass")


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in exported and hasattr(L, n), n
    assert re.search(r"#define MI355_BLS_FK20_BITREV 2u\b", hdr) and m.FK20_BITREV == 2 == m.P1S_NTT_BITREV
    assert re.search(r"#define MI355_BLS_FK20_H 4u\b", hdr) and m.FK20_H == 4
    assert "typedef struct mi355_bls_fk20_setup mi355_bls_fk20_setup;" in hdr
    block = hdr[hdr.index("ALL n openings of each of k polynomials"):hdr.index("#define MI355_BLS_FK20_BITREV")]
    for words in ("VARIABLE TIME", "h_(n-1) = infinity", "omega_n^(l t)", "NOT checked", "profiles/fk20_bench.json", "bit-reversed order", "all zero: infinity",
                  "one polynomial always forms a pass", "a setup of another device", "above 2^31", "NULL: no-op", "every output is infinity", "acts as its value mod r"):
        assert words in block, words
    for f in ("fk20_setup_sizeof", "fk20_setup_create", "fk20_setup_create_device", "fk20_setup_destroy", "fk20OpenAllMany", "fk20OpenAllMany_device",
              "debug_fk20_set_pass", "Fk20Setup"):
        assert callable(getattr(m, f)), f


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n in NAMES:
        ret, args = re.search(r"\b(int|void|size_t)\s+%s\s*\(([^)]*)\)" % n, hdr).groups()
        args = [a.strip() for a in args.split(",")]
        f = getattr(L, n)
        assert {"int": ctypes.c_int, "void": None, "size_t": ctypes.c_size_t}[ret] is f.restype, n
        assert len(f.argtypes) == len(args), n
        for a, t in zip(args, f.argtypes):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.c_uint32, (n, a)
            else:
                assert "*" in a and t is ctypes.c_void_p, (n, a)


def test_setup_sizeof(m):
    assert [m.fk20_setup_sizeof(n) for n in (1, 2, 64, 4096, 1 << 31)] == [192, 384, 12288, 4096 * 192, 192 << 31]
    for n in (0, 3, 12, (1 << 31) + 1, 1 << 32):                     # what create refuses
        assert m.fk20_setup_sizeof(n) == 0, n


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    out, h = ctypes.create_string_buffer(96), ctypes.c_void_p()
    for k in (1, 0):                                                # the NULL context comes before k == 0
        assert L.mi355_bls_fk20_open_all_many(None, None, bytes(32), k, 0, out, None) < 0
        assert L.mi355_bls_fk20_open_all_many_device(None, None, None, k, 0, None, None, None) < 0
    for n in (1, 0, 3, 1 << 32):
        assert L.mi355_bls_fk20_setup_create(None, ctypes.byref(h), bytes(96), n) < 0 and not h.value
        assert L.mi355_bls_fk20_setup_create_device(None, ctypes.byref(h), None, n, None) < 0 and not h.value
    assert L.mi355_bls_debug_fk20_set_pass(None, 2) < 0
    assert out.raw == bytes(96)
    L.mi355_bls_fk20_setup_destroy(None)                            # NULL: no-op
    m.fk20_setup_destroy(None)


class _NoCache:
    _h = None


class _NoSetup:
    _h = None
    n = 4


def test_python_mirror_validates_and_handles_empty_input(m):
    c, s = _NoCache(), _NoSetup()
    for case in (dict(polys=bytes(31)), dict(polys=bytes(32 * 5)), dict(flags=1), dict(flags=8), dict(flags=-1)):
        a = dict(polys=bytes(32 * 4), flags=0)
        a.update(case)
        with pytest.raises(ValueError):
            m.fk20OpenAllMany(c, s, a["polys"], a["flags"])
    for flags in (0, m.FK20_BITREV, m.FK20_H, m.FK20_BITREV | m.FK20_H):
        assert m.fk20OpenAllMany(c, s, b"", flags) == (0, b"", b"")          # k == 0: nothing is called, nothing touched
    for case in (dict(flags=1), dict(flags=16), dict(k=-1), dict(d_polys=0), dict(d_out=None)):
        a = dict(d_polys=64, k=1, d_out=64, flags=0)
        a.update(case)
        with pytest.raises(ValueError):
            m.fk20OpenAllMany_device(c, s, a["d_polys"], a["k"], a["d_out"], a["flags"])
    assert m.fk20OpenAllMany_device(c, s, 0, 0, 0) == (0, b"")
    with pytest.raises(ValueError):
        m.fk20_setup_create(c, bytes(95))
