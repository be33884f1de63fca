"""CPU-only checks of the cell-proof entry points: exported and declared, prototypes bound as the header has them, loud failure without a
context (before the k == 0 rule and before every other refusal), argument validation of the Python mirror, and the contract's words in the
header.  The refusals that need a context (cell, ext_log2, flags, NULL arguments, alignment, a cells handle given to open_all_many) are in
tests/test_gpu_fk20_cells.py."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_fk20_setup_create_cells", "mi355_bls_fk20_setup_create_cells_device", "mi355_bls_fk20_open_cells_many", "mi355_bls_fk20_open_cells_many_device")


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
    block = hdr[hdr.index("The proofs of ALL CELLS of each of k polynomials"):hdr.index("int mi355_bls_fk20_setup_create_cells(")]
    block = re.sub(r"\s*\n \*\s*", " ", block)                     # the comment as running text: a phrase may be broken across lines
    for words in ("VARIABLE TIME", "h_(q-1) = infinity", "omega_N^(j s)", "c_(i + l(s+1))", "NOT checked", "profiles/fk20_cells_bench.json", "all zero: infinity",
                  "one polynomial always forms a pass", "a setup of another device", "above 2^31", "every output is infinity", "acts as its value mod r",
                  "x^64 = omega_128^rev7(i)", "the same bytes", "byte for byte", "mi355_bls_fk20_open_all_many refuses it", "no power of two or above n",
                  "n 2^ext_log2 > 2^32", "ext_log2 is still", "mi355_bls_debug_fk20_set_pass shortens these passes too", "p(X) div (X^l - omega_N^j)"):
        assert words in block, words
    for f in ("fk20_setup_create_cells", "fk20_setup_create_cells_device", "fk20OpenCellsMany", "fk20OpenCellsMany_device", "fk20_cells_rows"):
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


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    out, h = ctypes.create_string_buffer(96), ctypes.c_void_p()
    for k in (1, 0):                                                # the NULL context comes before k == 0
        for ext in (0, 1, 40):
            assert L.mi355_bls_fk20_open_cells_many(None, None, bytes(32), k, ext, 0, out, None) < 0
            assert L.mi355_bls_fk20_open_cells_many_device(None, None, None, k, ext, 0, None, None, None) < 0
    for n, cell in ((1, 1), (4, 2), (4, 0), (4, 3), (4, 8), (0, 1), (3, 1), (1 << 32, 1)):
        assert L.mi355_bls_fk20_setup_create_cells(None, ctypes.byref(h), bytes(96 * 4), n, cell) < 0 and not h.value
        assert L.mi355_bls_fk20_setup_create_cells_device(None, ctypes.byref(h), None, n, cell, None) < 0 and not h.value
    assert out.raw == bytes(96)


class _NoCache:
    _h = None


class _NoSetup:
    _h = None
    n = 16
    cell = 4


def test_python_mirror_validates_and_handles_empty_input(m):
    c, s = _NoCache(), _NoSetup()
    assert [m.fk20_cells_rows(s, x, f) for x, f in ((0, 0), (1, 0), (2, m.FK20_BITREV), (2, m.FK20_H), (1, m.FK20_H | m.FK20_BITREV))] == [4, 8, 16, 4, 4]
    for case in (dict(polys=bytes(31)), dict(polys=bytes(32 * 17)), dict(flags=1), dict(flags=8), dict(flags=-1), dict(ext=-1), dict(ext=29)):
        a = dict(polys=bytes(32 * 16), flags=0, ext=1)
        a.update(case)
        with pytest.raises(ValueError):
            m.fk20OpenCellsMany(c, s, a["polys"], a["ext"], a["flags"])
    for flags in (0, m.FK20_BITREV, m.FK20_H, m.FK20_BITREV | m.FK20_H):
        assert m.fk20OpenCellsMany(c, s, b"", 1, flags) == (0, b"", b"")      # k == 0: nothing is called, nothing touched
    for case in (dict(flags=1), dict(flags=16), dict(k=-1), dict(d_polys=0), dict(d_out=None), dict(ext=-1)):
        a = dict(d_polys=64, k=1, d_out=64, flags=0, ext=1)
        a.update(case)
        with pytest.raises(ValueError):
            m.fk20OpenCellsMany_device(c, s, a["d_polys"], a["k"], a["d_out"], a["ext"], a["flags"])
    assert m.fk20OpenCellsMany_device(c, s, 0, 0, 0) == (0, b"")
    with pytest.raises(ValueError):
        m.fk20_setup_create_cells(c, bytes(95), 1)
