"""CPU-only checks of the fr_open_many entry points: exported and declared, prototypes bound as the header has them, loud failure without a
context (before the k == 0 rule), argument validation of the Python mirror, and the contract's words in the header."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_fr_open_many", "mi355_bls_fr_open_many_device", "mi355_bls_debug_fropen_set_pass")


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
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert re.search(r"#define MI355_BLS_FR_OPEN_EVAL 1u\b", hdr) and m.FR_OPEN_EVAL == 1
    block = hdr[hdr.index("Openings of k polynomials over the scalar field"):hdr.index("#define MI355_BLS_FR_OPEN_EVAL")]
    for words in ("VARIABLE TIME", "NOT CHECKED", "PADDING SLOT", "one workgroup"):
        assert words in block, words
    for f in ("frOpenMany", "frOpenMany_device", "debug_fropen_set_pass"):
        assert callable(getattr(m, f)), f


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n in NAMES:
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args), n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.c_uint32, (n, a)
            else:
                assert "*" in a and t is ctypes.c_void_p, (n, a)


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    out = ctypes.create_string_buffer(64)
    for k in (1, 0):                                                # the NULL context comes before k == 0
        assert L.mi355_bls_fr_open_many(None, bytes(32), 1, bytes(32), k, 0, None, out, out, out) < 0
        assert L.mi355_bls_fr_open_many_device(None, None, 1, None, k, 0, None, None, None, out, None) < 0
    assert L.mi355_bls_debug_fropen_set_pass(None, 2) < 0


class _NoCache:
    _h = None


def test_python_mirror_validates_and_handles_empty_input(m):
    c = _NoCache()
    s = bytes(32)
    bad = [dict(polys=bytes(31)), dict(polys=s * 3), dict(polys=b""), dict(zs=bytes(33)), dict(n=0), dict(n=-1), dict(flags=2), dict(flags=3),
           dict(domain=s * 2),                                      # a domain without the flag
           dict(flags=m.FR_OPEN_EVAL),                              # the flag without a domain
           dict(flags=m.FR_OPEN_EVAL, domain=s),                    # a domain of the wrong length
           dict(flags=m.FR_OPEN_EVAL, domain=s * 3, n=3, polys=s * 3),      # n is no power of two
           dict(want_ys=False, want_quot=False)]
    for case in bad:
        a = dict(polys=s * 2, n=2, zs=s, flags=0, domain=None, want_ys=True, want_quot=True)
        a.update(case)
        with pytest.raises(ValueError):
            m.frOpenMany(c, a["polys"], a["n"], a["zs"], a["flags"], a["domain"], a["want_ys"], a["want_quot"])
    assert m.frOpenMany(c, b"", 4, b"") == (0, b"", b"", b"")
    assert m.frOpenMany(c, b"", 4, b"", m.FR_OPEN_EVAL, s * 4, want_ys=False) == (0, None, b"", b"")
    for case in (dict(n=0), dict(flags=2), dict(d_domain=64), dict(flags=1), dict(flags=1, d_domain=64, n=12), dict(k=-1),
                 dict(d_out_ys=None, want_status=False), dict(d_polys=0), dict(d_zs=None)):
        a = dict(d_polys=64, n=4, d_zs=64, k=1, flags=0, d_domain=None, d_out_ys=64, d_out_quot=None, want_status=True)
        a.update(case)
        with pytest.raises(ValueError):
            m.frOpenMany_device(c, a["d_polys"], a["n"], a["d_zs"], a["k"], a["flags"], a["d_domain"], a["d_out_ys"], a["d_out_quot"], 0, a["want_status"])
    assert m.frOpenMany_device(c, 0, 4, 0, 0) == (0, b"")
