"""CPU-only checks of the p1s_ntt_many entry points: exported and declared, prototypes bound as the header has them, the flags, loud failure
without a context (before the k == 0 rule), argument validation of the Python mirror, and the contract's words in the header."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_p1s_ntt_many", "mi355_bls_p1s_ntt_many_device", "mi355_bls_debug_p1ntt_set_pass")


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
    assert re.search(r"#define MI355_BLS_P1S_NTT_INVERSE 1u\b", hdr) and m.P1S_NTT_INVERSE == 1
    assert re.search(r"#define MI355_BLS_P1S_NTT_BITREV 2u\b", hdr) and m.P1S_NTT_BITREV == 2
    block = hdr[hdr.index("Number-theoretic transforms of k vectors of G1 POINTS"):hdr.index("#define MI355_BLS_P1S_NTT_INVERSE")]
    for words in ("VARIABLE TIME", "7^((r - 1) / n)", "IN PLACE", "NOT checked", "profiles/p1s_ntt_bench.json", "bit-reversed order", "all zero: infinity",
                  "one vector always forms a slice", "waits for it once at the end", "canonicalising copy"):
        assert words in block, words
    for f in ("p1sNttMany", "p1sNttMany_device", "debug_p1ntt_set_pass"):
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
    out = ctypes.create_string_buffer(96)
    for k in (1, 0):                                                # the NULL context comes before k == 0
        assert L.mi355_bls_p1s_ntt_many(None, bytes(96), 1, k, 0, out) < 0
        assert L.mi355_bls_p1s_ntt_many_device(None, None, 1, k, 0, None, None) < 0
    assert L.mi355_bls_debug_p1ntt_set_pass(None, 2) < 0
    assert out.raw == bytes(96)


class _NoCache:
    _h = None


def test_python_mirror_validates_and_handles_empty_input(m):
    c = _NoCache()
    p = bytes(96)
    for case in (dict(points=bytes(95)), dict(points=p * 3), dict(n=0), dict(n=-2), dict(n=3, points=p * 3), dict(n=1 << 33), dict(flags=4), dict(flags=7)):
        a = dict(points=p * 2, n=2, flags=0)
        a.update(case)
        with pytest.raises(ValueError):
            m.p1sNttMany(c, a["points"], a["n"], a["flags"])
    assert m.p1sNttMany(c, b"", 4) == b""                           # k == 0: nothing is called, nothing touched
    assert m.p1sNttMany(c, b"", 4, m.P1S_NTT_INVERSE | m.P1S_NTT_BITREV) == b""
    for case in (dict(n=0), dict(n=12), dict(n=(1 << 32) + 1), dict(flags=4), dict(k=-1), dict(d_in=0), dict(d_in=None)):
        a = dict(d_in=64, n=4, k=1, flags=0)
        a.update(case)
        with pytest.raises(ValueError):
            m.p1sNttMany_device(c, a["d_in"], a["n"], a["k"], a["flags"], 64)
    assert m.p1sNttMany_device(c, 0, 4, 0) is None
