"""CPU-only checks of the fr_ntt_many / fr_domain entry points: exported and declared, prototypes bound as the header has them, the flags,
loud failure without a context (before the k == 0 rule), argument validation of the Python mirror, and the contract's words in the header."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_fr_ntt_many", "mi355_bls_fr_ntt_many_device", "mi355_bls_fr_domain", "mi355_bls_fr_domain_device", "mi355_bls_debug_frntt_set_tile",
         "mi355_bls_debug_frntt_set_pass")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


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
    assert re.search(r"#define MI355_BLS_FR_NTT_INVERSE 1u\b", hdr) and m.FR_NTT_INVERSE == 1
    assert re.search(r"#define MI355_BLS_FR_NTT_BITREV 2u\b", hdr) and m.FR_NTT_BITREV == 2
    block = hdr[hdr.index("Number-theoretic transforms of k vectors over the scalar field"):hdr.index("#define MI355_BLS_FR_NTT_INVERSE")]
    for words in ("VARIABLE TIME", "7^((r - 1) / n)", "IN PLACE", "HOST memory", "0 mod r", "natural order"):
        assert words in block, words
    for f in ("frNttMany", "frNttMany_device", "frDomain", "frDomain_device", "debug_frntt_set_tile", "debug_frntt_set_pass"):
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
        assert L.mi355_bls_fr_ntt_many(None, bytes(32), 1, k, 0, None, out, out) < 0
        assert L.mi355_bls_fr_ntt_many_device(None, None, 1, k, 0, None, None, out, None) < 0
    assert L.mi355_bls_fr_domain(None, 1, 0, out) < 0 and L.mi355_bls_fr_domain_device(None, 1, 0, None, None) < 0
    assert L.mi355_bls_debug_frntt_set_tile(None, 2) < 0 and L.mi355_bls_debug_frntt_set_pass(None, 2) < 0
    assert out.raw == bytes(64)


class _NoCache:
    _h = None


def test_python_mirror_validates_and_handles_empty_input(m):
    c = _NoCache()
    s = bytes(32)
    zero_shifts = (s, R.to_bytes(32, "little"), (2 * R).to_bytes(32, "little"))
    bad = [dict(vectors=bytes(31)), dict(vectors=s * 3), dict(n=0), dict(n=-2), dict(n=3, vectors=s * 3), dict(n=1 << 33), dict(flags=4), dict(flags=7),
           dict(shift=bytes(31))] + [dict(shift=z) for z in zero_shifts]
    for case in bad:
        a = dict(vectors=s * 2, n=2, flags=0, shift=None)
        a.update(case)
        with pytest.raises(ValueError):
            m.frNttMany(c, a["vectors"], a["n"], a["flags"], a["shift"])
    assert m.frNttMany(c, b"", 4) == (0, b"", b"")                  # k == 0: nothing is called, nothing touched
    assert m.frNttMany(c, b"", 4, m.FR_NTT_INVERSE | m.FR_NTT_BITREV, (7).to_bytes(32, "little")) == (0, b"", b"")
    for case in (dict(n=0), dict(n=12), dict(n=(1 << 32) + 1), dict(flags=4), dict(k=-1), dict(d_in=0), dict(d_in=None), dict(shift=s), dict(shift=bytes(33))):
        a = dict(d_in=64, n=4, k=1, flags=0, shift=None)
        a.update(case)
        with pytest.raises(ValueError):
            m.frNttMany_device(c, a["d_in"], a["n"], a["k"], a["flags"], a["shift"], 64)
    assert m.frNttMany_device(c, 0, 4, 0) == (0, b"") and m.frNttMany_device(c, 0, 4, 0, want_status=False) == (0, None)
    for n, flags in ((0, 0), (3, 0), (1 << 33, 0), (4, m.FR_NTT_INVERSE), (4, 4)):
        with pytest.raises(ValueError):
            m.frDomain(c, n, flags)
        with pytest.raises(ValueError):
            m.frDomain_device(c, n, 64, flags)
    with pytest.raises(ValueError):
        m.frDomain_device(c, 4, None)
