"""CPU-only checks of the short-linear-combination entry points: exported and declared, prototypes bound as the header has them, loud failure
without a context, argument validation of the Python mirror, the k == 0 return."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_p1s_lincomb_many", "mi355_bls_p1s_lincomb_many_device", "mi355_bls_p2s_lincomb_many", "mi355_bls_p2s_lincomb_many_device",
         "mi355_bls_debug_lincomb_set_chunk")


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
    assert re.search(r"#define MI355_BLS_LINCOMB_SUBGROUP 1u\b", hdr) and m.LINCOMB_SUBGROUP == 1
    assert "VARIABLE TIME" in hdr[hdr.index("Short linear combinations"):hdr.index("#define MI355_BLS_LINCOMB_SUBGROUP")]
    for f in ("p1sLincombMany", "p2sLincombMany", "p1sLincombMany_device", "p2sLincombMany_device", "debug_lincomb_set_chunk"):
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
                assert "*" in a, (n, a)


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    out, offs = ctypes.create_string_buffer(192), (ctypes.c_size_t * 2)(0, 1)
    for n, row in (("mi355_bls_p1s_lincomb_many", 96), ("mi355_bls_p2s_lincomb_many", 192)):
        assert getattr(L, n)(None, bytes(row), 1, None, offs, 1, bytes(32), 255, 0, out, out) < 0
        assert getattr(L, n)(None, bytes(row), 1, None, offs, 0, bytes(32), 255, 0, out, out) < 0             # the NULL context comes before k == 0
        assert getattr(L, n + "_device")(None, None, 1, None, offs, 1, None, 255, 0, None, out, None) < 0
    assert L.mi355_bls_debug_lincomb_set_chunk(None, 16) < 0


class _NoCache:
    _h = None


def test_python_mirror_validates_and_handles_empty_input(m):
    c = _NoCache()
    p1, p2, s = bytes(96), bytes(192), bytes(32)
    for f, pt, other in ((m.p1sLincombMany, p1, p2), (m.p2sLincombMany, p2, bytes(191))):
        with pytest.raises(ValueError):
            f(c, [pt], [[bytes(31)]])                              # a scalar that is not 32 bytes
        with pytest.raises(ValueError):
            f(c, [pt], bytes(33))
        with pytest.raises(ValueError):
            f(c, [pt + pt], [[s]])                                 # one scalar for two terms
        with pytest.raises(ValueError):
            f(c, (pt, [0, 0], [0, 2]), bytes(96))
        with pytest.raises(ValueError):
            f(c, [other[:-1]], [[s]])                              # a point of the wrong size
        with pytest.raises(ValueError):
            f(c, [], [[s]])                                        # scalars without terms
        for nbits in (0, 257, -1):
            with pytest.raises(ValueError):
                f(c, [pt], [[s]], nbits)
        with pytest.raises(ValueError):
            f(c, [pt], [[s]], 255, 2)                              # an unknown flag bit
        with pytest.raises(OverflowError):
            f(c, [pt], [[1 << 256]])                               # an integer scalar that does not fit 32 bytes
        assert f(c, [], []) == (False, b"", b"")
        assert f(c, [], b"") == (False, b"", b"")
    with pytest.raises(ValueError):
        m.p1sLincombMany(c, [p1], [[s]], 255, m.LINCOMB_SUBGROUP)  # the subgroup flag is the G2 call's
    with pytest.raises(ValueError):
        m.p1sLincombMany_device(c, 0, 0, None, [0, 1], 0, 0, 255, m.LINCOMB_SUBGROUP)
    with pytest.raises(ValueError):
        m.p2sLincombMany_device(c, 0, 0, None, [0, 1], 0, 0, 0)
    assert m.p1sLincombMany_device(c, 0, 0, None, [0], 0, 0) == (False, b"")
    assert m.p2sLincombMany_device(c, 0, 0, None, [0], 0, 0, 255, m.LINCOMB_SUBGROUP) == (False, b"")
