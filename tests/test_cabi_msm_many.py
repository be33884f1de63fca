"""CPU-only checks of the many-MSM entry points: exported, declared and bound with the header's argument lists; the argument rules that are
decided before the context is looked into; the Python mirror's handling of k == 0 and of lengths that do not divide."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_p1s_mult_pippenger_many", "mi355_bls_p1s_mult_pippenger_many_device")
ERR_ARG = -3


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_both_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in ("p1s_mult_pippenger_many", "p1s_mult_pippenger_many_device"):
        assert callable(getattr(m, n)), n


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    want = {NAMES[0]: 8, NAMES[1]: 10}
    for n in NAMES:
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args) == want[n], n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("const size_t*"):
                assert t is ctypes.POINTER(ctypes.c_size_t), (n, a)
            else:
                assert "*" in a and t is ctypes.c_void_p, (n, a)


def offs(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_argument_rules_that_need_no_device(m):
    """A null context is refused before every other rule.  Every other rule here is decided before the context is looked into, so a block of
    zero bytes stands in for one: no call below may get as far as using it."""
    L = m.lib()
    many, dev = L.mi355_bls_p1s_mult_pippenger_many, L.mi355_bls_p1s_mult_pippenger_many_device
    ctx = ctypes.create_string_buffer(1 << 16)
    out = ctypes.create_string_buffer(144 * 4)
    pts, sc = ctypes.create_string_buffer(96 * 4), ctypes.create_string_buffer(32 * 8)
    good = offs(0, 2, 4)
    # null context: before the k == 0 rule, the size rules and everything else
    assert many(None, out, pts, 4, sc, good, 2, 255) == ERR_ARG
    assert many(None, out, pts, 4, sc, good, 0, 255) == ERR_ARG
    assert many(None, None, None, 0, None, None, 0, 0) == ERR_ARG
    assert dev(None, out, None, pts, 4, sc, good, 2, 255, None) == ERR_ARG
    assert dev(None, None, None, None, 0, None, None, 0, 255, None) == ERR_ARG
    # k == 0 returns 0 and touches nothing (not the outputs either, and no other rule is looked at)
    out.raw = b"\xaa" * len(out.raw)
    assert many(ctx, out, pts, 4, sc, offs(0), 0, 255) == 0
    assert many(ctx, None, None, 4, None, None, 0, 0) == 0
    assert dev(ctx, out, None, pts, 4, sc, None, 0, 255, None) == 0
    assert dev(ctx, None, None, None, 0, None, None, 0, 999, None) == 0
    assert out.raw == b"\xaa" * len(out.raw)
    # null arrays with work to do
    assert many(ctx, out, None, 4, sc, good, 2, 255) == ERR_ARG
    assert many(ctx, out, pts, 4, None, good, 2, 255) == ERR_ARG
    assert many(ctx, out, None, 4, sc, None, 2, 255) == ERR_ARG
    assert dev(ctx, out, None, None, 4, sc, good, 2, 255, None) == ERR_ARG
    assert dev(ctx, out, None, pts, 4, None, None, 2, 255, None) == ERR_ARG
    # bad offsets: decreasing, offsets[0] != 0, offsets[k] != npoints
    for bad in (offs(0, 3, 2, 4), offs(1, 2, 3, 4), offs(0, 1, 2, 3), offs(0, 1, 2, 5)):
        assert many(ctx, out, pts, 4, sc, bad, 3, 255) == ERR_ARG
        assert dev(ctx, out, None, pts, 4, sc, bad, 3, 255, None) == ERR_ARG
    # nbits out of range
    for nbits in (0, 257):
        assert many(ctx, out, pts, 4, sc, good, 2, nbits) == ERR_ARG
        assert many(ctx, out, pts, 4, sc, None, 2, nbits) == ERR_ARG
        assert dev(ctx, out, None, pts, 4, sc, good, 2, nbits, None) == ERR_ARG
    # one MSM of more than 2^28 points (the single call's limit), wherever it stands: refused before anything is launched
    big = (1 << 28) + 1
    assert many(ctx, out, pts, big + 2, sc, offs(0, 1, big + 1, big + 2), 3, 255) == ERR_ARG
    assert dev(ctx, out, None, pts, big + 2, sc, offs(0, 1, big + 1, big + 2), 3, 255, None) == ERR_ARG
    assert dev(ctx, out, None, pts, big, sc, None, 2, 255, None) == ERR_ARG
    # no output at all
    assert many(ctx, None, pts, 4, sc, good, 2, 255) == ERR_ARG
    assert dev(ctx, None, None, pts, 4, sc, good, 2, 255, None) == ERR_ARG
    assert ctx.raw == bytes(1 << 16)


class _NoCache:
    _h = None


def test_python_mirror_handles_no_msms_and_lengths_that_do_not_divide(m):
    c = _NoCache()
    assert m.p1s_mult_pippenger_many(c, b"", b"", offsets=[0]) == []                  # ragged, k == 0
    assert m.p1s_mult_pippenger_many(c, b"", b"") == []                               # shared, no points and no scalars
    assert m.p1s_mult_pippenger_many(c, bytes(96 * 3), b"") == []                     # shared, k = 0 / 3
    assert m.p1s_mult_pippenger_many_device(c, 0, 0, 0, None, 0) == []
    with pytest.raises(ValueError):
        m.p1s_mult_pippenger_many(c, bytes(96 * 3), bytes(32 * 7))                    # 7 scalars over 3 shared points
    with pytest.raises(ValueError):
        m.p1s_mult_pippenger_many(c, b"", bytes(32))                                  # scalars without points
    with pytest.raises(ValueError):
        m.p1s_mult_pippenger_many(c, bytes(96 * 3), bytes(32 * 3), offsets=[0, 2])    # offsets[k] != n
    with pytest.raises(ValueError):
        m.p1s_mult_pippenger_many(c, bytes(96 * 3), bytes(32 * 3), offsets=[0, 2, 1, 3])
    with pytest.raises(ValueError):
        m.p1s_mult_pippenger_many(c, bytes(96 * 3), bytes(32 * 2), offsets=[0, 3])    # ragged: a scalar per point
    with pytest.raises(ValueError):
        m.p1s_mult_pippenger_many_device(c, 0, 4, 0, [0, 4], 2)                       # k + 1 offsets
