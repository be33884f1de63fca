"""CPU-only checks of the per-batch entry points for many batches: exported, declared and bound with the header's argument lists; the argument
rules that are decided before the context's device is touched; the Python mirror's handling of no batches and of lists that do not match."""
import ctypes
import re
import subprocess

import pytest

HOST = ("mi355_bls_batch_verify_many_each", "mi355_bls_batch_verify_many_locate")
DEVICE = tuple(n + "_device" for n in HOST)
GT = "mi355_bls_debug_batch_verify_many_each_gt"
NAMES = HOST + DEVICE + (GT,)
ERR_ARG = -3


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_the_five_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES + ("mi355_bls_debug_batch_verify_many_each_passes",):
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in ("batchVerifyManyEach", "batchVerifyManyEach_device", "batchVerifyManyLocate", "batchVerifyManyLocate_device", "batchVerifyManyEachValues"):
        assert callable(getattr(m, n)), n


def test_prototypes_match_the_header_and_batch_verify_many(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()

    def args_of(n):
        return [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
    want = {n: 6 for n in HOST}
    want.update({n: 7 for n in DEVICE + (GT,)})
    for n in NAMES:
        args = args_of(n)
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args) == want[n], n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("const size_t "):
                assert t is ctypes.POINTER(ctypes.c_size_t), (n, a)
            else:
                assert ("*" in a or "[]" in a) and t in (ctypes.c_void_p, ctypes.c_char_p), (n, a)
    # arguments and layout are exactly those of mi355_bls_batch_verify_many
    strip = lambda a: re.sub(r"\s+", " ", a)
    for n in HOST:
        assert [strip(a) for a in args_of(n)] == [strip(a) for a in args_of("mi355_bls_batch_verify_many")], n
    for n in DEVICE:
        assert [strip(a) for a in args_of(n)] == [strip(a) for a in args_of("mi355_bls_batch_verify_many_device")], n
    assert [strip(a) for a in args_of(GT)][:6] == [strip(a) for a in args_of("mi355_bls_batch_verify_many")]


def cnt(*v):
    return (ctypes.c_size_t * max(len(v), 1))(*v)


def test_argument_rules_that_need_no_device(m):
    """A null context is refused before every other rule.  The other rules here are decided before the context's device is touched, so a block
    of zero bytes stands in for one (no batch pending): no call below may get as far as using it."""
    L = m.lib()
    ctx = ctypes.create_string_buffer(1 << 16)
    sets, rnds = ctypes.create_string_buffer(320 * 4), ctypes.create_string_buffer(32 * 3)
    out, gt = ctypes.create_string_buffer(3), ctypes.create_string_buffer(576 * 3)
    good = cnt(2, 0, 2)
    for n in HOST:
        f, d = getattr(L, n), getattr(L, n + "_device")
        # null context, whatever else is given
        assert f(None, sets, good, rnds, 3, out) == ERR_ARG
        assert f(None, None, None, None, 0, None) == ERR_ARG
        assert d(None, sets, good, rnds, 3, out, None) == ERR_ARG
        # null arrays: the rules of mi355_bls_batch_verify_many, k == 0 included
        assert f(ctx, None, good, rnds, 3, out) == ERR_ARG
        assert f(ctx, sets, None, rnds, 3, out) == ERR_ARG
        assert f(ctx, sets, good, None, 3, out) == ERR_ARG
        assert f(ctx, sets, good, rnds, 3, None) == ERR_ARG
        assert f(ctx, sets, None, rnds, 0, out) == ERR_ARG
        assert d(ctx, None, good, rnds, 3, out, None) == ERR_ARG
        assert d(ctx, sets, good, rnds, 3, None, None) == ERR_ARG
        # no batches, or empty ones only: 0, every verdict 0, nothing else touched
        out.raw = b"\xaa" * 3
        assert f(ctx, sets, cnt(), rnds, 0, out) == 0 and out.raw == b"\xaa" * 3
        assert f(ctx, sets, cnt(0, 0, 0), rnds, 3, out) == 0 and out.raw == bytes(3)
        out.raw = b"\xaa" * 3
        assert d(ctx, sets, cnt(0, 0, 0), rnds, 3, out, None) == 0 and out.raw == bytes(3)
    g = getattr(L, GT)
    assert g(None, sets, good, rnds, 3, out, gt) == ERR_ARG
    assert g(ctx, sets, good, rnds, 3, out, None) == ERR_ARG          # the values are what the hook is for
    assert g(ctx, sets, None, rnds, 3, out, gt) == ERR_ARG
    gt.raw = b"\xaa" * len(gt.raw)
    out.raw = b"\xaa" * 3
    assert g(ctx, sets, cnt(0, 0, 0), rnds, 3, out, gt) == 0 and out.raw == bytes(3) and gt.raw == bytes(576 * 3)      # empty batches: zero bytes
    assert L.mi355_bls_debug_batch_verify_many_each_passes(None) == ERR_ARG
    assert L.mi355_bls_debug_batch_verify_many_each_passes(ctx) == 0
    assert ctx.raw == bytes(1 << 16)


class _NoCache:
    _h = None


def test_python_mirror_handles_no_batches_and_lists_that_do_not_match(m):
    c = _NoCache()
    assert m.batchVerifyManyEach(c, [], []) == []
    assert m.batchVerifyManyLocate(c, [], []) == []
    assert m.batchVerifyManyEachValues(c, [], []) == ([], [])
    assert m.batchVerifyManyEach_device(c, 0, [], []) == []
    assert m.batchVerifyManyLocate_device(c, 0, [], []) == []
    for f in (m.batchVerifyManyEach, m.batchVerifyManyLocate, m.batchVerifyManyEachValues):
        with pytest.raises(ValueError):
            f(c, [b""], [])
    for f in (m.batchVerifyManyEach_device, m.batchVerifyManyLocate_device):
        with pytest.raises(ValueError):
            f(c, 0, [1, 2], [bytes(32)])
