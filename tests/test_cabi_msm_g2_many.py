"""CPU-only checks of the G2 many-MSM and Jacobian-to-affine entry points: exported, declared and bound with the header's argument lists; a
plain-C caller (tests/cabi/msm_g2_many_caller.c) that builds against the header alone; the argument rules that are decided before the context is
looked into; the Python mirror's handling of k == 0, n == 0 and lengths that do not divide."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3
PROTOTYPES = {
    "mi355_bls_p2s_mult_pippenger_many": 8,
    "mi355_bls_p2s_mult_pippenger_many_device": 10,
    "mi355_bls_p1s_to_affine": 4,
    "mi355_bls_p1s_to_affine_device": 5,
    "mi355_bls_p2s_to_affine": 4,
    "mi355_bls_p2s_to_affine_device": 5,
    "mi355_bls_debug_to_affine_set_run": 2,
}
MIRROR = ("p2s_mult_pippenger_many", "p2s_mult_pippenger_many_device", "p1s_to_affine", "p1s_to_affine_device", "p2s_to_affine", "p2s_to_affine_device",
          "debug_to_affine_set_run")


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_the_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in PROTOTYPES:
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in MIRROR:
        assert callable(getattr(m, n)), n


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n, count in PROTOTYPES.items():
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args) == count, n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("const size_t*"):
                assert t is ctypes.POINTER(ctypes.c_size_t), (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.c_uint32, (n, a)
            else:
                assert "*" in a and t is ctypes.c_void_p, (n, a)


def test_plain_c_caller(m, tmp_path):
    libdir = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "msm_g2_many_caller")
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-std=c99", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cabi", "msm_g2_many_caller.c"), "-o", exe, "-L", libdir, "-l:" + os.path.basename(m.LIB_PATH),
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.rsplit(" ", 1) for line in out.stdout.splitlines())
    assert kv["err_arg"] == str(ERR_ARG)
    for name in ("many_null_ctx", "many_null_ctx_k0", "many_device_null_ctx", "p1s_to_affine_null_ctx", "p1s_to_affine_null_ctx_n0", "p1s_to_affine_device_null_ctx",
                 "p2s_to_affine_null_ctx", "p2s_to_affine_device_null_ctx", "set_run_null_ctx"):
        assert kv[name] == str(ERR_ARG), name
    assert kv["out_untouched"] == "1"


def offs(*v):
    return (ctypes.c_size_t * len(v))(*v)


def test_argument_rules_that_need_no_device(m):
    """A null context is refused before every other rule.  Every other rule here is decided before the context is looked into, so a block of
    zero bytes stands in for one: no call below may get as far as using it."""
    L = m.lib()
    many, dev = L.mi355_bls_p2s_mult_pippenger_many, L.mi355_bls_p2s_mult_pippenger_many_device
    ctx = ctypes.create_string_buffer(1 << 16)
    out = ctypes.create_string_buffer(288 * 4)
    pts, sc = ctypes.create_string_buffer(192 * 4), ctypes.create_string_buffer(32 * 8)
    good = offs(0, 2, 4)
    assert many(None, out, pts, 4, sc, good, 2, 255) == ERR_ARG and many(None, None, None, 0, None, None, 0, 0) == ERR_ARG
    assert dev(None, out, None, pts, 4, sc, good, 2, 255, None) == ERR_ARG and dev(None, None, None, None, 0, None, None, 0, 255, None) == ERR_ARG
    out.raw = b"\xaa" * len(out.raw)
    assert many(ctx, out, pts, 4, sc, offs(0), 0, 255) == 0 and many(ctx, None, None, 4, None, None, 0, 0) == 0        # k == 0 touches nothing
    assert dev(ctx, out, None, pts, 4, sc, None, 0, 255, None) == 0 and dev(ctx, None, None, None, 0, None, None, 0, 999, None) == 0
    assert out.raw == b"\xaa" * len(out.raw)
    assert many(ctx, out, None, 4, sc, good, 2, 255) == ERR_ARG and many(ctx, out, pts, 4, None, good, 2, 255) == ERR_ARG
    assert dev(ctx, out, None, None, 4, sc, good, 2, 255, None) == ERR_ARG and dev(ctx, out, None, pts, 4, None, None, 2, 255, None) == ERR_ARG
    for bad in (offs(0, 3, 2, 4), offs(1, 2, 3, 4), offs(0, 1, 2, 3), offs(0, 1, 2, 5)):
        assert many(ctx, out, pts, 4, sc, bad, 3, 255) == ERR_ARG and dev(ctx, out, None, pts, 4, sc, bad, 3, 255, None) == ERR_ARG
    for nbits in (0, 257):
        assert many(ctx, out, pts, 4, sc, good, 2, nbits) == ERR_ARG and dev(ctx, out, None, pts, 4, sc, None, 2, nbits, None) == ERR_ARG
    big = (1 << 28) + 1
    assert many(ctx, out, pts, big + 2, sc, offs(0, 1, big + 1, big + 2), 3, 255) == ERR_ARG
    assert dev(ctx, out, None, pts, big, sc, None, 2, 255, None) == ERR_ARG
    assert many(ctx, None, pts, 4, sc, good, 2, 255) == ERR_ARG and dev(ctx, None, None, pts, 4, sc, good, 2, 255, None) == ERR_ARG      # no output
    assert dev(ctx, None, ctypes.c_void_p(ctypes.addressof(out) + 2), pts, 4, sc, good, 2, 255, None) == ERR_ARG                          # d_out not 4-byte aligned
    # to_affine: n == 0 touches nothing; NULL arrays with work to do; a device pointer that is not 4-byte aligned
    for host, device in ((L.mi355_bls_p1s_to_affine, L.mi355_bls_p1s_to_affine_device), (L.mi355_bls_p2s_to_affine, L.mi355_bls_p2s_to_affine_device)):
        assert host(None, pts, 0, out) == ERR_ARG and device(None, pts, 0, out, None) == ERR_ARG
        assert host(ctx, None, 0, None) == 0 and device(ctx, None, 0, None, None) == 0
        assert host(ctx, None, 2, out) == ERR_ARG and host(ctx, pts, 2, None) == ERR_ARG
        assert device(ctx, None, 2, out, None) == ERR_ARG and device(ctx, pts, 2, None, None) == ERR_ARG
        base = ctypes.addressof(pts)
        assert device(ctx, ctypes.c_void_p(base + 1), 1, out, None) == ERR_ARG and device(ctx, pts, 1, ctypes.c_void_p(ctypes.addressof(out) + 2), None) == ERR_ARG
    assert out.raw == b"\xaa" * len(out.raw)
    assert L.mi355_bls_debug_to_affine_set_run(None, 1) == ERR_ARG
    assert ctx.raw == bytes(1 << 16)


class _NoCache:
    _h = None


def test_python_mirror_handles_nothing_to_do_and_lengths_that_do_not_divide(m):
    c = _NoCache()
    assert m.p2s_mult_pippenger_many(c, b"", b"", offsets=[0]) == [] and m.p2s_mult_pippenger_many(c, b"", b"") == []
    assert m.p2s_mult_pippenger_many(c, bytes(192 * 3), b"") == [] and m.p2s_mult_pippenger_many_device(c, 0, 0, 0, None, 0) == []
    assert m.p1s_to_affine(c, b"") == b"" and m.p2s_to_affine(c, b"") == b""
    for bad in (lambda: m.p2s_mult_pippenger_many(c, bytes(192 * 3), bytes(32 * 7)), lambda: m.p2s_mult_pippenger_many(c, bytes(96), bytes(32)),
                lambda: m.p2s_mult_pippenger_many(c, bytes(192 * 3), bytes(32 * 3), offsets=[0, 2]),
                lambda: m.p2s_mult_pippenger_many(c, bytes(192 * 3), bytes(32 * 2), offsets=[0, 3]),
                lambda: m.p2s_mult_pippenger_many_device(c, 0, 4, 0, [0, 4], 2), lambda: m.p1s_to_affine(c, bytes(143)), lambda: m.p2s_to_affine(c, bytes(144))):
        with pytest.raises(ValueError):
            bad()
