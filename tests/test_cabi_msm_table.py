"""CPU-only checks of the fixed-base table MSM entry points: exported, declared and bound with the header's argument lists; a plain-C caller
(tests/cabi/msm_table_caller.c) that builds against the header alone, links against the library and makes the calls that are decided before a
device is looked at; the Python mirror's argument handling."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3
# name -> (result type in the header, number of arguments)
PROTOTYPES = {
    "mi355_bls_p1s_table_sizeof": ("size_t", 3),
    "mi355_bls_p1s_table_create": ("int", 6),
    "mi355_bls_p1s_table_create_device": ("int", 7),
    "mi355_bls_p1s_table_destroy": ("void", 1),
    "mi355_bls_p1s_mult_table": ("int", 5),
    "mi355_bls_p1s_mult_table_device": ("int", 6),
    "mi355_bls_p1s_mult_table_many": ("int", 6),
    "mi355_bls_p1s_mult_table_many_device": ("int", 8),
    "mi355_bls_debug_p1s_table_rows": ("int", 6),
    "mi355_bls_debug_p1s_table_last_plan": ("int", 2),
    "mi355_bls_debug_p1s_table_set_plan": ("int", 3),
}
MIRROR = ("p1s_table_sizeof", "p1s_table_create", "p1s_table_create_device", "p1s_table_destroy", "p1s_mult_table", "p1s_mult_table_device", "p1s_mult_table_many",
          "p1s_mult_table_many_device", "debug_p1s_table_rows", "debug_p1s_table_last_plan", "debug_p1s_table_set_plan")


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
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))      # the header's prototype count is the library's exports
    for n in MIRROR:
        assert callable(getattr(m, n)), n


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    assert "typedef struct mi355_bls_p1s_table mi355_bls_p1s_table;" in hdr
    for n, (res, count) in PROTOTYPES.items():
        args = [a.strip() for a in re.search(r"\b%s %s\s*\(([^)]*)\)" % (res, n), hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args) == count, n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t ") and "[" not in a:
                assert t is ctypes.c_uint32, (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.POINTER(ctypes.c_uint32), (n, a)
            else:
                assert ("*" in a or "[" in a) and t is ctypes.c_void_p, (n, a)


def test_plain_c_caller(m, tmp_path):
    libdir = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "msm_table_caller")
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-std=c99", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cabi", "msm_table_caller.c"), "-o", exe, "-L", libdir, "-l:" + os.path.basename(m.LIB_PATH),
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.rsplit(" ", 1) for line in out.stdout.splitlines())
    assert kv["err_arg"] == str(ERR_ARG)
    assert kv["sizeof_4096_12_255"] == str(22 * 4096 * 128)                                      # 256 bits in 12-bit windows
    assert kv["sizeof_rule_4096"] == str(32 * 4096 * 128)                                        # the rule's choice at 4 096 points: 8-bit windows
    assert kv["sizeof_refused"] == "0"
    for name in ("create_null_ctx", "create_device_null_ctx", "mult_null_ctx", "mult_device_null_ctx", "many_null_ctx", "many_device_null_ctx", "rows_null_table",
                 "last_plan_null_ctx", "set_plan_null_ctx"):
        assert kv[name] == str(ERR_ARG), name
    assert kv["table_still_null"] == "1" and kv["out_untouched"] == "1"


def test_argument_rules_that_need_no_device(m):
    """Every rule here is decided before the context is looked into, so a block of zero bytes stands in for one (and for a table)."""
    L = m.lib()
    ctx = ctypes.create_string_buffer(1 << 16)
    out = ctypes.create_string_buffer(144)
    h = ctypes.c_void_p()
    pts, sc = ctypes.create_string_buffer(96 * 4), ctypes.create_string_buffer(32 * 4)
    for n, wbits, nbits in ((0, 8, 255), (4, 4, 255), (4, 17, 255), (4, 8, 0), (4, 8, 257), ((1 << 31) // 22 + 1, 12, 255)):
        assert L.mi355_bls_p1s_table_create(ctx, ctypes.byref(h), pts, n, wbits, nbits) == ERR_ARG, (n, wbits, nbits)
        assert L.mi355_bls_p1s_table_create_device(ctx, ctypes.byref(h), pts, n, wbits, nbits, None) == ERR_ARG, (n, wbits, nbits)
    assert L.mi355_bls_p1s_table_create(ctx, None, pts, 4, 8, 255) == ERR_ARG and L.mi355_bls_p1s_table_create(ctx, ctypes.byref(h), None, 4, 8, 255) == ERR_ARG
    assert not h
    # k == 0 returns 0 and touches nothing; a null table, null scalars, no output
    out.raw = b"\xaa" * 144
    assert L.mi355_bls_p1s_mult_table_many(ctx, out, None, None, 0, 999) == 0
    assert L.mi355_bls_p1s_mult_table_many_device(ctx, out, None, None, None, 0, 0, None) == 0
    assert out.raw == b"\xaa" * 144
    assert L.mi355_bls_p1s_mult_table(ctx, out, None, sc, 255) == ERR_ARG
    assert L.mi355_bls_p1s_mult_table_many_device(ctx, out, None, None, sc, 2, 255, None) == ERR_ARG
    assert ctx.raw == bytes(1 << 16)


class _NoCache:
    _h = None


def test_python_mirror_checks_lengths(m):
    c = _NoCache()
    tab = m.P1sTable(None, 3, 8, 255)
    with pytest.raises(ValueError):
        m.p1s_table_create(c, bytes(95))
    with pytest.raises(ValueError):
        m.p1s_mult_table(c, tab, bytes(32 * 2))
    with pytest.raises(ValueError):
        m.p1s_mult_table_many(c, tab, bytes(32 * 4))
    assert m.p1s_mult_table_many(c, tab, b"") == []
    m.p1s_table_destroy(tab)
    m.p1s_table_destroy(None)
    assert m.p1s_table_sizeof(4096, 16, 255) == 16 * 4096 * 128 and m.p1s_table_sizeof(0) == 0
