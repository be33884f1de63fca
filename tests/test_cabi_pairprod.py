"""CPU-only checks of the pairing-product entry points: exported, declared and bound with the header's argument lists; a plain-C caller
(tests/cabi/pairprod_caller.c) that builds against the header alone, links against the library and makes the calls that are decided before a
device is looked at; the argument rules that return MI355_BLS_ERR_ARG without a device; the Python mirror's length checks."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3
COMMON = "mi355_bls_ctx* ctx, const void* %sp1s96, const void* %sq2s192, const size_t* offsets, size_t k, uint32_t flags, "
# name -> the argument list the issue gives it (d_: the device forms' pointer names)
PROTOTYPES = {
    "mi355_bls_pairing_check_each": COMMON % ("", "") + "uint8_t* out, uint8_t* status",
    "mi355_bls_pairing_check_each_device": COMMON % ("d_", "d_") + "uint8_t* out, uint8_t* status, void* stream",
    "mi355_bls_pairing_products": COMMON % ("", "") + "uint8_t* out, uint8_t* status, uint8_t* gt_out",
    "mi355_bls_pairing_products_device": COMMON % ("d_", "d_") + "uint8_t* out, uint8_t* status, uint8_t* gt_out, void* stream",
    "mi355_bls_batch_pairing_check": COMMON % ("", "") + "const uint8_t rnd32[32], uint8_t* status",
    "mi355_bls_batch_pairing_check_device": COMMON % ("d_", "d_") + "const uint8_t rnd32[32], uint8_t* status, void* stream",
    "mi355_bls_batch_pairing_check_locate": COMMON % ("", "") + "const uint8_t rnd32[32], uint8_t* status, uint8_t* out",
    "mi355_bls_batch_pairing_check_locate_device": COMMON % ("d_", "d_") + "const uint8_t rnd32[32], uint8_t* status, uint8_t* out, void* stream",
    "mi355_bls_debug_batch_pairing_check_scalars": COMMON % ("", "") + "const uint64_t* r, uint8_t* status, uint8_t* gt_out",
}
MIRROR = ("pairingCheckEach", "pairingProducts", "batchPairingCheck", "batchPairingCheckLocate", "batchPairingCheckScalars", "pairingCheckEach_device",
          "pairingProducts_device", "batchPairingCheck_device", "batchPairingCheckLocate_device")


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
    for name, value in (("MI355_BLS_PAIR_VALIDATE", "1u"), ("MI355_BLS_PAIR_OK", "0"), ("MI355_BLS_PAIR_P_OFF_CURVE", "1"), ("MI355_BLS_PAIR_P_NOT_IN_G1", "2"),
                        ("MI355_BLS_PAIR_Q_OFF_CURVE", "3"), ("MI355_BLS_PAIR_Q_NOT_IN_G2", "4")):
        assert re.search(r"#define %s %s\b" % (name, value), hdr), name
    assert (m.PAIR_VALIDATE, m.PAIR_OK, m.PAIR_P_OFF_CURVE, m.PAIR_P_NOT_IN_G1, m.PAIR_Q_OFF_CURVE, m.PAIR_Q_NOT_IN_G2) == (1, 0, 1, 2, 3, 4)


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n, want in PROTOTYPES.items():
        args = [" ".join(a.split()) for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        assert args == [a.strip() for a in want.split(",")], n
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args), n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.c_uint32, (n, a)
            elif a.startswith("const size_t*"):
                assert t is ctypes.POINTER(ctypes.c_size_t), (n, a)
            elif a.startswith("const uint64_t*"):
                assert t is ctypes.POINTER(ctypes.c_uint64), (n, a)
            else:
                assert ("*" in a or "[" in a) and t is ctypes.c_void_p, (n, a)


def test_plain_c_caller(m, tmp_path):
    libdir = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "pairprod_caller")
    subprocess.check_call(["gcc", "-Wall", "-Wextra", "-Werror", "-std=c99", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cabi", "pairprod_caller.c"), "-o", exe, "-L", libdir, "-l:" + os.path.basename(m.LIB_PATH),
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.rsplit(" ", 1) for line in out.stdout.splitlines())
    assert kv["err_arg"] == str(ERR_ARG) and kv["codes"] == "01234" and kv["validate_bit"] == "1"
    for name in ("each_null_ctx", "each_device_null_ctx", "products_null_ctx", "products_device_null_ctx", "batch_null_ctx", "batch_device_null_ctx",
                 "locate_null_ctx", "locate_device_null_ctx", "scalars_null_ctx", "null_ctx_k0"):
        assert kv[name] == str(ERR_ARG), name
    assert kv["untouched"] == "1"


def test_argument_rules_that_need_no_device(m):
    """Every rule here is decided before the context is looked into, so a block of zero bytes stands in for one."""
    L, sz = m.lib(), ctypes.c_size_t
    ctx = ctypes.create_string_buffer(1 << 16)
    p1, q2 = ctypes.create_string_buffer(96 * 4), ctypes.create_string_buffer(192 * 4)
    out, st, gt = ctypes.create_string_buffer(b"\xaa" * 2, 2), ctypes.create_string_buffer(b"\xaa" * 4, 4), ctypes.create_string_buffer(b"\xaa" * 1152, 1152)
    rnd = bytes(range(32))
    r = (ctypes.c_uint64 * 2)(3, 5)
    good = (sz * 3)(0, 1, 3)
    ap1, aq2 = ctypes.addressof(p1), ctypes.addressof(q2)

    def calls(p, q, offs, k, flags, status, o=out, g=gt, rn=rnd, rr=r, dev_p=None, only=range(9)):
        """the entry points `only` names, with the same arguments -> their results (a call that passes its argument rules would go on into the
        zero block, so a rule that binds some entry points only is asked of those alone)"""
        dp = dev_p if dev_p is not None else p
        fns = [lambda: L.mi355_bls_pairing_check_each(ctx, p, q, offs, k, flags, o, status),
               lambda: L.mi355_bls_pairing_check_each_device(ctx, dp, q, offs, k, flags, o, status, None),
               lambda: L.mi355_bls_pairing_products(ctx, p, q, offs, k, flags, o, status, g),
               lambda: L.mi355_bls_pairing_products_device(ctx, dp, q, offs, k, flags, o, status, g, None),
               lambda: L.mi355_bls_batch_pairing_check(ctx, p, q, offs, k, flags, rn, status),
               lambda: L.mi355_bls_batch_pairing_check_device(ctx, dp, q, offs, k, flags, rn, status, None),
               lambda: L.mi355_bls_batch_pairing_check_locate(ctx, p, q, offs, k, flags, rn, status, o),
               lambda: L.mi355_bls_batch_pairing_check_locate_device(ctx, dp, q, offs, k, flags, rn, status, o, None),
               lambda: L.mi355_bls_debug_batch_pairing_check_scalars(ctx, p, q, offs, k, flags, rr, status, g)]
        return [fns[i]() for i in only]

    assert calls(ap1, aq2, good, 0, 0, st) == [0] * 9                               # k == 0: 0, nothing written
    assert calls(None, aq2, good, 2, 0, st) == [ERR_ARG] * 9                        # NULL arrays with work to do
    assert calls(ap1, None, good, 2, 0, st) == [ERR_ARG] * 9
    assert calls(ap1, aq2, None, 2, 0, st) == [ERR_ARG] * 9
    assert calls(ap1, aq2, (sz * 3)(0, 2, 1), 2, 0, st) == [ERR_ARG] * 9            # offsets decrease
    assert calls(ap1, aq2, (sz * 3)(1, 2, 3), 2, 0, st) == [ERR_ARG] * 9            # offsets do not start at 0
    assert calls(ap1, aq2, good, 2, 2, st) == [ERR_ARG] * 9                         # unknown flag bits
    assert calls(ap1, aq2, good, 2, 0x80000001, st) == [ERR_ARG] * 9
    assert calls(ap1, aq2, good, 2, 1, None) == [ERR_ARG] * 9                       # validation without the status array
    assert calls(ap1, aq2, good, 2, 0, st, dev_p=ap1 + 2, only=(1, 3, 5, 7)) == [ERR_ARG] * 4      # a misaligned device pointer: the device forms
    assert calls(ap1, aq2, good, 2, 0, st, o=None, only=(0, 1, 2, 3, 6, 7)) == [ERR_ARG] * 6      # no verdict array where the call writes one
    assert calls(ap1, aq2, good, 2, 0, st, g=None, only=(2, 3, 8)) == [ERR_ARG] * 3
    assert calls(ap1, aq2, good, 2, 0, st, rn=None, rr=None, only=(4, 5, 6, 7, 8)) == [ERR_ARG] * 5
    assert ctx.raw == bytes(1 << 16) and out.raw == b"\xaa" * 2 and st.raw == b"\xaa" * 4 and gt.raw == b"\xaa" * 1152


class _NoCache:
    _h = None


def test_python_mirror_checks_lengths(m):
    c = _NoCache()
    p, q = bytes(96), bytes(192)
    for bad in ([[(bytes(95), q)]], [[(p, bytes(191))]], [[(p, q)], [(q, p)]]):
        for fn in (m.pairingCheckEach, m.pairingProducts):
            with pytest.raises(ValueError):
                fn(c, bad)
        with pytest.raises(ValueError):
            m.batchPairingCheck(c, bad, bytes(32))
    with pytest.raises(ValueError):
        m.batchPairingCheck(c, [[(p, q)]], bytes(31))                              # the random bytes are exactly 32
    with pytest.raises(ValueError):
        m.batchPairingCheckLocate(c, [[(p, q)]], b"")
    with pytest.raises(ValueError):
        m.pairingCheckEach(c, [[(p, q)]], flags=2)                                 # unknown flag bits
    with pytest.raises(ValueError):
        m.batchPairingCheckScalars(c, [[(p, q)], []], [3])                         # one scalar per group
    with pytest.raises(ValueError):
        m.batchPairingCheckScalars(c, [[(p, q)]], [1 << 64])
    with pytest.raises(ValueError):
        m.pairingCheckEach_device(c, 0, 0, [1, 2])                                 # offsets start at 0
    with pytest.raises(ValueError):
        m.pairingProducts_device(c, 0, 0, [0, 2, 1])
    assert m.pairingCheckEach(c, []) == [] and m.pairingProducts(c, []) == ([], []) and m.batchPairingCheck(c, [], bytes(32)) is False
    assert m.batchPairingCheckLocate(c, [], bytes(32)) == (False, []) and m.pairingCheckEach_device(c, 0, 0, [0]) == ([], [])
