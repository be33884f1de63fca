"""CPU-only checks of the by-message entry points: exported and declared with the header's signatures, loud failure on null pointers and on a
zero scalar in the hook, the Python mirror's handling of empty input."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_batch_verify_by_message", "mi355_bls_batch_verify_by_message_device", "mi355_bls_last_message_groups",
         "mi355_bls_debug_batch_verify_by_message_scalars")
ERR_ARG = -3


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_four_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in ("batchVerifyByMessage", "batchVerifyByMessage_device", "lastMessageGroups", "debugBatchVerifyByMessageScalars"):
        assert callable(getattr(m, n)), n
    assert re.search(r"#define\s+MI355_BLS_ERR_ARG\s+\(?-3\)?", hdr)


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    want = {NAMES[0]: 4, NAMES[1]: 5, NAMES[2]: 1, NAMES[3]: 4}
    for n in NAMES:
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args) == want[n], n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            else:
                assert "*" in a or "[" in a, (n, a)
    # the same argument lists as the calls they shadow
    for mine, theirs in ((NAMES[0], "mi355_bls_batch_verify"), (NAMES[1], "mi355_bls_batch_verify_device"), (NAMES[3], "mi355_bls_debug_batch_verify_scalars")):
        assert list(getattr(L, mine).argtypes) == list(getattr(L, theirs).argtypes), mine


def test_null_pointers_and_a_zero_scalar_are_argument_errors(m):
    L = m.lib()
    rec, rnd = bytes(320), bytes(32)
    one, zero = (ctypes.c_uint64 * 1)(1), (ctypes.c_uint64 * 1)(0)
    assert L.mi355_bls_batch_verify_by_message(None, rec, 1, rnd) == ERR_ARG
    assert L.mi355_bls_batch_verify_by_message(None, rec, 0, rnd) == ERR_ARG          # a null context comes before the n == 0 rule, as in batch_verify
    assert L.mi355_bls_batch_verify(None, rec, 0, rnd) == ERR_ARG
    assert L.mi355_bls_batch_verify_by_message_device(None, None, 1, rnd, None) == ERR_ARG
    assert L.mi355_bls_last_message_groups(None) == ERR_ARG
    assert L.mi355_bls_debug_batch_verify_by_message_scalars(None, rec, 1, one) == ERR_ARG
    assert L.mi355_bls_debug_batch_verify_by_message_scalars(None, rec, 1, zero) == ERR_ARG
    assert L.mi355_bls_debug_batch_verify_by_message_scalars(None, None, 1, one) == ERR_ARG
    assert L.mi355_bls_debug_batch_verify_by_message_scalars(None, rec, 1, None) == ERR_ARG


class _NoCache:
    _h = None


def test_python_mirror_handles_empty_and_mismatched_input(m):
    c = _NoCache()
    assert m.batchVerifyByMessage(c, b"", bytes(32)) is False
    with pytest.raises(ValueError):
        m.debugBatchVerifyByMessageScalars(c, bytes(320), [1, 2])
