"""CPU-only checks of the signature aggregation entry points: exported and declared, loud failure without a context, argument validation of the
Python mirror."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_aggregate_signature_sets", "mi355_bls_compress_signatures", "mi355_bls_deserialize_signatures")


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_six_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES + tuple(n + "_device" for n in NAMES):
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in ("aggregateSignatureSets", "compressSignatures", "deserializeSignatures"):
        assert callable(getattr(m, n)) and callable(getattr(m, n + "_device")), n


def test_prototypes_match_the_header(m):
    """the argument lists the ctypes mirror binds are the header's: same count, size_t / uint32_t where the header says so"""
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n in NAMES + tuple(n + "_device" for n in NAMES):
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args), n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.c_uint32, (n, a)
            else:
                assert "*" in a or "[" in a, (n, a)


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    sg, out, offs = bytes(192), ctypes.create_string_buffer(192), (ctypes.c_size_t * 2)(0, 1)
    assert L.mi355_bls_aggregate_signature_sets(None, sg, 1, None, offs, 1, out, out, out) < 0
    assert L.mi355_bls_aggregate_signature_sets_device(None, None, 1, None, offs, 1, None, None, out, None) < 0
    assert L.mi355_bls_compress_signatures(None, sg, 1, out) < 0
    assert L.mi355_bls_compress_signatures_device(None, None, 1, None, None) < 0
    assert L.mi355_bls_deserialize_signatures(None, bytes(96), 1, 0, out, out) < 0
    assert L.mi355_bls_deserialize_signatures_device(None, None, 1, 0, None, out, None) < 0


class _NoCache:
    _h = None


def test_python_mirror_validates_and_handles_empty_input(m):
    c = _NoCache()
    with pytest.raises(ValueError):
        m.aggregateSignatureSets(c, [bytes(191)])
    with pytest.raises(ValueError):
        m.aggregateSignatureSets(c, (bytes(192), [0, 1], [0, 1]))          # offsets[k] is not the length of idx
    with pytest.raises(ValueError):
        m.aggregateSignatureSets(c, (bytes(192), [1 << 32], [0, 1]))
    with pytest.raises(ValueError):
        m.aggregateSignatureSets(c, [bytes(192)], want192=False, want96=False)
    with pytest.raises(ValueError):
        m.compressSignatures(c, bytes(193))
    with pytest.raises(ValueError):
        m.deserializeSignatures(c, bytes(95))
    with pytest.raises(ValueError):
        m.deserializeSignatures(c, bytes(96), sig_uncompressed=True)
    assert m.aggregateSignatureSets(c, []) == (False, b"", b"", b"")
    assert m.aggregateSignatureSets(c, [], want96=False) == (False, b"", None, b"")
    assert m.aggregateSignatureSets_device(c, 0, 0, None, [0], 0, 0) == (False, b"")
    assert m.compressSignatures(c, b"") == [] and m.compressSignatures(c, []) == []
    assert m.deserializeSignatures(c, b"") == (True, b"", b"")
    assert m.deserializeSignatures_device(c, 0, 0, 0) == (True, b"")
