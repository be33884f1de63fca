"""CPU-only checks of the threshold-signature recovery entry points: exported and declared, loud failure without a context, argument validation
of the Python mirror, the k == 0 return."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_recover_signature_sets", "mi355_bls_recover_signature_sets_device")


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_two_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert re.search(r"#define MI355_BLS_REC_ZERO_ID 6\b", hdr) and re.search(r"#define MI355_BLS_REC_DUP_ID 7\b", hdr)
    assert (m.REC_ZERO_ID, m.REC_DUP_ID) == (6, 7)
    assert callable(m.recoverSignatureSets) and callable(m.recoverSignatureSets_device) and callable(m.idFromUint32)


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
            else:
                assert "*" in a, (n, a)


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    sg, out, offs = bytes(192), ctypes.create_string_buffer(192), (ctypes.c_size_t * 2)(0, 1)
    assert L.mi355_bls_recover_signature_sets(None, sg, 1, None, offs, 1, bytes(32), out, out, out) < 0
    assert L.mi355_bls_recover_signature_sets_device(None, None, 1, None, offs, 1, None, None, None, out, None) < 0


class _NoCache:
    _h = None


def test_id_from_uint32(m):
    assert m.idFromUint32([0, 0, 0, 0, 0, 0, 0, 3]) == (3 << 224).to_bytes(32, "little")         # the reference test's blsIdFromUint32(3)
    assert m.idFromUint32([1, 2, 3, 4, 5, 6, 7, 8]) == b"".join(bytes([i, 0, 0, 0]) for i in range(1, 9))
    with pytest.raises(ValueError):
        m.idFromUint32([0] * 7)
    with pytest.raises(ValueError):
        m.idFromUint32([0] * 7 + [1 << 32])


def test_python_mirror_validates_and_handles_empty_input(m):
    c = _NoCache()
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, [bytes(192)], [[bytes(31)]])                        # an id that is not 32 bytes
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, [bytes(192)], bytes(33))
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, [bytes(384)], [[bytes(32)]])                        # one id for two members
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, (bytes(192), [0, 0], [0, 2]), bytes(96))
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, [bytes(192)], [[bytes(32)]], want192=False, want96=False)
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, [bytes(191)], [[bytes(32)]])
    with pytest.raises(ValueError):
        m.recoverSignatureSets(c, [], [[bytes(32)]])                                  # ids without members
    assert m.recoverSignatureSets(c, [], []) == (False, b"", b"", b"")
    assert m.recoverSignatureSets(c, [], b"", want96=False) == (False, b"", None, b"")
    assert m.recoverSignatureSets(c, [], [], want192=False) == (False, None, b"", b"")
    assert m.recoverSignatureSets_device(c, 0, 0, None, [0], 0, 0, 0) == (False, b"")
