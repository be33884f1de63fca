"""CPU-only checks of the key-table entry points (mi355_bls_deserialize_public_keys, mi355_bls_admit_keys and their _device forms): exported
and declared, the status constant, the bound prototypes, loud failure without a context, argument validation of the Python mirror."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_deserialize_public_keys", "mi355_bls_deserialize_public_keys_device", "mi355_bls_admit_keys", "mi355_bls_admit_keys_device")


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
    for n in ("deserializePublicKeys", "admitKeys"):
        assert callable(getattr(m, n)) and callable(getattr(m, n + "_device")), n


def test_bad_proof_constant(m):
    hdr = open(m.HEADER_PATH).read()
    assert re.search(r"^#define MI355_BLS_KEY_BAD_PROOF 8\s*$", hdr, re.M)
    assert m.KEY_BAD_PROOF == 8


def test_prototypes_match_the_header(m):
    """the argument lists the ctypes mirror binds are the header's: same count, size_t / uint32_t where the header says so"""
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n in NAMES:
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert bound is not None and len(bound) == len(args), n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t "):
                assert t is ctypes.c_uint32, (n, a)
            else:
                assert "*" in a or "[" in a, (n, a)
                assert t in (ctypes.c_void_p, ctypes.c_char_p), (n, a)
    assert len(L.mi355_bls_admit_keys.argtypes) == 8 and len(L.mi355_bls_admit_keys_device.argtypes) == 9
    assert len(L.mi355_bls_deserialize_public_keys.argtypes) == 6 and len(L.mi355_bls_deserialize_public_keys_device.argtypes) == 7


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    out, st, rnd = ctypes.create_string_buffer(96), ctypes.create_string_buffer(1), bytes(32)
    assert L.mi355_bls_deserialize_public_keys(None, bytes(48), 1, 0, out, st) < 0
    assert L.mi355_bls_deserialize_public_keys_device(None, None, 1, 0, None, st, None) < 0
    assert L.mi355_bls_admit_keys(None, bytes(48), bytes(96), 1, 0, rnd, out, st) < 0
    assert L.mi355_bls_admit_keys_device(None, None, None, 1, 0, rnd, None, st, None) < 0
    # and with nothing to do: still no context, still an error
    assert L.mi355_bls_deserialize_public_keys(None, None, 0, 0, None, None) < 0
    assert L.mi355_bls_admit_keys(None, None, None, 0, 0, rnd, None, st) < 0


class _NoCache:
    _h = None


def test_python_mirror_validates_and_handles_empty_input(m):
    c, rnd = _NoCache(), bytes(32)
    with pytest.raises(ValueError):
        m.deserializePublicKeys(c, bytes(47))
    with pytest.raises(ValueError):
        m.deserializePublicKeys(c, bytes(48), pk_uncompressed=True)               # 48 is no multiple of 96
    with pytest.raises(ValueError):
        m.admitKeys(c, bytes(49), bytes(96), rnd)
    with pytest.raises(ValueError):
        m.admitKeys(c, bytes(48), bytes(96), rnd, pk_uncompressed=True)
    with pytest.raises(ValueError):
        m.admitKeys(c, bytes(48), bytes(95), rnd)
    with pytest.raises(ValueError):
        m.admitKeys(c, bytes(96), bytes(96), rnd)                                 # two keys, one proof
    with pytest.raises(ValueError):
        m.admitKeys(c, [bytes(48)], [bytes(192), bytes(192)], rnd, sig_uncompressed=True)
    with pytest.raises(ValueError):
        m.admitKeys(c, bytes(48), bytes(96), bytes(31))
    with pytest.raises(ValueError):
        m.admitKeys(c, b"", b"", bytes(31))                                       # checked before the empty table returns
    with pytest.raises(ValueError):
        m.admitKeys_device(c, 0, 0, 1, bytes(31), 0)
    assert m.deserializePublicKeys(c, b"") == (True, b"", b"") and m.deserializePublicKeys(c, []) == (True, b"", b"")
    assert m.deserializePublicKeys_device(c, 0, 0, 0) == (True, b"")
    assert m.admitKeys(c, b"", b"", rnd) == (True, b"", b"")
    assert m.admitKeys_device(c, 0, 0, 0, rnd, 0) == (True, b"")
