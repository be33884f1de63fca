"""CPU-only checks of the popVerify entry points: exported and declared, loud failure without a context, argument validation of the Python mirror."""
import ctypes
import re

import pytest

NAMES = ("mi355_bls_pop_verify_each", "mi355_bls_batch_pop_verify", "mi355_bls_batch_pop_verify_locate", "mi355_bls_compress_public_keys", "mi355_bls_pop_prove")


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_new_names_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES + tuple(n + "_device" for n in NAMES) + ("mi355_bls_debug_pop_verify_each_gt",):
        assert n in declared, n
        assert hasattr(L, n), n
    for n in ("popVerifyEach", "batchPopVerify", "batchPopVerifyLocate", "compressPublicKeys", "popProve"):
        assert callable(getattr(m, n)) and callable(getattr(m, n + "_device")), n


def test_calls_without_a_context_fail_with_a_negative_code(m):
    """what a host without a GPU is left with: mi355_bls_ctx_create fails, and every entry point refuses the null context"""
    L = m.lib()
    pk, pr, rnd, out = bytes(96), bytes(192), bytes(32), ctypes.create_string_buffer(576)
    assert L.mi355_bls_pop_verify_each(None, pk, pr, 1, out) < 0
    assert L.mi355_bls_pop_verify_each_device(None, None, None, 1, out, None) < 0
    assert L.mi355_bls_debug_pop_verify_each_gt(None, pk, pr, 1, out, out) < 0
    assert L.mi355_bls_batch_pop_verify(None, pk, pr, 1, rnd) < 0
    assert L.mi355_bls_batch_pop_verify_device(None, None, None, 1, rnd, None) < 0
    assert L.mi355_bls_batch_pop_verify_locate(None, pk, pr, 1, rnd, out) < 0
    assert L.mi355_bls_batch_pop_verify_locate_device(None, None, None, 1, rnd, out, None) < 0
    assert L.mi355_bls_compress_public_keys(None, pk, 1, out) < 0
    assert L.mi355_bls_compress_public_keys_device(None, None, 1, None, None) < 0
    assert L.mi355_bls_pop_prove(None, bytes(32), 1, out, out, out) < 0
    assert L.mi355_bls_pop_prove_device(None, None, 1, None, None, None, out) < 0
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(m.BlsGpuError):
            m.BatchedBLSVerifierCache.init(max_sets=16)


class _NoCache:
    _h = None


def test_python_mirror_validates_lengths(m):
    c = _NoCache()
    for pks, proofs in ((bytes(95), bytes(192)), (bytes(96), bytes(191)), (bytes(192), bytes(192)), (bytes(96), bytes(384)), ([bytes(96)], [bytes(96)])):
        for fn in (m.popVerifyEach, m.popVerifyEachValues):
            with pytest.raises(ValueError):
                fn(c, pks, proofs)
        for fn in (m.batchPopVerify, m.batchPopVerifyLocate):
            with pytest.raises(ValueError):
                fn(c, pks, proofs, bytes(32))
    for rnd in (bytes(31), bytes(33), 32):
        with pytest.raises(ValueError):
            m.batchPopVerify(c, bytes(96), bytes(192), rnd)
        with pytest.raises(ValueError):
            m.batchPopVerifyLocate(c, bytes(96), bytes(192), rnd)
        with pytest.raises(ValueError):
            m.batchPopVerify_device(c, 0, 0, 1, rnd)
    with pytest.raises(ValueError):
        m.compressPublicKeys(c, bytes(97))
    with pytest.raises(ValueError):
        m.popProve(c, bytes(33))


def test_python_mirror_on_empty_input(m):
    c = _NoCache()
    assert m.popVerifyEach(c, b"", b"") == [] and m.popVerifyEach(c, [], []) == []
    assert m.batchPopVerify(c, b"", b"", bytes(32)) is False
    assert m.batchPopVerifyLocate(c, b"", b"", bytes(32)) == (False, [])
    assert m.compressPublicKeys(c, b"") == []
    assert m.popProve(c, b"") == (True, b"", b"", b"")
