"""CPU-only checks of the entry points of the key aggregation by participation bits: exported and declared, bound with the header's
prototypes, loud failure without a context, argument validation of the Python mirror before the cache is touched."""
import ctypes
import re
import subprocess

import pytest

NAMES = ("mi355_bls_aggregate_sets_bits", "mi355_bls_fast_aggregate_verify_each_bits", "mi355_bls_batch_fast_aggregate_verify_bits")
HOOK = "mi355_bls_debug_aggregate_bits_routes"


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as ge
    ge.build()
    return ge.load_package()


def test_seven_symbols_are_declared_and_exported(m):
    hdr = open(m.HEADER_PATH).read()
    declared = set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", m.LIB_PATH]).decode()
    exported = set(re.findall(r" T (mi355_[a-z0-9_]+)$", out, re.M))
    L = ctypes.CDLL(m.LIB_PATH)
    for n in NAMES + tuple(n + "_device" for n in NAMES) + (HOOK,):
        assert n in declared and n in exported and hasattr(L, n), n
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    for n in ("aggregateSetsBits", "fastAggregateVerifyEachBits", "batchFastAggregateVerifyBits"):
        assert callable(getattr(m, n)) and callable(getattr(m, n + "_device")), n
    assert callable(m.debug_aggregate_bits_routes)
    assert "subtractAll" in hdr and "bls_sig_min_pubkey.nim:234-258" in hdr


def test_prototypes_match_the_header(m):
    hdr = re.sub(r"/\*.*?\*/", "", open(m.HEADER_PATH).read(), flags=re.S)
    L = m.lib()
    for n in NAMES + tuple(n + "_device" for n in NAMES) + (HOOK,):
        args = [a.strip() for a in re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1).split(",")]
        bound = getattr(L, n).argtypes
        assert len(bound) == len(args), n
        for a, t in zip(args, bound):
            if a.startswith("size_t "):
                assert t is ctypes.c_size_t, (n, a)
            elif a.startswith("uint32_t ") and "[" not in a:
                assert t is ctypes.c_uint32, (n, a)
            else:
                assert "*" in a or "[" in a, (n, a)
        names = [re.split(r"[ *]", a.split("[")[0])[-1] for a in args]
        if n != HOOK:
            dev = n.endswith("_device")
            lead = ["ctx", "d_keys" if dev else "keys", "n_table", "d_idx" if dev else "idx", "c_offsets", "m", "d_committee_aggs" if dev else "committee_aggs",
                    "agg_stride", "which", "d_bits" if dev else "bits", "k"]
            assert names[:11] == lead, n


def test_calls_without_a_context_fail_with_a_negative_code(m):
    L = m.lib()
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    offs, which = (sz * 2)(0, 1), (u32 * 1)(0)
    key, out, st = bytes(96), ctypes.create_string_buffer(320), ctypes.create_string_buffer(1)
    host = (None, key, 1, None, offs, 1, None, 96, which, b"\x01", 1, bytes(32), bytes(192))
    dev = (None, None, 1, None, offs, 1, None, 96, which, None, 1, None, None)
    assert L.mi355_bls_aggregate_sets_bits(*host, out, st) < 0
    assert L.mi355_bls_aggregate_sets_bits_device(*dev, None, st, None) < 0
    assert L.mi355_bls_fast_aggregate_verify_each_bits(*host, st) < 0
    assert L.mi355_bls_fast_aggregate_verify_each_bits_device(*dev, st, None) < 0
    assert L.mi355_bls_batch_fast_aggregate_verify_bits(*host, bytes(32)) < 0
    assert L.mi355_bls_batch_fast_aggregate_verify_bits_device(*dev, bytes(32), None) < 0
    assert L.mi355_bls_debug_aggregate_bits_routes(None, (u32 * 2)()) < 0


class _NoCache:
    _h = None


def test_python_mirror_validates_before_the_cache_is_touched(m):
    c = _NoCache()
    two = [bytes(96 * 9), bytes(96 * 3)]                                        # committees of 9 and 3 keys
    ok = dict(which=[0, 1, 0], bits=[b"\x01\x00", b"\x07", b"\xff\x01"], messages=bytes(96), signatures=bytes(576))
    for f, tail in ((m.aggregateSetsBits, ()), (m.fastAggregateVerifyEachBits, ()), (m.batchFastAggregateVerifyBits, (bytes(32),))):
        def call(committees=two, committee_aggs=None, agg_stride=96, **kw):
            a = dict(ok, **kw)
            return f(c, committees, a["which"], a["bits"], a["messages"], a["signatures"], *tail, committee_aggs=committee_aggs, agg_stride=agg_stride)
        with pytest.raises(ValueError):
            call(committees=[bytes(95)])                                        # not whole keys
        with pytest.raises(ValueError):
            call(which=[0, 2, 0])                                               # a committee that is not there
        with pytest.raises(ValueError):
            call(which=[0, -1, 0])
        with pytest.raises(ValueError):
            call(bits=[b"\x01", b"\x07", b"\xff\x01"])                          # a field of the wrong length
        with pytest.raises(ValueError):
            call(bits=b"\x01\x00\x07\xff")                                      # packed: one byte short
        with pytest.raises(ValueError):
            call(bits=[b"\x01\x00", b"\x07"])                                   # one field per set
        with pytest.raises(ValueError):
            call(messages=bytes(64))
        with pytest.raises(ValueError):
            call(signatures=bytes(575))
        with pytest.raises(ValueError):
            call(committee_aggs=bytes(192), agg_stride=95)
        with pytest.raises(ValueError):
            call(committee_aggs=bytes(192), agg_stride=98)
        with pytest.raises(ValueError):
            call(committee_aggs=bytes(96 + 320 - 1), agg_stride=320)            # too short for two aggregates 320 bytes apart
        with pytest.raises(ValueError):
            call(committees=(bytes(96 * 4), [0, 1, 2], [0, 2]))                 # offsets[m] is not the length of idx
        with pytest.raises(ValueError):
            call(committees=(bytes(96 * 4), None, [0, 3, 2]), which=[0], bits=b"\x01", messages=bytes(32), signatures=bytes(192))      # decreasing
        with pytest.raises(m.BlsGpuError):
            call()                                                              # valid arguments reach the library, which refuses the missing context
    with pytest.raises(ValueError):
        m.batchFastAggregateVerifyBits(c, two, ok["which"], ok["bits"], ok["messages"], ok["signatures"], bytes(31))
    assert m.aggregateSetsBits(c, two, [], b"", b"", b"") == (False, b"", b"")
    assert m.fastAggregateVerifyEachBits(c, two, [], [], b"", b"") == []
    assert m.batchFastAggregateVerifyBits(c, two, [], b"", b"", b"", bytes(32)) is False
    assert m.aggregateSetsBits_device(c, 0, 12, None, [0, 9, 12], None, 96, [], 0, 0, 0, 0) == (False, b"")
    assert m.fastAggregateVerifyEachBits_device(c, 0, 12, None, [0, 9, 12], None, 96, [], 0, 0, 0) == []
    assert m.batchFastAggregateVerifyBits_device(c, 0, 12, None, [0, 9, 12], None, 96, [], 0, 0, 0, bytes(32)) is False
    with pytest.raises(ValueError):
        m.aggregateSetsBits_device(c, 0, 12, None, [0, 9, 12], None, 96, [2], 0, 0, 0, 0)
