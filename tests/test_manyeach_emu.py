"""The per-batch pass of mi355_bls_batch_verify_many_each executed on the CPU under the bounds tracker (tests/host_emu/manyeach.cpp): the lane
bodies of csrc/manyeach.hpp with the combsets / aggveach bodies they join, over the plan's own slices and tables, for tiny batches of 1, 2, 3
and 9 sets, one forged batch and one with an infinity key.  Every batch's verdict and 576-byte value equal the C restatement's batchVerify on
that batch alone (whose scalars the pass is given), in one slice and cut into slices that hold a batch or two."""
import ctypes
import hashlib
import os
import subprocess

import pytest

import c_oracle as co

HERE = os.path.dirname(os.path.abspath(__file__))
NT = 4
SIZES = [1, 2, 3, 9, 0, 3, 2]             # batch 5 is forged, batch 6 holds an infinity key


def rnd_of(i):
    return hashlib.sha256(b"manyeach emu" + bytes([i])).digest()


@pytest.fixture(scope="module")
def batches():
    bs = [co.make_batch(n, seed=700 + 13 * i) if n else b"" for i, n in enumerate(SIZES)]
    b = bytearray(bs[5])
    b[320 * 1 + 96 + 7] ^= 2                                  # another message in batch 5
    bs[5] = bytes(b)
    b = bytearray(bs[6])
    b[320:320 + 96] = bytes(96)                               # an infinity key in batch 6
    bs[6] = bytes(b)
    return bs


@pytest.fixture(scope="module")
def oracle(batches):
    """per batch: (verdict, {"r", "gt"}) of batchVerify on that batch alone - the serial chain below three sets, as the dispatch has it"""
    out = []
    for i, b in enumerate(batches):
        if not b:
            out.append((False, {"r": [], "gt": bytes(576)}))
            continue
        out.append(co.batch_verify(b, rnd_of(i), NT if len(b) // 320 >= 3 else 0, stages=True))
    return out


@pytest.fixture(scope="module")
def emu(batches, oracle):
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_manyeach.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libmanyeach.so"))
    sz = ctypes.c_size_t
    L.emu_manyeach.argtypes = [ctypes.c_char_p, ctypes.POINTER(sz), sz, ctypes.POINTER(ctypes.c_uint64), sz, sz, ctypes.c_char_p, ctypes.c_char_p]
    k = len(SIZES)
    r = [x for _, st in oracle for x in st["r"]]
    assert len(r) == sum(SIZES) and all(r)

    def run(cap_sets, cap_pairs):
        v, gt = ctypes.create_string_buffer(k), ctypes.create_string_buffer(576 * k)
        ns = L.emu_manyeach(b"".join(batches), (sz * k)(*SIZES), k, (ctypes.c_uint64 * len(r))(*r), cap_sets, cap_pairs, v, gt)
        raw = gt.raw
        return ns, [(v.raw[i], raw[576 * i:576 * i + 576]) for i in range(k)]
    return run


@pytest.fixture(scope="module")
def plain(emu):
    return emu(1 << 16, 1 << 17)


def test_verdicts_and_values_equal_the_oracle_per_batch(plain, oracle):
    ns, res = plain
    assert ns == 1
    assert [ok for ok, _ in res] == [1, 1, 1, 1, 0, 0, 0]
    for i, ((ok, gt), (want_ok, st)) in enumerate(zip(res, oracle)):
        assert bool(ok) == want_ok, i
        if i == 6:
            continue                                          # the restatement stops at the infinity key (update returns false): verdict only
        assert gt == st["gt"], i
    assert res[4][1] == bytes(576)                            # the empty batch: no lane, zero bytes
    assert res[5][1] != oracle[2][1]["gt"]                    # the forged batch has a value of its own, not one


def test_slices_change_nothing(emu, plain):
    ns, res = emu(9, 12)                                      # 1 + 2 + 3 sets and 3 slots; the batch of nine alone; 3 + 2 sets
    assert ns == 3 and res == plain[1]
    ns, res = emu(9, 10)                                      # the pair store binds: a slice filled exactly by nine sets and one slot
    assert ns == 3 and res == plain[1]
    ns, res = emu(3, 4)                                       # a batch or two per slice; the batch of nine goes to the single path
    assert ns == 6 and [x for i, x in enumerate(res) if i != 3] == [x for i, x in enumerate(plain[1]) if i != 3]


def test_a_batch_that_fits_no_slice_is_left_to_the_single_path(emu, plain):
    ns, res = emu(8, 16)
    assert res[3][0] == 2                                     # the batch of nine: not this pass's
    assert [x for i, x in enumerate(res) if i != 3] == [x for i, x in enumerate(plain[1]) if i != 3]
