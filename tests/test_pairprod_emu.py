"""The pair-slot bodies of the pairing-product calls (csrc/pairprod.hpp) executed on the CPU under the bounds tracker
(tests/host_emu/pairprod.cpp) against oracle/bls12381_py.py: the status codes for a P off the curve, a P on the curve outside G1 and likewise for
Q (the torsion points of tests/golden/deser_adversarial.json), infinity in either slot, what a failing pair leaves in the pair store, and the
expansion of the group scalars to the pair slots across group boundaries, empty groups and parts."""
import ctypes
import os
import subprocess

import pytest

import bls12381_py as o
import pairprod_cases as pc
from util import g1_jac_to_affine, g2_jac_to_affine

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_pairprod.sh"), "emu"])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libpairprod.so"))
    sz, cp = ctypes.c_size_t, ctypes.c_char_p
    L.emu_pairprod_setup.argtypes = [cp, cp, sz, ctypes.c_uint32, cp, cp, cp, cp]
    L.emu_pairprod_expand.argtypes = [ctypes.POINTER(sz), sz, sz, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    return L


def setup(emu, pairs, validate):
    n = len(pairs)
    st, p, q, key = (ctypes.create_string_buffer(n * w) for w in (1, 144, 288, 96))
    emu.emu_pairprod_setup(b"".join(a for a, _ in pairs), b"".join(b for _, b in pairs), n, validate, st, p, q, key)
    return (list(st.raw), [p.raw[144 * i:144 * i + 144] for i in range(n)], [q.raw[288 * i:288 * i + 288] for i in range(n)],
            [key.raw[96 * i:96 * i + 96] for i in range(n)])


def is_inf1(b):
    return b[96:144] == bytes(48)


def is_inf2(b):
    return b[192:288] == bytes(96)


def test_status_codes_and_operands(emu):
    adv = pc.adversarial()
    P, Q = pc.g1(5), pc.g2(9)
    p, q = pc.p1b(P), pc.q2b(Q)
    pairs, want = [(p, q), (pc.INF1, q), (p, pc.INF2), (pc.INF1, pc.INF2)], [0, 0, 0, 0]
    for name, (img, st) in sorted(adv.items()):
        pairs.append((img, q) if len(img) == 96 else (p, img))
        want.append(st)
    off1, off2 = adv["g1_off_curve"][0], adv["g2_off_curve"][0]
    tor1, tor2 = adv["g1_ord3_0_pos"][0], adv["g2_ord13_0_pos"][0]
    pairs += [(off1, off2), (tor1, off2), (tor1, tor2), (pc.INF1, tor2), (off1, pc.INF2)]      # P is checked first; infinity passes
    want += [pc.P_OFF_CURVE, pc.P_NOT_IN_G1, pc.P_NOT_IN_G1, pc.Q_NOT_IN_G2, pc.P_OFF_CURVE]
    st, ps, qs, keys = setup(emu, pairs, pc.VALIDATE)
    assert st == want and set(want) == {0, 1, 2, 3, 4}
    for i, ((a, b), s) in enumerate(zip(pairs, st)):
        if s:                                                              # a failing pair: both operands infinite, a zero key for k_pkmul
            assert is_inf1(ps[i]) and is_inf2(qs[i]) and keys[i] == bytes(96), i
            continue
        assert keys[i] == a
        assert is_inf1(ps[i]) == (a == pc.INF1) and is_inf2(qs[i]) == (b == pc.INF2), i
        if a != pc.INF1:
            assert g1_jac_to_affine(ps[i]) == o.g1_from_blst_affine(a)
        if b != pc.INF2:
            assert g2_jac_to_affine(qs[i]) == o.g2_from_blst_affine(b)
    # without validation nothing is judged: every pair goes on as it is
    st0, ps0, qs0, keys0 = setup(emu, pairs, 0)
    assert st0 == [0] * len(pairs) and keys0 == [a for a, _ in pairs]
    assert [is_inf1(x) for x in ps0] == [a == pc.INF1 for a, _ in pairs] and [is_inf2(x) for x in qs0] == [b == pc.INF2 for _, b in pairs]


def test_status_agrees_with_the_oracle_on_valid_points(emu):
    pairs = [(pc.p1b(pc.g1(a)), pc.q2b(pc.g2(b))) for a, b in ((1, 1), (2, 3), (o.R - 1, o.R - 1), (12345, 67890))]
    for a, b in pairs:
        assert o.g1_in_subgroup(o.g1_from_blst_affine(a)) and o.g2_in_subgroup(o.g2_from_blst_affine(b))
    assert setup(emu, pairs, pc.VALIDATE)[0] == [0] * 4


def test_scalar_expansion_across_groups_and_parts(emu):
    sz, u64 = ctypes.c_size_t, ctypes.c_uint64
    for lengths in ([3], [0, 2, 0, 0, 5, 1, 0], [1] * 9, [7, 0, 8, 9, 0, 0, 1], [0, 0]):
        offs = [0]
        for n in lengths:
            offs.append(offs[-1] + n)
        k, n = len(lengths), offs[-1]
        r = [0x9e3779b97f4a7c15 * (g + 1) % (1 << 64) for g in range(k)]
        want = [r[g] for g, m in enumerate(lengths) for _ in range(m)]
        for cap in (1, 2, 3, 8, 64):
            out = (u64 * max(n, 1))()
            parts = emu.emu_pairprod_expand((sz * (k + 1))(*offs), k, cap, (u64 * k)(*r), out)
            assert parts == (n + cap - 1) // cap and list(out[:n]) == want, (lengths, cap)
