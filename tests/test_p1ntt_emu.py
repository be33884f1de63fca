"""The transforms over G1 executed on the CPU under the bounds tracker (tests/host_emu/p1ntt.cpp walks csrc/p1ntt.hpp's lane bodies in the host
call's order): every case of tests/golden/p1ntt.json byte for byte, forced slices, the twiddle-major lane order at every stage of every
small length, the twiddle table against Python integers, and the new Jacobian-base multiplication against the oracle's g1_mul."""
import ctypes
import os
import random
import subprocess

import pytest

import frntt_cases as fc
import p1ntt_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
R = pc.R
SZ = ctypes.c_size_t
U32, U64 = ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call([os.path.join(HERE, "host_emu", "build_p1ntt.sh")])
    L = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", "libp1ntt.so"))
    cp = ctypes.c_char_p
    L.emu_p1ntt.argtypes = [cp, SZ, SZ, U32, SZ, cp, ctypes.POINTER(SZ), ctypes.POINTER(SZ)]
    L.emu_p1ntt_mul.argtypes = [cp, cp, cp, cp]
    L.emu_p1ntt_twiddles.argtypes = [SZ, ctypes.c_int, cp]
    L.emu_p1ntt_twiddles.restype = None
    L.emu_p1ntt_lanes.argtypes = [U32, U32, U64]
    L.emu_p1ntt_lanes.restype = U64
    L.emu_p1ntt_pair.argtypes = [U32, U32, U64, U64, ctypes.POINTER(U64)]
    L.emu_p1ntt_pair.restype = None
    return L


def run(lib, images, n, flags, forced=0):
    k = len(images) // (n * 96)
    out = ctypes.create_string_buffer(len(images))
    slices, loads = SZ(), SZ()
    assert lib.emu_p1ntt(images, n, k, flags, forced, out, ctypes.byref(slices), ctypes.byref(loads)) == 0
    return out.raw, slices.value, loads.value


def test_fixture_holds_what_the_tests_speak_of():
    assert os.path.getsize(os.path.join(HERE, "golden", "p1ntt.json")) < 200 << 10
    fx = pc.fixture()
    assert int(fx["r"], 16) == R
    by = {c["name"]: c for c in fx["cases"]}
    for n in (1, 2, 4, 8, 16):
        c = by["n%d_k3" % n]
        assert (c["n"], c["k"]) == (n, 3) and sorted(c["out"]) == ["0", "1", "2", "3"]
    assert (by["n64_k1"]["n"], by["n64_k1"]["k"]) == (64, 1) and sorted(by["n64_k1"]["out"]) == ["0", "3"]
    for n in (4, 8):
        c = by["special_n%d" % n]
        v = pc.scalars(c)
        p = v[1][0]
        assert v[0] == [0] * n and v[1] == [p] * n and v[2] == [p] + [0] * (n - 1) and v[3] == [0] * (n - 1) + [p]
        assert v[4] == [p, R - p] * (n // 2) and v[5].count(0) == 2 and fc.ntt(v[6])[3] == 0 and all(v[6])
        rows = pc.rows(bytes.fromhex(c["out"]["0"]))
        assert rows[6 * n + 3] == bytes(96) and rows[n:2 * n].count(bytes(96)) == n - 1            # the hole; the constant vector's transform
    for c in fx["cases"]:                                                                         # zero scalars are the all-zero image
        for a, img in zip([a for v in pc.scalars(c) for a in v], pc.rows(bytes.fromhex(c["in"]))):
            assert (a == 0) == (img == bytes(96))


def test_every_case_of_the_fixture(lib):
    for name, n, k, flags, images, want in pc.cases():
        got, slices, loads = run(lib, images, n, flags)
        assert slices == 1 and loads == pc.twiddle_multiplications(n, k, flags), (name, flags)
        for i, (a, b) in enumerate(zip(pc.rows(got), pc.rows(want))):
            assert a == b, (name, flags, i)


def test_forced_slices_give_the_same_bytes(lib):
    for name, n, k, flags, images, want in pc.cases():
        if k >= 3 and n in (1, 4, 8):
            for forced in (1, 2):
                got, slices, _ = run(lib, images, n, flags, forced)
                assert got == want and slices == -(-k // forced), (name, flags, forced)


def test_round_trip_and_the_generator_image(lib):
    c = pc.case("n16_k3")
    images = bytes.fromhex(c["in"])
    for br in (0, pc.BITREV):
        assert run(lib, run(lib, images, 16, br)[0], 16, br | pc.INVERSE)[0] == images
    assert run(lib, pc.G_IMAGE, 1, 0)[0] == pc.G_IMAGE                                             # n = 1: the canonicalising copy of [1]G


def test_lane_order_is_twiddle_major_at_every_stage(lib):
    """for every length up to 2^7, every stage and vector counts around a wave: the lanes pair every element exactly once, a lane's twiddle is
    the one of its place, and the lanes come twiddle by twiddle - those with twiddle 1 first, Q = k 2^(m - 1 - b) of them"""
    out = (U64 * 3)()
    for m in range(1, 8):
        n = 1 << m
        for k in (1, 3, 64, 65):
            for b in range(m):
                lanes = lib.emu_p1ntt_lanes(m, b, k)
                assert lanes == k * n // 2
                q_count = k << (m - 1 - b)
                seen, tws = set(), []
                for lane in range(lanes):
                    lib.emu_p1ntt_pair(m, b, k, lane, out)
                    i0, i1, tw = out
                    assert i1 == i0 + (1 << b) and not i0 >> b & 1 and i1 < k * n
                    assert tw == (i0 & ((1 << b) - 1)) << (m - 1 - b) and tw < max(n // 2, 1)
                    assert i0 not in seen and i1 not in seen
                    seen |= {i0, i1}
                    tws.append(tw)
                assert len(seen) == k * n
                assert tws == sorted(tws) and tws.count(0) == q_count and all(tws.count(t) == q_count for t in set(tws))


def test_twiddle_table_is_plain_and_canonical(lib):
    for n in (2, 4, 32, 64, 1024):
        for inverse in (0, 1):
            out = ctypes.create_string_buffer(n // 2 * 32)
            lib.emu_p1ntt_twiddles(n, inverse, out)
            w = fc.omega(n)
            if inverse:
                w = pow(w, -1, R)
            assert fc.images(out.raw) == [pow(w, j, R) for j in range(n // 2)]


def test_jacobian_base_multiplication_against_the_oracle(lib):
    import bls12381_py as o
    rng = random.Random(20261020)
    a = int(pc.case("n2_k3")["scalars"][0][0], 16)
    base = bytes.fromhex(pc.case("n2_k3")["in"])[:96]
    pt = o.g1_from_blst_affine(base)
    assert pt == o.g1_mul(o.G1_GEN, a) and o.g1_to_blst_affine(o.G1_GEN) == pc.G_IMAGE
    chosen = [0, 1, 8, R - 1] + [16 ** j * 8 + 8 for j in (1, 15, 16, 62)] + [rng.randrange(R) for _ in range(4)] + [(1 << 256) - 1, int("8" * 64, 16)]
    got, ref = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    for s in chosen:
        assert lib.emu_p1ntt_mul(base, s.to_bytes(32, "little"), got, ref) == 1, hex(s)
        q = o.g1_mul(pt, s)
        assert got.raw == (bytes(96) if q is None else o.g1_to_blst_affine(q)), hex(s)
    assert lib.emu_p1ntt_mul(bytes(96), (5).to_bytes(32, "little"), got, ref) == 1 and got.raw == bytes(96)      # the infinity base
