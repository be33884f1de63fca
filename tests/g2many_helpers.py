"""Helpers of the tests of the G2 many-MSM call and the Jacobian-to-affine calls: the host libraries of tests/host_emu/build_msmmany_g2.sh behind
Python functions, the oracle's G2 MSM, and the inputs several of those tests share."""
import ctypes
import os
import random
import subprocess

import bls12381_py as o
from util import g1_inf_image, g1_jac_image, g2_inf_image, g2_jac_image

HERE = os.path.dirname(os.path.abspath(__file__))
CONSTANTS = ("VWIN_MAX", "BUCKETS_MAX", "PAIRS_MAX", "MSM_WINDOWS_MAX", "G2_BUCKETS_MAX", "G2_TAIL_WAVES", "G1_WORDS", "G2_WORDS", "MSM_SEG", "WAVE", "HEAD", "ROW")
WIN = ("nwin", "wbase", "wrem", "nbits", "cbk") + tuple("H%d" % j for j in range(9))
BUFFERS = ("pts_int", "offs_dev", "hist", "chist", "sorted", "buckets", "segout", "part")
HEAD = WIN + ("shared", "n_ref", "buckets_per_msm", "segs_per_win", "nsplit", "tail_waves", "tail_lanes", "msms_max") + tuple("size_" + b for b in BUFFERS)
ROW = ("single", "j0", "j1", "pair0", "pairs", "points", "nv", "total", "nseg", "pair_grid", "order_grid", "bucket_grid", "team", "segred_grid") + BUFFERS
_libs = {}


def _build(what, name):
    if name not in _libs:
        subprocess.check_call([os.path.join(HERE, "host_emu", "build_msmmany_g2.sh"), what])
        _libs[name] = ctypes.CDLL(os.path.join(HERE, "host_emu", "_build", name))
    return _libs[name]


def plan_lib():
    L = _build("plan", "libplan_msmmany_g2.so")
    u64p, szp, sz = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t
    L.plan_manymsm_g2_constants.argtypes = [u64p]
    L.plan_manymsm_g2_call.argtypes = [szp, sz, sz, sz, ctypes.c_int, u64p, u64p, sz]
    L.plan_manymsm_g2_call.restype = sz
    L.plan_to_affine_call.argtypes = [sz, ctypes.c_uint32, u64p, sz]
    L.plan_to_affine_call.restype = sz
    L.plan_to_affine_constants.argtypes = [u64p]
    return L


def constants():
    c = (ctypes.c_uint64 * 12)()
    plan_lib().plan_manymsm_g2_constants(c)
    C = dict(zip(CONSTANTS, c))
    assert C["HEAD"] == len(HEAD) and C["ROW"] == len(ROW)
    return C


def offsets_of(lengths):
    acc = [0]
    for v in lengths:
        acc.append(acc[-1] + v)
    return acc


def call_plan(k, nbits, n=None, lengths=None, g2=True):
    """-> (head, passes) of a shared call (n points, k MSMs) or a ragged one (lengths), with the plan's G2 flag on or off"""
    if lengths is None:
        offs, npoints = None, n
    else:
        acc = offsets_of(lengths)
        offs, npoints, k = (ctypes.c_size_t * len(acc))(*acc), acc[-1], len(lengths)
    head = (ctypes.c_uint64 * len(HEAD))()
    cap = k + 1
    rows = (ctypes.c_uint64 * (cap * len(ROW)))()
    count = plan_lib().plan_manymsm_g2_call(offs, npoints, k, nbits, int(g2), head, rows, cap)
    assert count <= cap
    return dict(zip(HEAD, head)), [dict(zip(ROW, rows[i * len(ROW):(i + 1) * len(ROW)])) for i in range(count)]


def to_affine_plan(n, force_run=0):
    """-> (run, chunk, [(first, n, lanes, grid), ...])"""
    cap = n // (1 << 20) + 2
    out = (ctypes.c_uint64 * (2 + 4 * cap))()
    count = plan_lib().plan_to_affine_call(n, force_run, out, cap)
    assert count <= cap
    return out[0], out[1], [tuple(out[2 + 4 * i:6 + 4 * i]) for i in range(count)]


def to_affine_constants():
    c = (ctypes.c_uint64 * 3)()
    plan_lib().plan_to_affine_constants(c)
    return dict(zip(("DEVICE_LANES", "RUN_MAX", "CHUNK_POINTS"), c))


def tail_lib():
    L = _build("msmmany_g2", "libmsmmany_g2.so")
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.emu_g2_many_windows.argtypes = [ctypes.c_size_t, ctypes.c_size_t, u32p, u32p]
    L.emu_g2_many_windows.restype = ctypes.c_uint32
    L.emu_g2_many_digits.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
    L.emu_g2_many_digits.restype = ctypes.c_uint32
    L.emu_g2_tail_walk.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p, u32p]
    L.emu_g2_tail_walk.restype = None
    return L


def toaffine_lib():
    L = _build("toaffine", "libtoaffine.so")
    for fn in (L.emu_to_affine_g1, L.emu_to_affine_g2):
        fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p]
        fn.restype = ctypes.c_int
    return L


def windows(n_ref, nbits):
    """-> (nwin, [bit offset of window w for w in 0 .. nwin])"""
    win, offs = (ctypes.c_uint32 * 14)(), (ctypes.c_uint32 * 65)()
    nwin = tail_lib().emu_g2_many_windows(n_ref, nbits, win, offs)
    return nwin, list(offs[:nwin + 1])


def digits(scalar, n_ref, nbits):
    d = (ctypes.c_int32 * 64)()
    nwin = tail_lib().emu_g2_many_digits(scalar.to_bytes(32, "little"), n_ref, nbits, d)
    return list(d[:nwin])


def msm_g2(points, scalars, nbits=255):
    """the oracle's G2 MSM: sum [k mod 2^nbits] P over affine points (None = infinity)"""
    acc = None
    for p, k in zip(points, scalars):
        k &= (1 << nbits) - 1
        if p is not None and k:
            acc = o.g2_add(acc, o.g2_mul(p, k))
    return acc


def g2_affine_bytes(p):
    return o.g2_to_blst_affine(p) if p is not None else bytes(192)


def g1_affine_bytes(p):
    return o.g1_to_blst_affine(p) if p is not None else bytes(96)


# ---- inputs of the to_affine tests (CPU emulation and GPU): points with a chosen Z, infinities at chosen places --------------------------------
def to_affine_case(g2, n, inf_at=(), seed=0, unit_z_at=()):
    """-> (n Jacobian images, the n affine images expected).  Point i is (x lam^2, y lam^3, lam) of an oracle point for a random lam, Z == 1 at
    unit_z_at, and an infinity (Z == 0 under non-zero X, Y on the odd places, the all-zero image on the even ones) at inf_at."""
    rng = random.Random(1000 * n + seed + (500000 if g2 else 0))
    gen, mul = (o.G2_GEN, o.g2_mul) if g2 else (o.G1_GEN, o.g1_mul)
    base = [mul(gen, rng.randrange(1, o.R)) for _ in range(min(n, 12))]
    ins, want = [], []
    for i in range(n):
        p = base[i % len(base)]                                # a dozen points under ever new Z: the images differ, the oracle stays cheap
        if i in inf_at:
            if g2:
                ins.append(g2_inf_image((rng.randrange(1, o.P), 5), (7, rng.randrange(1, o.P))) if i & 1 else bytes(288))
            else:
                ins.append(g1_inf_image(rng.randrange(1, o.P), rng.randrange(1, o.P)) if i & 1 else bytes(144))
            want.append(bytes(192 if g2 else 96))
            continue
        if g2:
            lam = (1, 0) if i in unit_z_at else (rng.randrange(o.P), rng.randrange(1, o.P))
            ins.append(g2_jac_image(p, lam))
            want.append(o.g2_to_blst_affine(p))
        else:
            lam = 1 if i in unit_z_at else rng.randrange(1, o.P)
            ins.append(g1_jac_image(p, lam))
            want.append(o.g1_to_blst_affine(p))
    return b"".join(ins), b"".join(want)


def infinity_placements(n, run):
    """the placements both to_affine tests use, for n points cut into runs of `run`: none; the first, a middle and the last place of a run; a
    whole run of infinities (with finite runs around it when n allows); every point"""
    r0 = run * (1 if n >= 3 * run else 0)                      # the run the placements go into: the second when there are three
    last = min(r0 + run, n) - 1
    out = [(), (r0,), (last,), tuple(range(r0, last + 1)), tuple(range(n))]
    if last - r0 >= 2:
        out.append(((r0 + last) // 2,))
        out.append((r0, (r0 + last) // 2, last))
    return out
