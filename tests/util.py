"""Shared helpers for tests: fixture loading and canonicalisation of projective outputs."""
import ctypes
import hashlib
import itertools
import json
import os
import random
import subprocess

import bls12381_py as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def buf(n):
    return ctypes.create_string_buffer(n)


def fp_int(b):
    return o.fp_from_mont_bytes(bytes(b))


def fp2_int(b):
    return (fp_int(b[:48]), fp_int(b[48:96]))


def g1_jac_to_affine(b):
    """144-byte Jacobian (Montgomery) -> oracle affine point."""
    x, y, z = fp_int(b[:48]), fp_int(b[48:96]), fp_int(b[96:144])
    if z == 0:
        return None
    zi = o.fp_inv(z)
    return (x * zi * zi % o.P, y * zi * zi * zi % o.P)


def g2_jac_to_affine(b):
    x, y, z = fp2_int(b[:96]), fp2_int(b[96:192]), fp2_int(b[192:288])
    if z == (0, 0):
        return None
    zi = o.f2inv(z)
    zi2 = o.f2sqr(zi)
    return (o.f2mul(x, zi2), o.f2mul(y, o.f2mul(zi2, zi)))


def g1_aff_to_jac_bytes(p):
    if p is None:
        return bytes(144)
    return o.g1_to_blst_affine(p) + o.fp_to_mont_bytes(1)


def g2_aff_to_jac_bytes(p):
    if p is None:
        return bytes(288)
    return o.g2_to_blst_affine(p) + o.fp_to_mont_bytes(1) + bytes(48)


# ---- Jacobian images with a chosen Z.  (lam^2 x, lam^3 y, lam) is the point (x, y) for every lam != 0; two images of one point (or of a point and
# its negative) with different lam are what two partial sums of a reduction look like when they meet, and the only inputs for which the
# complete addition's H = U2 - U1 is a non-zero multiple of p in the device's redundant limbs instead of literally zero.
_FP_ALL_HIGH = ((o.P >> 364) - 1 << 364) | ((1 << 364) - 1)          # below p; every 28-bit limb under the top one is 0xfffffff
_lam_rng = random.Random(20261017)
LAMBDAS_FP = (1, o.P - 1, 2, (o.P + 1) // 2, _FP_ALL_HIGH, _lam_rng.randrange(1, o.P), _lam_rng.randrange(1, o.P))
LAMBDAS_FP2 = tuple((a, 0) for a in LAMBDAS_FP[:4]) + ((_FP_ALL_HIGH, _FP_ALL_HIGH),) + tuple(
    (_lam_rng.randrange(1, o.P), _lam_rng.randrange(1, o.P)) for _ in range(2)) + ((0, 1), (o.P - 1, o.P - 1))
assert _FP_ALL_HIGH < o.P and len(set(LAMBDAS_FP)) == 7 and len(set(LAMBDAS_FP2)) == 9


def fp2_to_mont_bytes(a):
    return o.fp_to_mont_bytes(a[0]) + o.fp_to_mont_bytes(a[1])


def g1_jac_image(p, lam):
    """blst_p1 image (Montgomery, R = 2^384, like g1_aff_to_jac_bytes) of (lam^2 x, lam^3 y, lam), lam in Fp*; None -> the all-zero image"""
    if p is None:
        return bytes(144)
    lam %= o.P
    assert lam
    l2 = lam * lam % o.P
    return o.fp_to_mont_bytes(p[0] * l2 % o.P) + o.fp_to_mont_bytes(p[1] * l2 * lam % o.P) + o.fp_to_mont_bytes(lam)


def g2_jac_image(q, lam):
    """blst_p2 image of (lam^2 x, lam^3 y, lam), lam in Fp2*; None -> the all-zero image"""
    if q is None:
        return bytes(288)
    assert lam != (0, 0)
    l2 = o.f2sqr(lam)
    return fp2_to_mont_bytes(o.f2mul(q[0], l2)) + fp2_to_mont_bytes(o.f2mul(q[1], o.f2mul(l2, lam))) + fp2_to_mont_bytes(lam)


def g1_inf_image(x, y):
    """the point at infinity the way a formula may leave it: Z = 0 under arbitrary X, Y (blst_p1_is_inf looks at Z alone)"""
    return o.fp_to_mont_bytes(x % o.P) + o.fp_to_mont_bytes(y % o.P) + bytes(48)


def g2_inf_image(x, y):
    return fp2_to_mont_bytes(x) + fp2_to_mont_bytes(y) + bytes(96)


def fp12_from_bytes(b):
    """576-byte blst_fp12 image -> oracle flat tuple."""
    t = [fp2_int(b[96 * i:96 * i + 96]) for i in range(6)]
    return (t[0], t[3], t[1], t[4], t[2], t[5])


def fp12_hexlist_to_flat(h):
    t = [(fp_int(bytes.fromhex(c[0])), fp_int(bytes.fromhex(c[1]))) for c in h]
    return (t[0], t[3], t[1], t[4], t[2], t[5])


def fp12_to_bytes(a):
    t = o.f12_to_tower_ints(a)
    return b"".join(o.fp_to_mont_bytes(c[0]) + o.fp_to_mont_bytes(c[1]) for c in t)


# ---- the host layer's launch plans.  csrc/plan.hpp decides which kernel, grid and stream every stage of a call takes; it is plain C++, and
# tests/host_emu/plan.cpp compiles it for the host.  The tests that must sit on the plan's boundaries ask that library, i.e. the product's own
# code, where they are: nothing below restates a rule.  S = the context's wave slots (4 x CU count).
_PLAN = None
_PLAN_CONSTANTS = ("WAVE", "N_LINES", "SIG_SLOTS_MAX", "SIG_WIDE_MIN", "FORK_ITEMS_PER_SLOT", "TEAM_CLEAR_ITEMS_PER_SLOT", "TEAM_LINES_ITEMS_PER_SLOT")
TEAM_FORMS = ("rows", "rows2", "spread", "wide")
_STAGE = ("team", "form", "grid")
_LINES = ("main_pairs",) + tuple("main_" + f for f in _STAGE) + ("extra_pairs",) + tuple("extra_" + f for f in _STAGE)
_SLICE = (("nb", "hash_map", "hash_map_grid") + tuple("clear_" + f for f in _STAGE) + ("pkmul_spread", "side", "pk_stream", "sig_stream", "cw", "nwin",
          "total", "lshift", "bucket_grid", "extra_apart") + tuple("extra_lines_" + f for f in _STAGE) + tuple("lines_" + f for f in _LINES))
_LINEPROD = ("nblk", "m", "per_lane", "live", "per", "nb1")
_MSM_CONSTANTS = ("MSM_SEG", "MSM_ORD_PER", "PIP_SLICES", "PIP_SORT_THREADS", "PIP_SORT_MAX_CBK", "MSM_TEAM_LANES_MAX", "MSM_TAIL_WAVES_MAX", "MSM_WINDOWS_MAX",
                  "MSM_NSPLIT_MAX", "MSM_GROUPS_MAX", "SUM_PARTS_BYTES", "G1_WORDS", "G2_WORDS", "F12_WORDS")
_MSM_GROUP = ("w0", "w1", "g0", "gc", "t0", "tc", "order_grid", "bucket_grid", "team", "segred_grid", "tail_waves", "tail_lanes")
MSM_BUFFERS = ("d_pts", "d_sc", "pts_int", "hist", "chist", "shist", "part", "sorted", "buckets", "segout", "winout", "out")
_MSM = (("nwin", "wbase", "wrem", "nbits", "cbk") + tuple("H%d" % j for j in range(9)) + ("n", "total", "segs_per_win", "nseg", "nsplit", "lds_sort", "per",
        "point_grid", "slice_scan_grid", "ngroups", "cut0", "cut1", "cut2") + tuple("g%d_%s" % (g, f) for g in range(2) for f in _MSM_GROUP) +
        tuple("touch_" + b for b in MSM_BUFFERS) + tuple("size_" + b for b in MSM_BUFFERS))
_CTX = ("stride", "mstride", "nblk_cap", "lpart_words", "lpart_mid_words", "export_bytes")


def plan_lib():
    """csrc/plan.hpp as a ctypes library (built on first use, well under a second)"""
    global _PLAN
    if _PLAN is None:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emu")
        subprocess.check_call([os.path.join(here, "build_plan.sh")])
        L = ctypes.CDLL(os.path.join(here, "_build", "libplan.so"))
        u32, sz, i, out, u64p = ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        for name, res, args in (("plan_constants", None, (out,)), ("plan_team_rows_max", u32, (u32,)), ("plan_team_lines_max", u32, (u32,)),
                                ("plan_team_form", u32, (u32, u32)), ("plan_lines", None, (u32, i, u32, u32, out)),
                                ("plan_slice", None, (u32, i, i, sz, out)), ("plan_lineprod", None, (u32, u32, u32, u32, i, out)),
                                ("plan_aggv_cut", sz, (out, sz, sz, sz)), ("plan_aggv_all32", i, (out, sz)), ("plan_shard_nslices", sz, (sz, sz)),
                                ("plan_shard_workspaces", i, (sz,)), ("plan_shard_slice_count", sz, (sz, sz, sz, u32)),
                                ("plan_shard_workspace_of", i, (sz, u32, i)), ("plan_chunk_of_tuple", u32, (sz, u32, sz)),
                                ("plan_msm_constants", None, (u64p,)), ("plan_msm_row", sz, ()), ("plan_msm_many", None, (u64p, sz, sz, i, i, i, u64p)),
                                ("plan_sum_many", None, (i, u32, out, sz, out)), ("plan_ctx", None, (u32, sz, u64p)),
                                ("plan_lineprod_many", None, (u32, u32, u32, u32, sz, i, out))):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        _PLAN = L
    return _PLAN


def _plan_call(fn, fields, *args):
    """fn(*args, out) -> {field: word}"""
    out = (ctypes.c_uint32 * len(fields))()
    getattr(plan_lib(), fn)(*args, out)
    return dict(zip(fields, out))


def __getattr__(name):
    """the plan's constants (TEAM_CLEAR_ITEMS_PER_SLOT, SIG_WIDE_MIN, ...), read from the compiled plan"""
    if name in _PLAN_CONSTANTS:
        return _plan_call("plan_constants", _PLAN_CONSTANTS)[name]
    if name in _MSM_CONSTANTS:
        out = (ctypes.c_uint64 * len(_MSM_CONSTANTS))()
        plan_lib().plan_msm_constants(out)
        return dict(zip(_MSM_CONSTANTS, out))[name]
    raise AttributeError(name)


def slice_plan(n, S, coop=True, have_side=True):
    """plan.hpp slice_for: everything run_pairs follows for a slice of n sets"""
    return _plan_call("plan_slice", _SLICE, S, int(coop), int(have_side), n)


def lines_plan(npairs, extra, S, coop=True):
    """plan.hpp lines_for"""
    return _plan_call("plan_lines", _LINES, S, int(coop), npairs, extra)


def lineprod_plan(S, nblk_cap, stride, npairs, fold):
    """plan.hpp lineprod_for"""
    return _plan_call("plan_lineprod", _LINEPROD, S, nblk_cap, stride, npairs, int(fold))


def msm_plans(npoints, nbits, g2=False, allow_split=True, have_side=True):
    """plan.hpp msm_for for every entry of `npoints` at once -> {field: numpy uint64 array}: the plan (g0_* / g1_*: its window groups), touch_<buffer>
    = msm_extents of it, size_<buffer> = msm_sizes_for what msm_reserve grows an empty workspace to for that call (MSM_BUFFERS names the buffers)"""
    import numpy as np
    L = plan_lib()
    assert L.plan_msm_row() == len(_MSM)
    pts = np.ascontiguousarray(npoints, dtype=np.uint64)
    rows = np.empty((len(pts), len(_MSM)), dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.plan_msm_many(pts.ctypes.data_as(u64p), len(pts), nbits, int(g2), int(allow_split), int(have_side), rows.ctypes.data_as(u64p))
    return {f: rows[:, j] for j, f in enumerate(_MSM)}


def msm_plan(n, nbits, g2=False, allow_split=True, have_side=True):
    """one plan -> {field: int}"""
    return {f: int(v[0]) for f, v in msm_plans([n], nbits, g2, allow_split, have_side).items()}


MSM_FORMS = ("lds_sort", "g0_team", "ngroups", "nsplit")      # what msm_enqueue launches differently from one size to the next


def msm_hand_overs(nbits, below, g2=False):
    """[(form, t)]: the plan of a call with fork streams changes `form` (of MSM_FORMS) between t and t + 1 points, for every t + 1 < below"""
    import numpy as np
    out = []
    step = 1 << 14
    for lo in range(1, below, step):                 # chunks that overlap by one size
        p = msm_plans(np.arange(lo, min(lo + step + 1, below)), nbits, g2)
        out += [(f, lo + int(j)) for f in MSM_FORMS for j in np.nonzero(p[f][1:] != p[f][:-1])[0]]
    return sorted(out, key=lambda x: (x[1], x[0]))


def sum_plans(g2, S, n):
    """plan.hpp g1_sum_for / g2_sum_for for every entry of n -> (nblk, m) as numpy arrays"""
    import numpy as np
    u32p = ctypes.POINTER(ctypes.c_uint32)
    n = np.ascontiguousarray(n, dtype=np.uint32)
    rows = np.empty((len(n), 2), dtype=np.uint32)
    plan_lib().plan_sum_many(int(g2), S, n.ctypes.data_as(u32p), len(n), rows.ctypes.data_as(u32p))
    return rows[:, 0].astype(np.uint64), rows[:, 1].astype(np.uint64)


def lineprod_plans(S, nblk_cap, stride, first, count, fold):
    """plan.hpp lineprod_for for npairs = first .. first + count - 1 -> {field: numpy array}"""
    import numpy as np
    rows = np.empty((count, len(_LINEPROD)), dtype=np.uint32)
    plan_lib().plan_lineprod_many(S, nblk_cap, stride, first, count, int(fold), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return {f: rows[:, j].astype(np.uint64) for j, f in enumerate(_LINEPROD)}


def ctx_sizes(S, max_sets):
    """plan.hpp ctx_for"""
    out = (ctypes.c_uint64 * len(_CTX))()
    plan_lib().plan_ctx(S, max_sets, out)
    return dict(zip(_CTX, out))


def rows_max(S):
    """the row executor's bound"""
    return plan_lib().plan_team_rows_max(S)


def team_form(count, S):
    """which form of an engine kernel (clearing or Miller lines) takes `count` items"""
    return TEAM_FORMS[plan_lib().plan_team_form(S, count)]


def _stage_name(p, stage):
    return "team_" + TEAM_FORMS[p[stage + "_form"]] if p[stage + "_team"] else "one_lane"


def latency_plan(n, S):
    """The executors a latency-mode (cooperative) context with side streams picks for a blocking call of n sets (`lines`: of the tuple pairs)."""
    p = slice_plan(n, S)
    return {"hash_map": ("rows", "spread", "plain")[p["hash_map"]], "clear": _stage_name(p, "clear"), "side": ("none", "fork", "fork_sig")[p["side"]],
            "lines": _stage_name(p, "lines_main"), "extra_pairs": p["total"]}


def latency_hand_overs(S):
    """(stage, t): the plan changes `stage`'s executor between t and t + 1 sets - the hand-overs of the 4 S .. 32 S range, stage by stage."""
    plans = [latency_plan(n, S) for n in range(4 * S, 32 * S + 2)]
    return [(stage, 4 * S + i) for stage in ("clear", "side", "lines", "hash_map") for i in range(len(plans) - 1) if plans[i][stage] != plans[i + 1][stage]]


def apply_defect(rec, d):
    """A defect of tests/golden/latency_handover.json (the kinds of tests/gpu_soak.py) applied to the 320-byte records `rec` (bytearray, in place)."""
    i = d["indices"][0]
    if d["kind"] == "swap":                                   # two signatures swapped
        j = d["indices"][1]
        rec[320 * i + 128:320 * i + 320], rec[320 * j + 128:320 * j + 320] = rec[320 * j + 128:320 * j + 320], rec[320 * i + 128:320 * i + 320]
    elif d["kind"] == "msg":                                  # one message bit flipped
        rec[320 * i + 96 + d["byte"]] ^= 1 << d["bit"]
    elif d["kind"] == "infpk":                                # public key at infinity
        rec[320 * i:320 * i + 96] = bytes(96)
    elif d["kind"] == "infsig":                               # signature at infinity
        rec[320 * i + 128:320 * i + 320] = bytes(192)
    else:
        raise ValueError(d["kind"])


# ---- variable-length aggregateVerify inputs: tests/golden/gen_aggv_varlen.py (fixture) and tests/test_gpu_aggv_varlen.py (device) build the
# same keys and messages from this rule.  Every byte is SHA-256 in counter mode over a fixed label (no `random`: the two sides cannot drift).
VARLEN_LABEL = b"nim-blscurve_amd/aggv_varlen/v1"
VARLEN_CASES = ("one", "wave", "mixed", "wide", "long")
VARLEN_PREFIXES = {"one": (1,), "wave": (63, 64, 65), "mixed": (1000,), "wide": (4097,), "long": (40,)}      # the sizes a case is verified at
VARLEN_RUN32 = (301, 581)           # `mixed`: messages [301, 581) are all 32 bytes long, between two far ones
VARLEN_LONG = 20000                 # `long`: eight messages of this length
# with the scheme's 43-byte DST, Z_pad | msg | 0x0100 | 0x00 | DST | len is len(msg) + 111 bytes: the 0x80 byte and the 8-byte bit count
# fall at the end of one block / into the next one at len(msg) mod 64 in {8, 9, 16, 17}
VARLEN_PAD_EDGES = [b + d for d in (0, 64, 128) for b in (8, 9, 16, 17)]
VARLEN_REQUIRED = [0, 1, 31, 32, 33] + VARLEN_PAD_EDGES + [1000, 4095, 4096, 4097]
VARLEN_SHORT_MAX, VARLEN_FAR_MIN = 191, 320      # a "short" length is <= 191, a "far" one >= 320: neighbours of different kinds differ by > 2 SHA blocks


def ctr_bytes(tag, n):
    """n bytes: SHA256(label | tag | LE64(0)) | SHA256(label | tag | LE64(1)) | ..."""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += hashlib.sha256(VARLEN_LABEL + b"|" + tag + b"|" + i.to_bytes(8, "little")).digest()
        i += 1
    return bytes(out[:n])


def _alternate(far, short, n):
    """far, short, far, short, ... (n lengths; both lists are consumed in order)"""
    out = []
    for i in range(n):
        out.append(far.pop(0) if i % 2 == 0 else short.pop(0))
    assert not far and not short, (len(far), len(short))
    return out


def _fill(kind, count, first):
    """`count` lengths of one kind walking the residues from `first`: short = r, r + 64, r + 128 in turn; far = r + 64 k, k = 5 .. 15 in turn"""
    out = []
    for j in range(count):
        r = (first + j) % 64
        out.append(r + 64 * (j % 3) if kind == "short" else r + 64 * (5 + j % 11))
    return out


def varlen_lengths(name):
    """The message lengths of a case.  Lanes alternate between far (>= 320) and short (<= 191) lengths, so adjacent lanes of a wave differ by
    more than a SHA block (outside `mixed`'s run of 32-byte messages).

    `mixed` and `wide` hold every length of VARLEN_REQUIRED and every residue mod 64.  `wave` cannot: its 64-message prefix has room for each
    residue once, and 8 / 72 / 136 (or 0 / 4096) share one.  It takes each residue exactly once in its first 64 messages - the padding edges
    8, 9, 16, 17 themselves, 0, 1, 31, 32, 33, 1000 and 4095 - and 4096 as the lone lane of its second block."""
    if name == "one":
        return [17]
    if name == "wave":
        short_req, far_req = [0, 1, 31, 32, 33, 8, 9, 16, 17], [1000, 4095]
        taken = {x % 64 for x in short_req + far_req}
        rest = [r for r in range(64) if r not in taken]                  # 53 residues: 23 short, 30 far
        short = [r + 64 * (j % 3) for j, r in enumerate(rest[:23])]
        far = [r + 64 * (5 + j % 11) for j, r in enumerate(rest[23:])]
        short = short[:3] + short_req + short[3:]                        # the zero-length message away from lane 63
        L = _alternate(far_req + far, short, 64) + [4096]
    elif name in ("mixed", "wide"):
        n = VARLEN_PREFIXES[name][0]
        short_req = [x for x in VARLEN_REQUIRED if x <= VARLEN_SHORT_MAX]
        far_req = [x for x in VARLEN_REQUIRED if x >= VARLEN_FAR_MIN]
        if name == "mixed":
            a, b = VARLEN_RUN32
            head = _alternate(far_req + _fill("far", (a + 1) // 2 - len(far_req), 0),
                              _fill("short", 3, 40) + short_req + _fill("short", a // 2 - 3 - len(short_req), 2), a)
            m = n - b
            tail = _alternate(_fill("far", (m + 1) // 2, 11), _fill("short", m // 2, 23), m)
            L = head + [32] * (b - a) + tail
        else:
            nf, ns = (n + 1) // 2, n // 2
            L = _alternate(far_req + _fill("far", nf - len(far_req), 0), _fill("short", 3, 40) + short_req + _fill("short", ns - 3 - len(short_req), 2), n)
    elif name == "long":
        # eight messages of 20 000 bytes between short ones, and the three around the one-message limit
        short = _fill("short", 20, 5)
        far = [VARLEN_LONG, 4096, VARLEN_LONG, 1000, VARLEN_LONG, VARLEN_LONG, 4095] + [VARLEN_LONG, 4097, 333] + [VARLEN_LONG] * 3 + _fill("far", 7, 50)
        L = _alternate(far, short, 40)
        assert L.count(VARLEN_LONG) == 8
    else:
        raise ValueError(name)
    n = len(L)
    assert n == max(VARLEN_PREFIXES[name])
    run = range(*VARLEN_RUN32) if name == "mixed" else range(0)
    for i in range(n - 1):                                              # adjacent lanes: more than one SHA block apart
        if i // 64 == (i + 1) // 64 and not (i in run and i + 1 in run):
            assert abs(L[i] - L[i + 1]) > 64, (name, i, L[i], L[i + 1])
    if n >= 64:
        assert {x % 64 for x in L[:64]} == set(range(64)) or name != "wave"
        assert {x % 64 for x in L} == set(range(64)), name
        need = VARLEN_REQUIRED if name != "wave" else [0, 1, 31, 32, 33, 8, 9, 16, 17, 1000, 4095, 4096]
        assert all(x in L for x in need), (name, [x for x in need if x not in L])
        assert any(x != 32 for x in L) and 32 in L
    if name == "mixed":
        assert all(L[i] == 32 for i in run) and len(run) >= 256 and all(L[i] != 32 or i in run or L.count(32) > len(run) for i in range(n))
    return L


def varlen_case(name):
    """-> (sks, msgs): secret keys (ints below the group order, as bench.secret_key masks them) and messages of varlen_lengths(name)."""
    L = varlen_lengths(name)
    tag = name.encode()
    sks = []
    for i in range(len(L)):
        sk = bytearray(ctr_bytes(b"sk|" + tag + b"|%d" % i, 32))
        sk[31] &= 0x3f
        sk[0] |= 1
        sks.append(int.from_bytes(sk, "little"))
    msgs = [ctr_bytes(b"msg|" + tag + b"|%d" % i, n) for i, n in enumerate(L)]
    return sks, msgs


# ---- aggregateVerify's greedy cut (plan.hpp aggv_cut, aggv_all32): a slice takes pairs while it holds fewer than `cap` of them and the staged
# bytes stay within the context's buffer; a slice whose messages are all 32 bytes long takes the batch path's hashing kernels, any other k_hash_var.
def _offsets(lengths):
    return (ctypes.c_uint32 * (len(lengths) + 1))(*itertools.accumulate(lengths, initial=0))


def aggv_slice_plan(lengths, cap):
    """-> [(a, b, cut, all32)]: slice [a, b), cut = "pairs" | "bytes" | "end", or None where one message does not fit (MI355_BLS_ERR_CAPACITY)"""
    L, n, offs = plan_lib(), len(lengths), _offsets(lengths)
    a, plan = 0, []
    while a < n:
        b = L.plan_aggv_cut(offs, n, a, cap)
        if b == a:
            return None
        cut = "end" if b == n else "pairs" if b - a >= cap else "bytes"
        plan.append((a, b, cut, bool(L.plan_aggv_all32(ctypes.cast(ctypes.byref(offs, 4 * a), ctypes.POINTER(ctypes.c_uint32)), b - a))))
        a = b
    return plan


def aggv_one_slice_cap(lengths):
    """the smallest context that takes the whole input in one slice (the cut is monotone in cap: bisection)"""
    L, n, offs = plan_lib(), len(lengths), _offsets(lengths)
    lo = hi = max(n, 1)
    while L.plan_aggv_cut(offs, n, 0, hi) != n:
        lo, hi = hi + 1, 2 * hi
    while lo < hi:
        mid = (lo + hi) // 2
        if L.plan_aggv_cut(offs, n, 0, mid) == n:
            hi = mid
        else:
            lo = mid + 1
    return hi


def varlen_defect(msgs, d):
    """A defect of tests/golden/aggv_varlen.json applied to the list of messages -> a new list."""
    out = list(msgs)
    i = d["index"]
    if d["kind"] == "shift":                                  # the first byte of message i + 1 moves to the end of message i: same bytes, one offset differs
        out[i], out[i + 1] = out[i] + out[i + 1][:1], out[i + 1][1:]
        assert b"".join(out) == b"".join(msgs)
    elif d["kind"] == "trail":                                # one byte appended (0x00, or the SHA padding byte 0x80)
        out[i] = out[i] + bytes([d["byte"]])
    elif d["kind"] == "flip":                                 # the lowest bit of the last byte of a long message
        assert len(out[i]) >= 4096
        out[i] = out[i][:-1] + bytes([out[i][-1] ^ 1])
    elif d["kind"] == "swap":                                 # two messages of different lengths change places
        j = d["other"]
        assert len(out[i]) != len(out[j])
        out[i], out[j] = out[j], out[i]
    else:
        raise ValueError(d["kind"])
    return out
