"""Shared helpers for tests: fixture loading and canonicalisation of projective outputs."""
import ctypes
import json
import os

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


# ---- the latency-mode plan of one blocking batch call (csrc/host_api.inc), restated for the tests that must sit on its boundaries.
# S = the context's wave slots (4 x CU count).  test_latency_plan_mirror.py reads these constants and bounds out of host_api.inc.
TEAM_CLEAR_ITEMS_PER_SLOT = 11      # the lane-team engine clears up to 11 S messages, k_hash_clear beyond (launch_hash_clear)
TEAM_LINES_ITEMS_PER_SLOT = 18      # the engine walks up to 18 S pairs' Miller lines, k_lines beyond (launch_lines)
SIG_WIDE_MIN = 40000                # the signature side's 8-bit digits (2048 extra pairs) from here, 4-bit ones (256) below
FORK_ITEMS_PER_SLOT = 16            # run_pairs: `fork` up to 16 S sets, `fork_sig` beyond
WAVE = 64


def rows_max(S):
    """team_form_for: the row executor's bound (room left for the fork streams' waves)"""
    return (S - S // 8) // 4


def team_form(count, S):
    """team_form_for: which form of an engine kernel (clearing or Miller lines) takes `count` items"""
    if count <= rows_max(S):
        return "rows"
    if count <= 2 * rows_max(S):
        return "rows2"
    return "spread" if (count + 3) // 4 <= S else "wide"


def latency_plan(n, S):
    """The executors a latency-mode (cooperative) context with side streams picks for a blocking call of n sets."""
    if (2 * n + 3) // 4 <= S - S // 8:
        hash_map = "rows"                                     # k_hash_map_rows
    elif (2 * n + WAVE - 1) // WAVE <= S:
        hash_map = "spread"                                   # k_hash_map_spread
    else:
        hash_map = "plain"                                    # k_hash_map
    clear = "team_" + team_form(n, S) if n <= TEAM_CLEAR_ITEMS_PER_SLOT * S else "one_lane"      # ... + k_clear_fix | k_hash_clear
    lines = "team_" + team_form(n, S) if n <= TEAM_LINES_ITEMS_PER_SLOT * S else "one_lane"      # the tuple pairs' lines | k_lines
    side = "fork" if n <= FORK_ITEMS_PER_SLOT * S else "fork_sig"
    extra = 2048 if n >= SIG_WIDE_MIN else 256
    return {"hash_map": hash_map, "clear": clear, "side": side, "lines": lines, "extra_pairs": extra}


def latency_hand_overs(S):
    """(stage, t): the plan changes `stage`'s executor between t and t + 1 sets - the hand-overs of the 4 S .. 32 S range."""
    return [("clear", 4 * S), ("clear", TEAM_CLEAR_ITEMS_PER_SLOT * S), ("side", FORK_ITEMS_PER_SLOT * S),
            ("lines", 4 * S), ("lines", TEAM_LINES_ITEMS_PER_SLOT * S), ("hash_map", 32 * S)]


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
