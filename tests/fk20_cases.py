"""The cases the fk20 tests share (tests/test_fk20_emu.py on the CPU, tests/test_gpu_fk20.py on the device): tests/golden/fk20.json, made by
tests/golden/gen_fk20.py from the oracle's point arithmetic and Python integers mod r.  Nothing here comes from the code under test."""
import functools
import json
import os

import frntt_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
R = fc.R
BITREV, H = 2, 4                                      # the flags
REDUCED = 2                                           # the status byte's bit
ROW = 96                                              # a blst_p1_affine image; all zero: infinity


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "fk20.json")) as f:
        return json.load(f)


TAU = int(fixture()["tau"], 16)


def cases():
    """-> [(name, n, k, flags, setup images, coefficient images, expected images, expected status bytes)] over every case and every flag
    value it is stored for"""
    out = []
    for c in fixture()["cases"]:
        for f in sorted(c["out"], key=int):
            out.append((c["name"], c["n"], c["k"], int(f), bytes.fromhex(c["setup"]), bytes.fromhex(c["polys"]), bytes.fromhex(c["out"][f]), bytes(c["status"])))
    return out


def case(name):
    return [c for c in fixture()["cases"] if c["name"] == name][0]


def coefficients(c):
    """the k rows of coefficient IMAGES as integers (some are >= r)"""
    v = fc.images(bytes.fromhex(c["polys"]))
    return [v[g * c["n"]:(g + 1) * c["n"]] for g in range(c["k"])]


def rows(b):
    return [b[i:i + ROW] for i in range(0, len(b), ROW)]


def circulant(c):
    """b of one polynomial: [c_(n-1), 0 (n times), c_0, ..., c_(n-2)]"""
    n = len(c)
    return [c[n - 1]] + [0] * n + list(c[:n - 1])
