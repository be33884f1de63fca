"""The cases the cell-proof tests share (tests/test_fk20_cells_emu.py on the CPU, tests/test_gpu_fk20_cells.py on the device):
tests/golden/fk20_cells.json, made by tests/golden/gen_fk20_cells.py from the oracle's point arithmetic and Python integers mod r.  Nothing
here comes from the code under test."""
import functools
import json
import os

import frntt_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
R = fc.R
BITREV, H = 2, 4                                      # the flags
REDUCED = 2                                           # the status byte's bit
ROW = 96                                              # a blst_p1_affine image; all zero: infinity
INF = bytes(ROW)


@functools.lru_cache(maxsize=None)
def fixture():
    """the fixture with every image and every polynomial written out: it stores each distinct image once (`points`), the cases name images
    by number, and a case whose polynomials an earlier case holds names that case (and takes its own first k of them)"""
    with open(os.path.join(HERE, "golden", "fk20_cells.json")) as f:
        fx = json.load(f)
    pts = fx["points"]
    assert pts[0] == INF.hex() and len(set(pts)) == len(pts)
    by = {c["name"]: c for c in fx["cases"]}
    for c in fx["cases"]:
        if c["polys"] in by:
            c["polys"] = by[c["polys"]]["polys"][:c["k"] * c["n"] * 64]
        c["setup"] = "".join(pts[i] for i in c["setup"])
        c["out"] = {f: "".join(pts[i] for i in v) for f, v in c["out"].items()}
    return fx


TAU = int(fixture()["tau"], 16)


@functools.lru_cache(maxsize=None)
def cases():
    """-> ((name, n, k, cell, ext, flags, setup images, coefficient images, expected images, expected status bytes)) over every case and
    every flag value it is stored for"""
    out = []
    for c in fixture()["cases"]:
        for f in sorted(c["out"], key=int):
            out.append((c["name"], c["n"], c["k"], c["cell"], c["ext"], int(f), bytes.fromhex(c["setup"]), bytes.fromhex(c["polys"]), bytes.fromhex(c["out"][f]),
                        bytes(c["status"])))
    return tuple(out)


def case(name):
    return [c for c in fixture()["cases"] if c["name"] == name][0]


def coefficients(c):
    """the k rows of coefficient IMAGES as integers (some are >= r)"""
    v = fc.images(bytes.fromhex(c["polys"]))
    return [v[g * c["n"]:(g + 1) * c["n"]] for g in range(c["k"])]


def rows(b):
    return [b[i:i + ROW] for i in range(0, len(b), ROW)]


def per_poly(c, flags):
    """the images one polynomial of case c gives under flags"""
    q = c["n"] // c["cell"]
    return q if flags & H else q << c["ext"]
