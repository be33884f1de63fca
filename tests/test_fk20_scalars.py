"""tests/fk20_scalars.py against itself and against the stored fixtures: the O(n) form for an SRS, the two defining sums and the long
division by X^l - omega_N^j agree, and for every SRS case of tests/golden/fk20.json and tests/golden/fk20_cells.json the module's scalars
name the fixture's images - a scalar becomes an image through the case's own setup entries (tau^i -> entry i) and through the C oracle's
[a]G (tests/g1_images.py) for the rest."""
import random

import pytest

import fk20_cases as k1
import fk20_cells_cases as kc
import fk20_scalars as ks
import frntt_cases as fc
import g1_images as gi

R = ks.R
SHAPES = [(16, 4, 1), (64, 16, 0), (64, 16, 1), (128, 64, 2), (256, 128, 1), (512, 64, 1)]


@pytest.mark.parametrize("n,l,ext", SHAPES)
def test_the_three_statements_agree(n, l, ext):
    rng = random.Random(n * 1000 + l * 10 + ext)
    tau = rng.randrange(2, R)
    c = [rng.randrange(R) for _ in range(n)]
    q, big = n // l, (n // l) << ext
    hs = ks.srs_h(tau, c, l)
    assert len(hs) == q and hs[q - 1] == 0 and (q == 1 or all(hs[:q - 1]))
    assert hs == ks.h_scalars(ks.srs(tau, n), c, l)
    pis = ks.srs_pi(tau, c, l, ext)
    assert len(pis) == big and pis == ks.pi_scalars(hs, ext)
    assert pis == [ks.quotient_at(c, l, pow(fc.omega(big), j, R), tau) for j in range(big)]
    assert len(set(pis)) == (big if q > 2 else 1)                            # no trivial list; q = 2: h_1 = 0 and every pi_j is h_0
    assert ks.expected_srs(tau, [c], l, ext, ks.BITREV) == ks.expected_any(ks.srs(tau, n), [c], l, ext, ks.BITREV)
    assert (ks.expected_srs(tau, [c], l, ext, ks.BITREV) != [pis]) == (q > 2)
    assert ks.expected_srs(tau, [c], l, ext, ks.H) == [hs] and ks.expected_srs(tau, [c], l, ext, 0) == [pis]


def test_one_polynomial_of_4096_in_the_o_n_form():
    """the form the device tests lean on at sizes the sums cannot reach: checked against the division at three j"""
    n = 4096
    c = list(fc.random_vectors(4096, 1, n)[0])
    pis = ks.srs_pi(kc.TAU, c, 1, 0)
    for j in (0, 1, 4095):
        assert pis[j] == ks.quotient_at(c, 1, pow(fc.omega(n), j, R), kc.TAU)


def images_of(scalars, known):
    return b"".join(known[a] if a in known else gi.multiples_of_g_cpu([a]) for a in scalars)


def test_the_modules_scalars_name_the_fixtures_images():
    assert kc.TAU == k1.TAU
    tau = kc.TAU
    powers = ks.srs(tau, 64)
    srs_images = gi.multiples_of_g_cpu(powers)                               # the oracle's own SRS: which cases hold one
    seen, not_srs = 0, []
    old = [(c["name"], c["n"], 1, 0, c["setup"], k1.coefficients(c), c["out"]) for c in k1.fixture()["cases"]]
    new = [(c["name"], c["n"], c["cell"], c["ext"], c["setup"], kc.coefficients(c), c["out"]) for c in kc.fixture()["cases"]]
    for name, n, l, ext, setup, polys, out in old + new:
        setup = bytes.fromhex(setup)
        if setup != srs_images[:n * 96]:
            not_srs.append(name)
            continue
        known = {0: gi.INF}
        known.update({powers[i]: setup[i * 96:(i + 1) * 96] for i in range(n)})          # the fixture's own entries
        for f, want in out.items():
            rows = ks.expected_srs(tau, polys, l, ext, int(f))
            assert images_of([a for row in rows for a in row], known) == bytes.fromhex(want), (name, f)
            seen += 1
    assert not_srs == ["linear_n8", "sums_n16"] and seen > 50
