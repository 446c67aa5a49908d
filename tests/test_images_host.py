"""The float64 restatement of the lens-equation solver's scan stage (tests/images_cases.py scan64) on inputs where it is exact:
dyadic linear maps on dyadic grids.  Every interior point of the quarter-cell lattice -- vertices, edge and diagonal midpoints,
interiors -- is claimed by exactly one triangle; the window is half-open in the way `claimed_sides` derives from the ownership
rule alone; and the frozen Einstein-ring cases of the candidate-list tests have the hit counts and margins they are used for.
No device needed."""
import functools

import numpy as np
import pytest

from tests import images_cases as IC

WINDOWS = [((-2.0, 2.0, -2.0, 2.0), 4), ((-2.0, 2.0, -2.0, 2.0), 8), ((-1.0, 3.0, -1.5, 0.5), 8)]
MAPS = [(g1, g2, c) for g1, g2 in IC.SHEAR_MAPS for c in (1.0, 0.5)]


@functools.lru_cache(maxsize=None)
def _claims(g1, g2, c, window, n):
    """Hits per lattice point: theta [K, 2], boundary [K], number of claiming triangles [K], the Jacobian."""
    jac = IC.shear_jacobian(g1, g2, c)
    X, Y, boundary = IC.quarter_lattice(window, n)
    SX, SY = IC.apply_jac(jac, X, Y)
    counts = np.array([len(IC.scan64(IC.shear_beta(g1, g2), window, n, sx, sy, scale=c)["hits"]) for sx, sy in zip(SX, SY)])
    return X, Y, boundary, counts, jac


@pytest.mark.parametrize("window,n", WINDOWS)
@pytest.mark.parametrize("g1,g2,c", MAPS)
def test_every_interior_lattice_point_is_claimed_once(g1, g2, c, window, n):
    X, Y, boundary, counts, _ = _claims(g1, g2, c, window, n)
    assert np.all(counts[~boundary] == 1), list(zip(X[~boundary][counts[~boundary] != 1], Y[~boundary][counts[~boundary] != 1]))
    assert np.all(counts[boundary] <= 1)


@pytest.mark.parametrize("window,n", WINDOWS)
@pytest.mark.parametrize("g1,g2,c", MAPS)
def test_the_window_is_half_open_as_the_rule_says(g1, g2, c, window, n):
    X, Y, boundary, counts, jac = _claims(g1, g2, c, window, n)
    want = np.array([IC.boundary_claim(jac, window, x, y) for x, y in zip(X[boundary], Y[boundary])])
    assert np.array_equal(counts[boundary], want)
    # one of bottom / top and one of left / right, so: a side without its far corner (4 n points) + a side with neither corner
    # or with both ... in every case 8 n - 1 of the 16 n boundary points
    sides = IC.claimed_sides(jac)
    assert sides["bottom"] != sides["top"] and sides["left"] != sides["right"]
    assert counts[boundary].sum() == 8 * n - 1 and boundary.sum() == 16 * n


def test_which_sides_each_orientation_claims():
    # identity: bottom and right; 31 of the 64 boundary lattice points of a 4 x 4 grid
    assert IC.claimed_sides(IC.shear_jacobian(0.0, 0.0)) == dict(bottom=True, right=True, top=False, left=False)
    _, _, boundary, counts, _ = _claims(0.0, 0.0, 1.0, (-2.0, 2.0, -2.0, 2.0), 4)
    assert (int(counts[boundary].sum()), int((counts[boundary] == 0).sum())) == (31, 33)
    # beta = (-0.5 x, 2.5 y), negative parity: the mirror image in x -- bottom and LEFT
    assert IC.claimed_sides(IC.shear_jacobian(1.5, 0.0)) == dict(bottom=True, right=False, top=False, left=True)
    # the sheared map beta = (x - y / 2, y - x / 2): the bottom side runs downwards in the source plane, so TOP and right
    assert IC.claimed_sides(IC.shear_jacobian(0.0, 0.5)) == dict(bottom=False, right=True, top=True, left=False)


def test_negative_parity_mirrors_positive_parity():
    """beta = (-x / 2, 5 y / 2) against its mirror image beta = (+x / 2, 5 y / 2): the image theta of a source is claimed once
    under both, by the same triangle with the same seed wherever no tie decides, and on the boundary the claimed sides are
    mirrored in x."""
    window, n = (-2.0, 2.0, -2.0, 2.0), 4
    X, Y, boundary = IC.quarter_lattice(window, n)
    neg, pos = IC.shear_jacobian(1.5, 0.0), ((0.5, 0.0), (0.0, 2.5))
    assert neg == ((-0.5, 0.0), (0.0, 2.5))
    beta_pos = lambda x, y: (0.5 * x, 2.5 * y)
    for x, y, bd in zip(X, Y, boundary):
        a = IC.scan64(IC.shear_beta(1.5, 0.0), window, n, *IC.apply_jac(neg, x, y))
        b = IC.scan64(beta_pos, window, n, *IC.apply_jac(pos, x, y))
        if not bd:
            assert len(a["hits"]) == len(b["hits"]) == 1
            if a["margin"][a["hits"][0]] > 0:  # strictly inside: the same triangle, the same seed
                assert a["hits"][0] == b["hits"][0] and np.array_equal(a["seeds"], b["seeds"])
            assert np.array_equal(a["seeds"], [[x, y]]) and np.array_equal(b["seeds"], [[x, y]])
        else:
            assert len(a["hits"]) == IC.boundary_claim(neg, window, x, y)
            assert len(b["hits"]) == IC.boundary_claim(pos, window, x, y)
    sn, sp = IC.claimed_sides(neg), IC.claimed_sides(pos)
    assert (sn["left"], sn["right"]) == (sp["right"], sp["left"]) and (sn["bottom"], sn["top"]) == (sp["bottom"], sp["top"])


def test_seeds_are_the_preimage_and_waves_add_up():
    window, n = (-1.0, 3.0, -1.5, 0.5), 8
    for g1, g2, c in MAPS:
        jac = IC.shear_jacobian(g1, g2, c)
        cx, cy = IC.triangle_centroids(window, n)
        for t in (0, 1, 31, 32, 33, 64, 127):
            sx, sy = IC.apply_jac(jac, cx[t], cy[t])
            r = IC.scan64(IC.shear_beta(g1, g2), window, n, sx, sy, scale=c)
            assert r["hits"].tolist() == [t] and r["n_cand"] == 1 and r["n_over"] == 0
            assert r["per_wave"] == [int(w == t // 32) for w in range(4)]
            np.testing.assert_allclose(r["seeds"], [[cx[t], cy[t]]], rtol=0, atol=1e-14)
    # a range that is no multiple of four: T = 50, per = 13, the last wave holds 11 -- every triangle belongs to one wave
    window, n = (-2.0, 2.0, -2.0, 2.0), 5
    cx, cy = IC.triangle_centroids(window, n)
    for t in range(2 * n * n):
        r = IC.scan64(IC.shear_beta(0.0, 0.5), window, n, *IC.apply_jac(IC.shear_jacobian(0.0, 0.5), cx[t], cy[t]))
        assert r["hits"].tolist() == [t] and r["per_wave"] == [int(w == t // 13) for w in range(4)]


def test_flagged_and_degenerate_triangles_are_skipped():
    window, n = (-2.0, 2.0, -2.0, 2.0), 4
    # a NaN vertex at (0, 0): its six triangles drop out, a source inside one of them has no claim
    def holed(x, y):
        bad = (x == 0) & (y == 0)
        return np.where(bad, np.nan, x), np.where(bad, np.nan, y)
    assert len(IC.scan64(holed, window, n, 0.25, 0.125)["hits"]) == 0
    assert len(IC.scan64(holed, window, n, 1.25, 0.125)["hits"]) == 1
    r = IC.scan64(holed, window, n, 1.25, 0.125)
    assert int(np.isnan(r["margin"]).sum()) == 6
    # a map that squashes the plane onto a line: every triangle has zero area
    assert len(IC.scan64(lambda x, y: (x + y, x + y), window, n, 0.5, 0.5)["hits"]) == 0


@pytest.mark.parametrize("n", sorted(IC.RING_CASES))
def test_ring_cases_have_their_counts_and_margins(n):
    (_, hits, per_wave) = IC.RING_CASES[n]
    r, cx, cy = IC.ring_scan(n)
    assert len(r["hits"]) == hits and r["per_wave"] == per_wave
    assert np.nanmin(np.abs(r["margin"])) >= IC.RING_MARGIN
    assert r["n_cand"] == min(hits, 64) and r["n_over"] == hits - min(hits, 64)
    # what each grid is for
    if n == 16:
        assert hits < 64
    if n == 32:
        assert max(per_wave) <= 64 < hits
    if n == 72:
        assert max(per_wave) > 64
