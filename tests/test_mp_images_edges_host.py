"""CPU-side conditions of the edge cases of the lens-equation solver on lens planes (tests/mp_images_edge_cases.py): the new read-back
of the scan counts is exported, declared and bound; the closed-form Jacobians are those of the table the cases were designed on; the
tie-rule inputs are exact in float32, so that ``images_cases.scan64`` restates the kernel bit for bit and not merely closely; every
margin the GPU tests (tests/test_gpu_mp_images_edges.py) rely on holds in float64; and the float64 solver alone meets the caps of the
general cases.  No device is needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import images_cases as IC
from tests import mp_images_cases as C
from tests import mp_images_edge_cases as E
from tests import multilens_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOL = "gl_multiplane_image_positions_stage_counts"


def _f32_exact(*arrays):
    return all(np.array_equal(np.asarray(a, np.float64), np.asarray(a, np.float64).astype(np.float32)) for a in arrays)


def test_stage_counts_symbol_exported_declared_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    raw = ctypes.CDLL(_native.lib_path())
    header = open(os.path.join(ROOT, "include", "gigalens_hip.h")).read()
    assert hasattr(raw, NEW_SYMBOL) and f" {NEW_SYMBOL}(" in header
    assert _native.SYMBOLS[NEW_SYMBOL] == _native.SYMBOLS["gl_image_positions_stage_counts"]
    assert getattr(_native.lib(), NEW_SYMBOL).argtypes == _native.SYMBOLS[NEW_SYMBOL][1]
    assert callable(_native.Model.multiplane_image_positions_stage_counts)


# ---- exact linear maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.LINEAR))
def test_linear_jacobians_are_those_of_the_table(name):
    c = E.linear_case(name)
    det, asym = E.LINEAR_TABLE[name]
    A = c["A"]
    assert abs(np.linalg.det(A) - det) <= 5e-4 and abs((A[0, 1] - A[1, 0]) - asym) <= 5e-4, (name, A)
    assert _f32_exact(A)
    # the recursion of multilens_cases in float64 IS this matrix: beta(theta) = A theta at a few dyadic points, exactly
    lp = E.shear_params([c["shears"]])
    X, Y = np.array([1.0, 0.0, -0.75, 0.5]), np.array([0.0, 1.0, 0.25, -1.5])
    bx, by = E.plane_beta(c["phys"], c["mp"], lp, 0, c["target"])(X, Y)
    ex, ey = IC.apply_jac(E.jac_tuple(A), X, Y)
    assert np.array_equal(bx, ex) and np.array_equal(by, ey)


def test_linear_jacobian_generalises_the_two_shear_case():
    _, _, mp, lp, T, A = MC.two_shear_case()
    shears = [(float(d["gamma1"][0]), float(d["gamma2"][0])) for d in lp]
    couplings = {(0, 1): float(np.float32(mp.lens_scales[0, 1]))}
    got = E.linear_jacobian(shears, couplings, [float(np.float32(t)) for t in T])
    assert np.abs(got - A).max() <= 1e-15


@pytest.mark.parametrize("window,n", E.LATTICES)
@pytest.mark.parametrize("name", E.TIE_MAPS)
def test_tie_rule_inputs_are_exact_in_float32(name, window, n):
    """Sources, vertex values, plane sums and every edge function of the scan are the same numbers in float32 and in float64; the
    scan's count on the boundary is the half-open rule ``boundary_claim`` on the row's own A_t; both rows are used and differ."""
    c, rows, As = E.tie_rows(name)
    assert not np.array_equal(As[0], As[1]) and all(abs(np.linalg.det(A)) > 0.1 for A in As)
    if name == "rot":
        assert rows[1] == E.LINEAR["front"][2] and np.array_equal(As[1], E.linear_case("front")["A"])
    X, Y, boundary, SX, SY, row = E.tie_sources(name, window, n)
    assert len(X) == (4 * n + 1) ** 2 and _f32_exact(SX, SY)
    lp = E.shear_params([c["shears"]])
    xs, ys = IC.grid_vertices(window, n)
    VX, VY = (a.ravel() for a in np.meshgrid(xs, ys))
    vx, vy = torch.as_tensor(VX), torch.as_tensor(VY)
    sums = MC.plane_sums(c["phys"], c["mp"], E.sample_params(lp, 0), vx, vy)
    for (ax, ay), (px, py) in zip(sums, E.plane_positions(c["mp"], sums, vx, vy)):
        assert _f32_exact(ax.numpy(), ay.numpy(), px.numpy(), py.numpy())
    for r in (0, 1):
        bx, by = E.plane_beta(c["phys"], c["mp"], lp, 0, rows[r])(VX, VY)
        assert _f32_exact(bx, by)
        pick = row == r
        w32 = E.edge_functions(bx, by, n, SX[pick], SY[pick], np.float32)
        w64 = E.edge_functions(bx, by, n, SX[pick], SY[pick], np.float64)
        assert np.array_equal(w32, w64)
    want = E.tie_want(name, window, n)
    for k in np.flatnonzero(boundary):
        assert want[k] == IC.boundary_claim(E.jac_tuple(As[row[k]]), window, X[k], Y[k]), (k, X[k], Y[k])
    # (both outcomes occur on the boundary, under both rows)
    for r in (0, 1):
        assert set(want[boundary & (row == r)].tolist()) == {0, 1}
    # an interior point: one triangle, checked on a sample of them against the scan itself
    for k in np.flatnonzero(~boundary)[:: max(1, len(X) // 40)]:
        assert len(E.scan(c["phys"], c["mp"], lp, 0, rows[row[k]], window, n, SX[k], SY[k])["hits"]) == 1


@pytest.mark.parametrize("K", sorted(E.WAVE_SHEARS))
def test_wave_range_maps(K):
    """Three different non-singular maps in the three samples; a source at a triangle's centroid is claimed by that triangle alone
    (checked with the scan on the coarsest and the finest grid of the case, on the float32 values of the sources)."""
    phys, _, mp, lp, row, As = E.wave_case(K)
    assert mp.K == K and len(As) == 3
    assert all(abs(np.linalg.det(A)) > 0.1 for A in As)
    assert all(not np.array_equal(As[i], As[j]) for i in range(3) for j in range(i))
    for n in (min(E.WAVE_CELLS[K]), max(E.WAVE_CELLS[K])):
        cx, cy = IC.triangle_centroids(E.SQUARE, n)
        for b, A in enumerate(As):
            sx, sy = (a.astype(np.float32) for a in IC.apply_jac(E.jac_tuple(A), cx, cy))
            for t in range(0, len(cx), max(1, len(cx) // 8)):
                r = E.scan(phys, mp, lp, b, row, E.SQUARE, n, sx[t], sy[t])
                assert r["hits"].tolist() == [t] and np.nanmin(np.abs(r["margin"])) >= IC.RING_MARGIN


# ---- flag rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.FLAG_CASES)
def test_flag_cases(name):
    c = E.flag_case(name)
    phys, mp, lp = c["phys"], c["mp"], c["lens_params"]
    xs, ys = IC.grid_vertices(E.FLAG_WINDOW, E.FLAG_CELLS)
    vx, vy = c["vertex"]
    assert vx in xs[1:-1] and vy in ys[1:-1]  # an interior vertex
    # the singular centre is, bit for bit, where the ray from that vertex meets the lens's own plane
    l = [type(p).__name__ for p in phys.lenses].index("SIS")
    j = int(mp.plane_of_lens[l])
    assert j == {"front": 0, "second": 1, "third": 2}[name]
    x, y = torch.tensor([vx], dtype=torch.float64), torch.tensor([vy], dtype=torch.float64)
    sums = MC.plane_sums(phys, mp, E.sample_params(lp, 0), x, y)
    pj = E.plane_positions(mp, sums, x, y)[j]
    assert (float(pj[0]), float(pj[1])) == c["centre"] and _f32_exact(c["centre"])
    assert float(lp[l]["center_x"][0]) == c["centre"][0] and float(lp[l]["center_y"][0]) == c["centre"][1]
    if j > 0:
        assert c["centre"] != c["vertex"]  # (the flag must be taken on theta_j, not on theta)
    near, far = E.flag_scans(name), E.flag_scans(name, far=True)
    assert len(near) == len(c["flagged"]) and True in c["flagged"]
    for s, (a, b) in enumerate(zip(near, far)):
        flagged = c["flagged"][s]
        assert flagged == bool(c["rows"][s][j] != 0)
        print(f"{name} source {s} row {c['rows'][s].tolist()}: {len(a['hits'])} hit(s), {int(np.isnan(a['margin']).sum())} triangles skipped, "
              f"smallest margin {np.nanmin(np.abs(a['margin'])):.2e}")
        assert int(np.isnan(a["margin"]).sum()) == (6 if flagged else 0) and int(np.isnan(b["margin"]).sum()) == 0
        assert np.nanmin(np.abs(a["margin"])) >= IC.RING_MARGIN and np.nanmin(np.abs(b["margin"])) >= IC.RING_MARGIN
        assert len(a["hits"]) >= 1
        if not flagged:  # the SIS is not part of this source's ray at all
            assert np.array_equal(a["hits"], b["hits"]) and np.array_equal(a["seeds"], b["seeds"])
            # ... and its hit is a triangle of the vertex: a scan that lets the plane behind the source flag it loses the hit
            assert set(a["hits"].tolist()) & set(E.vertex_triangles(c["vertex"], E.FLAG_WINDOW, E.FLAG_CELLS))
        else:
            assert np.all(np.isnan(a["margin"][E.vertex_triangles(c["vertex"], E.FLAG_WINDOW, E.FLAG_CELLS)]))
    if name != "front":
        assert False in c["flagged"]


# ---- the ring through two planes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sis_plane", E.RING_PLACEMENTS)
@pytest.mark.parametrize("n", sorted(IC.RING_CASES))
def test_ring_through_two_planes_is_the_single_plane_ring(n, sis_plane):
    phys, _, mp, lp, cx, cy = E.ring_case(n, sis_plane)
    assert [type(p).__name__ for p in phys.lenses][sis_plane] == "SIS" and float(mp.lens_scales[0, 1]) == 0.5
    xs, ys = IC.grid_vertices(IC.RING_WINDOW, n)
    X, Y = np.meshgrid(xs, ys)
    bx, by = E.plane_beta(phys, mp, lp, 0, E.RING_ROW)(X, Y)
    ex, ey = IC.sis_beta(1.0, cx, cy)(X, Y)
    assert np.abs(bx - ex).max() <= 1e-15 and np.abs(by - ey).max() <= 1e-15
    r = E.ring_scan(n, sis_plane)
    assert (len(r["hits"]), r["per_wave"]) == IC.RING_CASES[n][1:]
    assert np.nanmin(np.abs(r["margin"])) >= IC.RING_MARGIN and not np.isnan(r["margin"]).any()


def test_max_images_source_is_multiply_imaged():
    ref = E.max_images_reference()
    assert len(ref) >= 3 and not C.fold_pair(ref, C.GENERAL_WINDOW, C.GENERAL_CELLS)


# ---- every lens set, other windows ------------------------------------------------------------------------------------------------------
def _caps(name, ref, z, sx, sy, window, n_cells):
    """The caps of the general cases on a reference ``{(b, s): [K, 3]}``."""
    c = MC.map_case(name)
    folds = [k for k, r in ref.items() if C.fold_pair(r, window, n_cells)]
    assert 4 * len(folds) <= len(ref), folds
    assert max(int(np.sum(np.abs(r[:, 2]) >= C.MU_MIN)) for k, r in ref.items() if k not in folds) >= 3
    for (b, s), r in ref.items():
        if (b, s) in folds:
            continue
        for xi, yi, mi in r:
            if abs(mi) >= C.MU_MIN:
                d = C.singular_centre_cells(name, b, c["mp"].target_scales(z[s]), xi, yi, window, n_cells)
                assert d >= 1.0, (b, s, xi, yi, d)
        # the solver's own procedure, run in float64, yields every compared image on this grid
        assert E.yields_every_image(c["phys"], c["mp"], c["lens_params"], b, c["mp"].target_scales(z[s]), sx[b, s], sy[b, s], window,
                                    n_cells, r), (b, s)
    X, Y = E.window_vertices(n_cells, window)
    assert MC.min_centre_distance(c["phys"], c["mp"], c["lens_params"], X, Y) >= 1e-3


@pytest.mark.parametrize("name", ["shared", "dpis|sie", "nfw|dpie|sis>"])
def test_every_lens_set_reaches_the_solver(name):
    """The three lens sets added to ``mp_images_cases.GENERAL``: one source between the last two planes, one behind all, and no vertex
    of the general window on a lens centre (the other caps: tests/test_mp_images_host.py runs over GENERAL)."""
    assert set(C.GENERAL) == set(MC.MAP_CASES)
    c = MC.map_case(name)
    z, sx, sy = C.general_sources(name)
    zp = c["mp"].z_planes
    assert zp[-2] < z[0] < zp[-1] < z[1]
    _caps(name, C.general_reference(name), z, sx, sy, C.GENERAL_WINDOW, C.GENERAL_CELLS)
    if name == "dpis|sie":  # the excess is there: the reference mu is not the derivative of the deflection
        T = c["mp"].target_scales(z[1])
        plain = C.solve64(c["phys"], c["mp"], c["lens_params"], 0, T, sx[0, 1], sy[0, 1], C.GENERAL_WINDOW, 2 * C.GENERAL_CELLS)
        ref = C.general_reference(name)[0, 1]
        assert C.reference_maps(name) is MC.maps_hessian and np.array_equal(plain[:, :2], ref[:, :2])
        assert np.abs(plain[:, 2] / ref[:, 2] - 1).max() > 10 * 1e-3
    else:
        assert C.reference_maps(name) is None


@pytest.mark.parametrize("n_cells,window", E.WINDOWS)
@pytest.mark.parametrize("name", E.WINDOW_SETS)
def test_window_sources_meet_the_caps(name, n_cells, window):
    z, sx, sy = E.window_sources(name, n_cells)
    assert sx.shape == sy.shape == (3, 2) and window[1] - window[0] != window[3] - window[2]
    _caps(name, E.window_reference(name, n_cells, window), z, sx, sy, window, n_cells)


def test_rotated_map_defeats_a_transposed_jacobian():
    phys, _, mp, lp = E.rotated_case()
    assert mp.K == 2 and mp.target_scales(E.ROTATED_Z[0])[1] == 0 and mp.target_scales(E.ROTATED_Z[1])[1] > 0
    ref, rate = E.rotated_reference()
    slow = 0
    for s, z in enumerate(E.ROTATED_Z):
        assert len(ref[s]) >= 1 and not C.fold_pair(ref[s], E.ROTATED_WINDOW, E.ROTATED_CELLS)
        for (xi, yi, mi), r in zip(ref[s], rate[s]):
            assert abs(mi) >= C.MU_MIN
            d = C.singular_centre_cells_of(phys, mp, lp, 0, mp.target_scales(z), xi, yi, E.ROTATED_WINDOW, E.ROTATED_CELLS)
            print(f"source {s}: image ({xi:+.4f}, {yi:+.4f}) mu {mi:+.3f}, {d:.2f} cells from the SIS centre, transposed-Newton rate {r:.3f}")
            assert d >= 1.0
            slow += r >= E.ROTATED_RATE
    assert slow >= 2
    X, Y = E.window_vertices(E.ROTATED_CELLS, E.ROTATED_WINDOW)
    assert MC.min_centre_distance(phys, mp, lp, X, Y) >= 1e-3
