"""Lens-equation solver at its grid and list edges (gl_images.hip.h: map -> scan -> newton): the scan's tie rule and half-open
window bit for bit against the float64 restatement of tests/images_cases.py on dyadic linear maps (through
gl_image_positions_stage_counts, because Newton's merge hides a double claim from the public outputs); every split of the
triangle range over the scan's four waves; the candidate list below, at and beyond its 64 entries; which images survive
``max_images``; and coarse, rectangular, off-centre grids against the float64 Newton reference."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import images_cases as IC
from tests.test_gpu_image_positions import _c2_truth, _rows, _sim

pytestmark = pytest.mark.gpu

SQUARE, RECT = (-2.0, 2.0, -2.0, 2.0), (-1.0, 3.0, -1.5, 0.5)
MAX_S = 512  # sources per sample in one call


@functools.lru_cache(maxsize=None)
def _shear_sim():
    from gigalens_amd.profiles.mass.shear import Shear
    sim = _sim([Shear()], 16, 0.25, 1)
    assert [n for p in sim.phys_model.lenses for n in p._native_params()] == ["gamma1", "gamma2"]
    return sim


def _solve(sim, packed, sx, sy, window, n, c=1.0, max_images=8):
    """One call: x, y, mu [B, S, M], n, n_dropped, n_cand, n_over [B, S] as numpy (the model handle's call: it reports n_dropped
    as numbers; LensSimulator.image_positions turns them into a warning)."""
    B, S = sx.shape
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=sim.device)
    scales = None if c == 1.0 else np.full(S, c, np.float32)
    out, n_img, dropped = sim._model.image_positions(packed, f32(sx), f32(sy), window, n, max_images, IC._default_tol(window), 30,
                                                     scales=scales)
    n_cand, n_over = sim._model.image_positions_stage_counts(B, S, n)
    out = out.cpu().numpy().astype(np.float64)
    return (out[..., 0], out[..., 1], out[..., 2]) + tuple(t.cpu().numpy() for t in (n_img, dropped, n_cand, n_over))


def _as_rows(values, S):
    """[K] -> [ceil(K / S), S], the tail padded with the last value."""
    K = len(values)
    B = -(-K // S)
    return np.concatenate([values, np.full(B * S - K, values[-1])]).reshape(B, S)


# ---- a. the tie rule, exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,n", [(SQUARE, 4), (SQUARE, 8), (RECT, 8)])
@pytest.mark.parametrize("c", [1.0, 0.5])
@pytest.mark.parametrize("g1,g2", IC.SHEAR_MAPS)
def test_tie_rule_and_half_open_window(g1, g2, c, window, n):
    sim = _shear_sim()
    jac = IC.shear_jacobian(g1, g2, c)
    det = jac[0][0] * jac[1][1] - jac[0][1] * jac[1][0]
    X, Y, boundary = IC.quarter_lattice(window, n)
    SX, SY = IC.apply_jac(jac, X, Y)
    assert np.array_equal(SX, SX.astype(np.float32)) and np.array_equal(SY, SY.astype(np.float32))  # bit-exact sources
    # what the restatement says of every lattice point (exact on these inputs): 1 inside, 0 or 1 on the boundary
    want = np.ones(len(X), np.int64)
    for k in np.flatnonzero(boundary):
        r = IC.scan64(IC.shear_beta(g1, g2), window, n, SX[k], SY[k], scale=c)
        want[k] = len(r["hits"])
        assert want[k] == IC.boundary_claim(jac, window, X[k], Y[k])
    S = min(len(X), 363)  # (4 n + 1)^2 = 289 or 1089 = 3 x 363
    rows = lambda a: _as_rows(a, S)
    B = rows(X).shape[0]
    packed = _rows(sim, np.tile(np.array([[g1, g2]]), (B, 1)))
    x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, packed, rows(SX), rows(SY), window, n, c)
    tx, ty, want = rows(X), rows(Y), rows(want)
    print(f"g = ({g1}, {g2}), c = {c}, n = {n}: {int(boundary.sum())} boundary points, {int(want[rows(boundary)].sum())} claimed; "
          f"n_cand {np.bincount(n_cand.ravel()).tolist()}")
    assert np.array_equal(n_cand, want), np.argwhere(n_cand != want)
    assert np.all(n_over == 0) and np.all(dropped == 0)
    assert np.array_equal(n_img, want), np.argwhere(n_img != want)
    assert np.all(np.isnan(x[..., 1:])) and np.all(np.isnan(x[..., 0]) == (want == 0))
    got = want == 1
    gx, gy, gm = x[..., 0][got], y[..., 0][got], mu[..., 0][got]
    assert np.all(np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gm))
    bx, by = IC.apply_jac(jac, gx, gy)
    res = np.hypot(bx - rows(SX)[got], by - rows(SY)[got])
    assert res.max() <= 2 * IC._default_tol(window), res.max()
    # (the map is linear: the image is theta itself, to the residual gate carried through the inverse map)
    inv_norm = 1.0 / np.linalg.svd(np.array(jac), compute_uv=False).min()
    assert np.hypot(gx - tx[got], gy - ty[got]).max() <= 2 * IC._default_tol(window) * inv_norm
    np.testing.assert_allclose(gm, 1.0 / det, rtol=1e-4)


# ---- b. every split of the triangle range over the four waves --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 8, 12, 16])
@pytest.mark.parametrize("c", [1.0, 0.5])
def test_wave_ranges_one_source_per_triangle(n, c):
    sim = _shear_sim()
    window = SQUARE
    cx, cy = IC.triangle_centroids(window, n)
    T = 2 * n * n
    for maps in (((0.0, 0.0), (0.0, 0.5)), ((1.5, 0.0), (0.0, 0.0))):  # B = 2: a different map in each sample
        packed = _rows(sim, np.array(maps))
        jacs = [IC.shear_jacobian(g1, g2, c) for g1, g2 in maps]
        src = [IC.apply_jac(j, cx, cy) for j in jacs]
        sx, sy = (np.stack([s[k] for s in src]).astype(np.float32) for k in (0, 1))
        x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, packed, sx, sy, window, n, c)
        assert n_cand.shape == (2, T)
        assert np.all(n_cand == 1), np.argwhere(n_cand != 1)
        assert np.all(n_over == 0) and np.all(n_img == 1) and np.all(dropped == 0)
        assert np.all(np.isnan(x[..., 1:]))
        for b, jac in enumerate(jacs):
            bx, by = IC.apply_jac(jac, x[b, :, 0], y[b, :, 0])
            tol = 2 * IC._default_tol(window)
            assert np.hypot(bx - sx[b].astype(np.float64), by - sy[b].astype(np.float64)).max() <= tol
            # at its own triangle's centroid: the residual gate through the inverse map, plus the float32 rounding of the source
            inv_norm = 1.0 / np.linalg.svd(np.array(jac), compute_uv=False).min()
            slack = (tol + IC.EPS32 * max(np.abs(sx[b]).max(), np.abs(sy[b]).max())) * inv_norm
            assert np.hypot(x[b, :, 0] - cx, y[b, :, 0] - cy).max() <= slack
            det = jac[0][0] * jac[1][1] - jac[0][1] * jac[1][0]
            np.testing.assert_allclose(mu[b, :, 0], 1.0 / det, rtol=1e-4)


# ---- c. the candidate list: a source on the centre of an SIS (an Einstein ring) ---------------------------------------------------
@pytest.mark.parametrize("max_images", [8, 64])
@pytest.mark.parametrize("n", sorted(IC.RING_CASES))
def test_candidate_list_on_an_einstein_ring(n, max_images):
    from gigalens_amd.profiles.mass.sis import SIS
    ref, cx, cy = IC.ring_scan(n)
    hits = len(ref["hits"])
    # condition, not measurement: every triangle's decision holds by 1e-5 in float64 (float32 beta is good to ~3e-7 here)
    assert np.nanmin(np.abs(ref["margin"])) >= IC.RING_MARGIN
    assert (hits, ref["per_wave"]) == IC.RING_CASES[n][1:]
    sim = _sim([SIS()], 16, 0.25, 1)
    packed = _rows(sim, np.array([[1.0, cx, cy]]))
    assert float(packed[0, 1]) == cx and float(packed[0, 2]) == cy
    src = np.array([[cx]]), np.array([[cy]])
    x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, packed, *src, IC.RING_WINDOW, n, max_images=max_images)
    k = int(n_img[0, 0])
    print(f"n = {n}: {hits} hits, per wave {ref['per_wave']}; n_cand {n_cand[0, 0]}, n_over {n_over[0, 0]}, images {k} of "
          f"{max_images}, n_dropped {dropped[0, 0]}")
    assert n_cand[0, 0] == min(hits, IC.IMG_MAXC) == ref["n_cand"]
    assert n_over[0, 0] == hits - n_cand[0, 0] == ref["n_over"]
    # the final outputs: what the header promises
    assert 0 <= k <= max_images
    rows = np.stack([x[0, 0], y[0, 0], mu[0, 0]], 1)
    assert np.all(np.isfinite(rows[:k])), rows[:k]
    assert np.all(np.isnan(rows[k:]))
    order = sorted(range(k), key=lambda i: (rows[i, 0], rows[i, 1]))
    assert order == list(range(k))
    assert dropped[0, 0] >= n_over[0, 0]
    sx, sy = (torch.tensor(a.astype(np.float32), device=sim.device) for a in src)
    kw = dict(window=IC.RING_WINDOW, num_cells=n, max_images=max_images)
    if dropped[0, 0] > 0:
        with pytest.raises(RuntimeError, match="not returned"):
            sim.image_positions(packed, sx, sy, strict=True, **kw)
        with pytest.warns(RuntimeWarning, match="not returned"):
            sim.image_positions(packed, sx, sy, **kw)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            sim.image_positions(packed, sx, sy, strict=True, **kw)


def test_triangles_of_a_flagged_vertex_are_skipped():
    """An SIS centre bit for bit on an interior vertex: the vertex is flagged and its six triangles drop out of the scan.  (Its
    deflection is defined as 0 there; taken for a value, beta = theta at that vertex makes one more triangle claim each source below.)"""
    from gigalens_amd.profiles.mass.sis import SIS
    window, n = SQUARE, 8
    sim = _sim([SIS()], 16, 0.25, 1)
    packed = _rows(sim, np.array([[1.0, 0.0, 0.0]]))
    src = np.array([[0.05, 0.01, -0.2]], np.float32), np.array([[0.02, -0.3, 0.4]], np.float32)
    want = []
    for sx, sy in zip(src[0][0].astype(np.float64), src[1][0].astype(np.float64)):
        with np.errstate(all="ignore"):
            r = IC.scan64(IC.sis_beta(1.0, 0.0, 0.0), window, n, sx, sy)
        assert np.nanmin(np.abs(r["margin"])) >= IC.RING_MARGIN and int(np.isnan(r["margin"]).sum()) == 6
        want.append(len(r["hits"]))
    assert want == [6, 4, 1]
    x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, packed, *src, window, n)
    assert n_cand[0].tolist() == want and n_over[0].tolist() == [0, 0, 0]
    print(f"n_cand {n_cand[0].tolist()}, images {n_img[0].tolist()}, n_dropped {dropped[0].tolist()}")
    # |beta| < theta_E: two images each.  (The inner image of the third source lies in a cell that touches the flagged vertex, whose
    # triangles are skipped: within a cell of the singular centre the solver promises nothing, and only its outer image is required.)
    assert n_img[0].tolist()[:2] == [2, 2] and n_img[0, 2] >= 1
    r = np.hypot(src[0][0].astype(np.float64), src[1][0].astype(np.float64))
    for s in range(3):  # theta = beta (1 +- theta_E / |beta|), sorted by x
        exp = np.array(sorted((src[0][0, s] * (1 + sg / r[s]), src[1][0, s] * (1 + sg / r[s])) for sg in (1.0, -1.0)))
        k = int(n_img[0, s])
        d = np.hypot(x[0, s, :k, None] - exp[None, :, 0], y[0, s, :k, None] - exp[None, :, 1])
        assert d.min(1).max() <= 2e-5 and len(set(d.argmin(1).tolist())) == k  # every image returned is one of the closed form
        assert d[:, int(np.argmax(np.hypot(exp[:, 0], exp[:, 1])))].min() <= 2e-5  # the outer one among them


# ---- d. max_images: which images survive ------------------------------------------------------------------------------------------
def test_max_images_keeps_the_first_of_the_sorted_images():
    _, sim, truth = _c2_truth()
    packed = sim.pack(truth)
    window, n = (-4.0, 4.0, -4.0, 4.0), 128
    src = np.array([[0.03]]), np.array([[-0.02]])
    fx, fy, fmu, fn, fdrop, _, _ = _solve(sim, packed, *src, window, n, max_images=8)
    assert fn[0, 0] == 4 and fdrop[0, 0] == 0
    full = np.stack([fx[0, 0, :4], fy[0, 0, :4], fmu[0, 0, :4]], 1)
    assert sorted(range(4), key=lambda i: (full[i, 0], full[i, 1])) == [0, 1, 2, 3]
    for m in (1, 2, 3, 4, 5):
        x, y, mu, n_img, dropped, _, _ = _solve(sim, packed, *src, window, n, max_images=m)
        keep = min(4, m)
        assert x.shape == (1, 1, m) and n_img[0, 0] == keep
        got = np.stack([x[0, 0], y[0, 0], mu[0, 0]], 1)
        assert np.array_equal(got[:keep].astype(np.float32).view(np.int32), full[:keep].astype(np.float32).view(np.int32)), (m, got)
        assert np.all(np.isnan(got[keep:]))
        assert dropped[0, 0] == max(0, 4 - m), (m, dropped)


# ---- e. coarse and rectangular grids against the float64 Newton reference ------------------------------------------------------
GRIDS = [(40, (-3.0, 3.0, -3.0, 3.0)), (100, (-4.0, 4.0, -3.0, 3.0)), (24, (-2.5, 3.5, -2.0, 2.0))]


def c1_c2_draw(config, sim_of):
    """The C1 (SIE) and C2 (EPL + Shear, gamma >= 2) draws of tests/test_gpu_image_positions.py: packed rows and sources [B, S]."""
    from gigalens_amd import workloads
    B, S = 10, 3
    wl = workloads.make(config, num_pix=64, batch=B)
    sim = sim_of(wl, B)
    packed = H.sample_packed(wl, sim, seed=21)
    if config == "C2":
        packed[:, 1] = 2.0 + (packed[:, 1] - 2.0).abs()
    g = np.random.default_rng(5)
    theta_E = packed[:, 0].double().cpu().numpy()
    ccx, ccy = packed[:, 3 if config == "C1" else 4].cpu().numpy(), packed[:, 4 if config == "C1" else 5].cpu().numpy()
    frac = np.concatenate([g.uniform(0.0, 0.08, (B, 1)), g.uniform(0.15, 0.6, (B, S - 1))], axis=1)
    phi = g.uniform(0, 2 * np.pi, (B, S))
    srcx = (ccx[:, None] + frac * theta_E[:, None] * np.cos(phi)).astype(np.float32)
    srcy = (ccy[:, None] + frac * theta_E[:, None] * np.sin(phi)).astype(np.float32)
    return sim, packed, srcx, srcy


@pytest.mark.parametrize("n_cells,window", GRIDS)
@pytest.mark.parametrize("config", ["C1", "C2"])
def test_coarse_and_rectangular_grids_vs_f64(config, n_cells, window):
    from gigalens_amd.simulator import LensSimulator
    sim, packed, srcx, srcy = c1_c2_draw(config, lambda wl, B: LensSimulator(wl.phys_model, wl.sim_config, bs=B))
    srcx, srcy = (torch.tensor(a, device=sim.device) for a in (srcx, srcy))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        compared, counts = IC._check_against_f64(sim, packed, srcx, srcy, window, n_cells)
    print(f"{config} n = {n_cells} window {window}: {compared} of {srcx.numel()} pairs compared, image counts {sorted(set(counts))}")
    assert compared >= srcx.numel() // 2
