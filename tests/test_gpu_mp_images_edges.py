"""The lens-equation solver on lens planes at its plane, grid and list edges (gl_multiplane_images.hip.h: map -> scan -> newton), against
the float64 restatements of tests/mp_images_edge_cases.py (tests/test_mp_images_edges_host.py asserts their conditions on the CPU).
The scan's counts are read through gl_multiplane_image_positions_stage_counts, because Newton's merge hides a double or a missed claim
from the public outputs.  Gates: those of tests/test_gpu_images_edges.py for the exact linear maps (counts bit for bit; residual
<= 2 tol, the image within 2 tol / sigma_min(A_t) of its lattice point, mu = 1 / det A_t to 1e-4), those of
``mp_images_cases.check_against_f64`` against the float64 solver."""
import warnings

import numpy as np
import pytest
import torch

from tests import images_cases as IC
from tests import mp_images_cases as C
from tests import mp_images_edge_cases as E
from tests import multilens_cases as MC
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
_SIMS = {}


def _sim(gl, key, phys_mp, B):
    from gigalens_amd.simulator import SimulatorConfig
    if (key, B) not in _SIMS:
        _SIMS[key, B] = gl.LensSimulator(phys_mp, SimulatorConfig(delta_pix=0.1, num_pix=8), bs=B)
    return _SIMS[key, B]


def _lens_t(lens_params):
    return [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)) for k, v in d.items()} for d in lens_params]


def _solve(sim, lens_params, sx, sy, rows, window, n, max_images=8):
    """One native call: x, y, mu [B, S, M] (float64 holding the float32 outputs), n_images, n_dropped, n_cand, n_over [B, S]."""
    B, S = np.shape(sx)
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=sim.device)
    packed = sim._pack_partial({"lens_mass": _lens_t(lens_params)})
    assert tuple(packed.shape)[0] == B
    out, n_img, dropped = sim._model.multiplane_image_positions(packed, f32(sx), f32(sy), np.asarray(rows, dtype=np.float32), window, n,
                                                                max_images, IC._default_tol(window), 30)
    n_cand, n_over = sim._model.multiplane_image_positions_stage_counts(B, S, n)
    out = out.cpu().numpy().astype(np.float64)
    return (out[..., 0], out[..., 1], out[..., 2]) + tuple(t.cpu().numpy() for t in (n_img, dropped, n_cand, n_over))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).view(np.int32)


def _repeat(lens_params, B):
    return [{k: np.repeat(np.asarray(v, dtype=np.float32)[:1], B) for k, v in d.items()} for d in lens_params]


# ---- 0. the read-back itself ----------------------------------------------------------------------------------------------------------
def test_stage_counts_entries_know_their_layout(gl):
    """The multi-plane entry reads behind the K maps; the single-plane entry refuses a model with planes, and the multi-plane entry a
    model without (before this, the single-plane entry copied bytes of the plane map of such a workspace)."""
    import ctypes

    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    L = _native.lib()
    c = E.linear_case("k3")
    sim = _sim(gl, "linear3", c["phys_mp"], 1)
    lp = E.shear_params([c["shears"]])
    with pytest.raises(_native.NativeLibraryError, match="no multiplane_image_positions call"):
        gl.LensSimulator(c["phys_mp"], SimulatorConfig(delta_pix=0.1, num_pix=8), bs=1)._model.multiplane_image_positions_stage_counts(1, 1, 4)
    # one source inside, one outside the window
    A = c["A"]
    sx, sy = IC.apply_jac(E.jac_tuple(A), np.array([0.25, 5.0]), np.array([-0.5, 0.0]))
    *_, n_img, dropped, n_cand, n_over = _solve(sim, lp, sx[None], sy[None], [c["target"]] * 2, E.SQUARE, 5)
    assert n_cand.dtype == np.int32 and n_cand.tolist() == [[1, 0]] and n_over.tolist() == [[0, 0]] and n_img.tolist() == [[1, 0]]
    ws = sim._model._scratch_bufs["multiplane_image_positions"]
    out = torch.full((2, 2), -7, dtype=torch.int32, device=sim.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    h = sim._model._h
    rc = L.gl_image_positions_stage_counts(h, 1, 2, 5, ptr(ws), ws.numel(), ptr(out[0]), ptr(out[1]), None)
    assert rc == _native.GL_EUNSUPPORTED and b"lens planes" in L.gl_last_error()
    with pytest.raises(_native.NativeLibraryError):  # (the binding: that model has filled no single-plane workspace)
        sim._model.image_positions_stage_counts(1, 2, 5)
    GL_EINVAL, GL_ENOMEM = -1, -4
    entry = L.gl_multiplane_image_positions_stage_counts
    need = L.gl_multiplane_image_positions_workspace_bytes(h, 1, 2, 5, 8)
    assert 0 < need <= ws.numel()
    assert entry(h, 1, 2, 5, ptr(ws), need - 1, ptr(out[0]), ptr(out[1]), None) == GL_ENOMEM
    for bad in ((0, 2, 5), (1, 0, 5), (1, 2, 0), (1, 2, 8193)):
        assert entry(h, *bad, ptr(ws), ws.numel(), ptr(out[0]), ptr(out[1]), None) == GL_EINVAL, bad
    plain = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:1], [], []), SimulatorConfig(delta_pix=0.1, num_pix=8), bs=1)
    assert entry(plain._model._h, 1, 2, 5, ptr(ws), ws.numel(), ptr(out[0]), ptr(out[1]), None) == GL_EINVAL
    assert b"gl_model_set_lens_planes has not been called" in L.gl_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all())  # nothing was copied by a refused call
    assert entry(h, 1, 2, 5, ptr(ws), need, ptr(out[0]), ptr(out[1]), None) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[1, 0], [0, 0]]


# ---- a. the tie rule and the half-open window, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("window,n", E.LATTICES)
@pytest.mark.parametrize("name", E.TIE_MAPS)
def test_tie_rule_and_half_open_window(gl, name, window, n):
    """One source per point of the quarter-cell lattice; even sources behind the planes of the map's own row, odd sources between
    planes 0 and 1, in ONE call: a kernel that takes another source's row, or another sample's or plane's map, misclaims."""
    c, rows, As = E.tie_rows(name)
    X, Y, boundary, SX, SY, row = E.tie_sources(name, window, n)
    want = E.tie_want(name, window, n)
    S = min(len(X), E.TIE_S)
    B = len(X) // S
    assert B * S == len(X)
    shape = lambda a: np.asarray(a).reshape(B, S)
    assert np.array_equal(shape(row), np.broadcast_to(np.arange(S) % 2, (B, S)))
    sim = _sim(gl, f"linear{len(c['shears'])}", c["phys_mp"], B)
    lp = E.shear_params([c["shears"]] * B)
    tx, ty, wnt = shape(X), shape(Y), shape(want)
    x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, lp, shape(SX), shape(SY), [rows[s % 2] for s in range(S)], window, n)
    assert np.all(np.isnan(x[..., 1:]))
    x, y, mu = x[..., 0], y[..., 0], mu[..., 0]
    print(f"{name} n = {n} window {window}: {int(boundary.sum())} boundary points, {int(want[boundary].sum())} claimed; "
          f"n_cand {np.bincount(n_cand.ravel()).tolist()}")
    assert np.array_equal(n_cand, wnt), np.argwhere(n_cand != wnt)
    assert np.all(n_over == 0) and np.all(dropped == 0)
    assert np.array_equal(n_img, wnt), np.argwhere(n_img != wnt)
    assert np.array_equal(np.isnan(x), wnt == 0)
    tol = IC._default_tol(window)
    for r_, A in enumerate(As):
        got = (wnt == 1) & (shape(row) == r_)
        gx, gy, gm = x[got], y[got], mu[got]
        assert got.sum() > 100 and np.all(np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gm))
        bx, by = IC.apply_jac(E.jac_tuple(A), gx, gy)
        assert np.hypot(bx - shape(SX)[got], by - shape(SY)[got]).max() <= 2 * tol
        inv_norm = 1.0 / np.linalg.svd(A, compute_uv=False).min()
        assert np.hypot(gx - tx[got], gy - ty[got]).max() <= 2 * tol * inv_norm
        np.testing.assert_allclose(gm, 1.0 / np.linalg.det(A), rtol=1e-4)


# ---- b. every split of the triangle range over the four waves; the [b][k][v] strides -----------------------------------------------------
@pytest.mark.parametrize("K,n", [(K, n) for K in sorted(E.WAVE_CELLS) for n in E.WAVE_CELLS[K]])
def test_wave_ranges_one_source_per_triangle(gl, K, n):
    phys, phys_mp, mp, lp, row, As = E.wave_case(K)
    sim = _sim(gl, f"linear{K}", phys_mp, 3)
    window = E.SQUARE
    cx, cy = IC.triangle_centroids(window, n)
    T = 2 * n * n
    src = [IC.apply_jac(E.jac_tuple(A), cx, cy) for A in As]
    sx, sy = (np.stack([s[k] for s in src]).astype(np.float32) for k in (0, 1))
    x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, lp, sx, sy, [row] * T, window, n)
    assert n_cand.shape == (3, T)
    assert np.all(n_cand == 1), np.argwhere(n_cand != 1)
    assert np.all(n_over == 0) and np.all(n_img == 1) and np.all(dropped == 0)
    assert np.all(np.isnan(x[..., 1:]))
    tol = 2 * IC._default_tol(window)
    for b, A in enumerate(As):
        bx, by = IC.apply_jac(E.jac_tuple(A), x[b, :, 0], y[b, :, 0])
        assert np.hypot(bx - sx[b].astype(np.float64), by - sy[b].astype(np.float64)).max() <= tol
        # at its own triangle's centroid: the residual gate through the inverse map, plus the float32 rounding of the source
        inv_norm = 1.0 / np.linalg.svd(A, compute_uv=False).min()
        slack = (tol + IC.EPS32 * max(np.abs(sx[b]).max(), np.abs(sy[b]).max())) * inv_norm
        assert np.hypot(x[b, :, 0] - cx, y[b, :, 0] - cy).max() <= slack
        np.testing.assert_allclose(mu[b, :, 0], 1.0 / np.linalg.det(A), rtol=1e-4)


# ---- c. the flag rules per plane ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.FLAG_CASES)
def test_flag_rules_per_plane(gl, name):
    """A singular centre bit for bit on the ray of an interior vertex, on the lens's own plane: the sources behind that plane lose the
    vertex's six triangles; a source in front of it loses none, and sees bit for bit what it sees with the lens moved far away."""
    c = E.flag_case(name)
    sim = _sim(gl, "flag " + name, c["phys_mp"], 1)
    near, far = E.flag_scans(name), E.flag_scans(name, far=True)
    sx, sy = c["sx"][None], c["sy"][None]
    got = _solve(sim, c["lens_params"], sx, sy, c["rows"], E.FLAG_WINDOW, E.FLAG_CELLS)
    away = _solve(sim, c["far"], sx, sy, c["rows"], E.FLAG_WINDOW, E.FLAG_CELLS)
    print(f"{name}: n_cand {got[5][0].tolist()} (lens far away: {away[5][0].tolist()}), images {got[3][0].tolist()}, n_dropped {got[4][0].tolist()}")
    assert got[5][0].tolist() == [r["n_cand"] for r in near] and got[6][0].tolist() == [0] * len(near)
    assert away[5][0].tolist() == [r["n_cand"] for r in far] and away[6][0].tolist() == [0] * len(far)
    for s, flagged in enumerate(c["flagged"]):
        if flagged:
            continue
        for k in range(7):  # x, y, mu (the same bits), n_images, n_dropped, n_cand, n_over of that source
            same = _bits if k < 3 else np.asarray
            assert np.array_equal(same(got[k][0, s]), same(away[k][0, s])), (s, k)
        assert got[3][0, s] >= 1
    # the images that are returned solve the lens equation of their own row
    tol = IC._default_tol(E.FLAG_WINDOW)
    for s in range(len(near)):
        k = int(got[3][0, s])
        deriv = C.deriv64(c["phys"], c["mp"], c["lens_params"], 0, c["rows"][s])
        res = IC._residual64(deriv, got[0][0, s, :k], got[1][0, s, :k], float(c["sx"][s]), float(c["sy"][s]))
        assert np.all(res <= 2 * tol) and np.all(np.isnan(got[0][0, s, k:]))


def test_nan_sample_leaves_its_neighbour_alone(gl):
    """B = 2 with a NaN lens parameter in sample 1: every vertex of that sample is flagged on every plane behind the NaN -- no
    candidate, no image, nothing dropped, all-NaN outputs; sample 0 is bit for bit the B = 1 call."""
    c = E.flag_case("second")
    lp2 = _repeat(c["lens_params"], 2)
    lp2[0]["gamma2"][1] = np.nan  # the Shear of plane 0: plane 1 is reached not finite
    S = len(c["sx"])
    sx, sy = np.tile(c["sx"], (2, 1)), np.tile(c["sy"], (2, 1))
    two = _solve(_sim(gl, "flag second", c["phys_mp"], 2), lp2, sx, sy, c["rows"], E.FLAG_WINDOW, E.FLAG_CELLS)
    one = _solve(_sim(gl, "flag second", c["phys_mp"], 1), c["lens_params"], sx[:1], sy[:1], c["rows"], E.FLAG_WINDOW, E.FLAG_CELLS)
    for k in (3, 4, 5, 6):
        assert two[k][1].tolist() == [0] * S, k
        assert np.array_equal(two[k][0], one[k][0])
    for k in (0, 1, 2):
        assert np.all(np.isnan(two[k][1]))
        assert np.array_equal(_bits(two[k][0]), _bits(one[k][0]))
    assert int(one[3].min()) >= 1


# ---- d. the candidate list below, at and beyond 64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_images", [8, 64])
@pytest.mark.parametrize("sis_plane", E.RING_PLACEMENTS)
@pytest.mark.parametrize("n", sorted(IC.RING_CASES))
def test_candidate_list_on_an_einstein_ring(gl, monkeypatch, n, sis_plane, max_images):
    phys, phys_mp, mp, lp, cx, cy = E.ring_case(n, sis_plane)
    ref = E.ring_scan(n, sis_plane)
    hits = len(ref["hits"])
    assert (hits, ref["per_wave"]) == IC.RING_CASES[n][1:]
    sim = _sim(gl, f"ring {n} {sis_plane}", phys_mp, 1)
    src = np.array([[cx]]), np.array([[cy]])
    x, y, mu, n_img, dropped, n_cand, n_over = _solve(sim, lp, *src, [E.RING_ROW], IC.RING_WINDOW, n, max_images=max_images)
    k = int(n_img[0, 0])
    print(f"n = {n}, SIS on plane {sis_plane}: {hits} hits, per wave {ref['per_wave']}; n_cand {n_cand[0, 0]}, n_over {n_over[0, 0]}, "
          f"images {k} of {max_images}, n_dropped {dropped[0, 0]}")
    assert n_cand[0, 0] == min(hits, IC.IMG_MAXC) == ref["n_cand"]
    assert n_over[0, 0] == hits - n_cand[0, 0] == ref["n_over"]
    assert 0 <= k <= max_images
    rows = np.stack([x[0, 0], y[0, 0], mu[0, 0]], 1)
    assert np.all(np.isfinite(rows[:k])), rows[:k]
    assert np.all(np.isnan(rows[k:]))
    assert sorted(range(k), key=lambda i: (rows[i, 0], rows[i, 1])) == list(range(k))
    assert dropped[0, 0] >= n_over[0, 0]
    # the public call on the same row: any redshift behind both planes names the row (1, 1) on this model
    monkeypatch.setattr(mp, "target_scales", lambda z: np.asarray(E.RING_ROW, dtype=np.float64))
    sx, sy = (torch.tensor(a.astype(np.float32)) for a in src)
    kw = dict(window=IC.RING_WINDOW, num_cells=n, max_images=max_images, source_redshifts=2.0)
    if dropped[0, 0] > 0:
        with pytest.raises(RuntimeError, match="not returned"):
            sim.image_positions(_lens_t(lp), sx, sy, strict=True, **kw)
        with pytest.warns(RuntimeWarning, match="not returned"):
            out = sim.image_positions(_lens_t(lp), sx, sy, **kw)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = sim.image_positions(_lens_t(lp), sx, sy, strict=True, **kw)
    assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(x)) and out[3].cpu().tolist() == [[k]]


# ---- e. max_images: which images survive ---------------------------------------------------------------------------------------------
def test_max_images_keeps_the_first_of_the_sorted_images(gl):
    phys, phys_mp, mp, lp = C.four_plane_case()
    sim = _sim(gl, "four_planes", phys_mp, 1)
    src = np.array([[E.MAX_IMAGES_SOURCE[0]]]), np.array([[E.MAX_IMAGES_SOURCE[1]]])
    rows = [mp.target_scales(E.MAX_IMAGES_Z)]
    fx, fy, fmu, fn, fdrop, _, _ = _solve(sim, lp, *src, rows, C.GENERAL_WINDOW, C.GENERAL_CELLS, max_images=8)
    found = int(fn[0, 0])
    full = np.stack([fx[0, 0, :found], fy[0, 0, :found], fmu[0, 0, :found]], 1)
    assert found >= 3 and fdrop[0, 0] == 0
    assert C.compare_images(full, E.max_images_reference(), "four planes") >= 3  # the images of the float64 solver, all of them
    assert sorted(range(found), key=lambda i: (full[i, 0], full[i, 1])) == list(range(found))
    for m in range(1, found + 2):
        x, y, mu, n_img, dropped, _, _ = _solve(sim, lp, *src, rows, C.GENERAL_WINDOW, C.GENERAL_CELLS, max_images=m)
        keep = min(found, m)
        assert x.shape == (1, 1, m) and n_img[0, 0] == keep
        got = np.stack([x[0, 0], y[0, 0], mu[0, 0]], 1)
        assert np.array_equal(_bits(got[:keep]), _bits(full[:keep])), (m, got)
        assert np.all(np.isnan(got[keep:]))
        assert dropped[0, 0] == max(0, found - m), (m, dropped)


# ---- f. other windows and a strongly rotated map against the float64 solver ------------------------------------------------------------
# (every lens set of multilens_cases.MAP_CASES on the general window: tests/test_gpu_mp_images.py over mp_images_cases.GENERAL)
@pytest.mark.parametrize("n_cells,window", E.WINDOWS)
@pytest.mark.parametrize("name", E.WINDOW_SETS)
def test_coarse_rectangular_and_off_centre_windows(gl, name, n_cells, window):
    c = MC.map_case(name)
    z, sx, sy = E.window_sources(name, n_cells)
    sim = _sim(gl, name, c["phys_mp"], 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        compared, counts = C.check_against_f64(sim, c["phys"], c["mp"], c["lens_params"], z, sx, sy, window, n_cells,
                                               maps=C.reference_maps(name))
    print(f"{name} n = {n_cells} window {window}: pairs compared {compared}, images per pair {counts}")
    assert 4 * (6 - compared) <= 6 and max(counts) >= 3


def test_rotated_map_against_float64(gl):
    """A_t far from symmetric on a map that is not linear (mp_images_edge_cases.rotated_case): Newton must step on A_t itself."""
    phys, phys_mp, mp, lp = E.rotated_case()
    sim = _sim(gl, "rotated", phys_mp, 1)
    sx, sy = (np.asarray(a, dtype=np.float32) for a in E.ROTATED_SOURCES)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        compared, counts = C.check_against_f64(sim, phys, mp, lp, E.ROTATED_Z, sx, sy, E.ROTATED_WINDOW, E.ROTATED_CELLS)
    assert compared == len(E.ROTATED_Z) and min(counts) >= 1
