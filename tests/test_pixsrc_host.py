"""The float64 restatement of the pixelated source reconstruction (tests/pixsrc_cases.py), pinned without a GPU and independently of
the kernels: its forward operator against the interpolated-light restatement, its evidence against the Gaussian marginal
likelihood computed directly, the closed-form ``log det R`` against a dense determinant, and the zero rows of the mapping."""
import math

import numpy as np
import pytest
import torch

from tests import interp_cases as IC
from tests import pixsrc_cases as PC


def _lens_params(c, B, dtype=torch.float64):
    return [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype).reshape(-1).expand(B) for k, v in d.items()}
            for d in c["params"]["lens_mass"]]


def test_forward_identity_with_interpolated_light():
    """``F s`` == the image of the same lens with ONE source ``Interpolated(image=s, order=1)`` at ``center``, ``phi = 0``,
    ``scale = pitch``, amplitude 1 (interp_cases.expected_image: a dense contraction per pixel, coded independently of ``L`` and
    ``F``), with a PSF at supersample 2, to 1e-11 of the largest pixel."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light import Interpolated
    from oracle import ref_torch as ref
    c = PC.case("A")
    B, kw = c["B"], c["kw"]
    ny, nx = kw["n_src"]
    s = np.stack([PC.smooth_source((ny, nx), b) for b in range(B)]).astype(np.float32)
    rs = ref.RefSimulator(c["phys"], c["cfg"], B, supersampled_kernel=c["psf"])
    fx, fy = PC.frame_beta(rs, _lens_params(c, B))
    for b in range(B):
        pitch, cx, cy = float(kw["pitch"][b]), float(kw["center"][0][b]), float(kw["center"][1][b])
        F = PC.operator(rs, PC.mapping(fx[:, b], fy[:, b], (ny, nx), pitch, cx, cy)).numpy()
        got = (F @ s[b].reshape(-1).astype(np.float64)).reshape(12, 10)
        phys = PhysicalModel(list(c["phys"].lenses), [], [Interpolated(s[b], order=1)])
        rsi = ref.RefSimulator(phys, c["cfg"], B, supersampled_kernel=c["psf"])
        one = lambda v: torch.full((B,), float(v), dtype=torch.float64)
        params = {"lens_mass": _lens_params(c, B),
                  "source_light": [dict(center_x=one(cx), center_y=one(cy), phi=one(0.0), scale=one(pitch), amp=one(1.0))]}
        want = IC.expected_image(rsi, params)[b].numpy()
        assert np.abs(want).max() > 0
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("reg", PC.REGS)
@pytest.mark.parametrize("n_src", [(2, 2), (3, 2)])
def test_evidence_is_the_gaussian_marginal_likelihood(reg, n_src):
    """``log_evidence`` == ``log N(y; 0, C + F (lambda R)^-1 F^T)`` computed directly in float64 (30 used pixels), to 1e-9 relative."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    c = PC.case("C11")
    phys = PhysicalModel([SIE(), Shear()], [], [Sersic()])
    cfg = SimulatorConfig(delta_pix=PC.DELTA_PIX, num_pix=(6, 6), supersample=1)
    mask = np.ones((6, 6), dtype=bool)
    mask[0, :] = False  # 30 used pixels
    rng = np.random.default_rng(19)
    err = (0.02 * rng.uniform(0.7, 1.4, size=(6, 6))).astype(np.float32)
    obs = (0.05 * rng.normal(size=(6, 6))).astype(np.float32)
    lam = np.float32(0.7)
    kw = dict(n_src=n_src, pitch=np.float32(0.12), center=(np.float32(0.01), np.float32(-0.02)), regularization=reg,
              strength=np.asarray([lam]), mask=mask)
    out, parts = PC.reconstruct(phys, cfg, None, c["params"], obs, err, **kw, return_parts=True)
    _, F, y, _, _ = parts[0]
    assert F.shape == (30, n_src[0] * n_src[1]) and np.abs(F).max() > 0
    sig = err.astype(np.float64).reshape(-1)[np.flatnonzero(mask.reshape(-1))]
    K = np.diag(sig ** 2) + F @ np.linalg.inv(float(lam) * PC.reg_matrix(reg, n_src)) @ F.T
    sign, logdet = np.linalg.slogdet(K)
    want = -0.5 * y @ np.linalg.solve(K, y) - 0.5 * logdet - 0.5 * len(y) * math.log(2 * math.pi)
    assert sign > 0
    assert abs(out["log_evidence"][0] - want) <= 1e-9 * abs(want)


@pytest.mark.parametrize("n_src", [(1, 1), (2, 3), (7, 6), (32, 32)])
@pytest.mark.parametrize("reg", PC.REGS)
def test_log_det_regularization_closed_form(reg, n_src):
    from gigalens_amd.simulator import LensSimulator
    got, want = LensSimulator.log_det_regularization(reg, n_src), PC.log_det_reg(reg, n_src)
    assert abs(got - want) <= 1e-10 * max(1.0, abs(want))


def test_unknown_regularization_is_refused():
    from gigalens_amd.simulator import LensSimulator
    with pytest.raises(ValueError, match="regularization"):
        LensSimulator.log_det_regularization("laplace", (3, 3))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_zero_rows(dtype):
    """Rows of ``L`` for a ``beta`` that is not finite, or far outside the grid, are exactly zero; a ray on a node has weight 1."""
    nan, inf = float("nan"), float("inf")
    bx = torch.tensor([0.0, nan, 0.0, inf, -inf, 1e30, 0.5, 0.0, -0.101], dtype=dtype)
    by = torch.tensor([0.0, 0.0, nan, 0.0, 0.0, 0.0, 0.0, -3e38, 0.0], dtype=dtype)
    L = PC.mapping(bx, by, (3, 4), 0.1, 0.05, 0.0).numpy()
    assert L.shape == (9, 12)
    assert np.all(L[1:8] == 0) and not np.isnan(L).any()
    assert L[0, 1 * 4 + 1] == 1.0 and np.count_nonzero(L[0]) == 1  # u = v = 1 exactly: node (1, 1) alone
    assert np.count_nonzero(L[8]) == 1  # u = -0.01: only node 0 of the row still sees the ray (zero extension)


def test_native_entries_validate_without_gpu():
    """The two C-ABI entries exist and refuse a null model before anything is launched."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    lib = _native.lib()
    assert lib.gl_pixsrc_workspace_bytes(None, 2, 1, 4, 4, 100) == 0
    null = ctypes.c_void_p(0)
    rc = lib.gl_pixsrc_reconstruct(None, null, null, 2, null, null, null, null, 100, 4, 4, null, 1, null, 1, null, null, null, null,
                                   null, 0, null)
    assert rc == -1 and b"null" in lib.gl_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the restatement from rays and the case matrix of tests/test_gpu_pixsrc_matrix.py
# ---------------------------------------------------------------------------------------------------------------------
def _dense_operator(c, u, v):
    """``F [H W, S]`` of one sample written with loops, independently of ``mapping`` / ``operator``: the hat product per (ray, node),
    a true 2-D convolution with the PSF (zero outside the frame), then the mean over ``ss x ss`` blocks."""
    (ny, nx), (H, W), ss, psf = c["n_src"], c["frame"], c["ss"], c["psf"]
    Hs, Ws = H * ss, W * ss
    F = np.zeros((H * W, ny * nx))
    for j in range(ny):
        for i in range(nx):
            plane = (np.maximum(0, 1 - np.abs(v - j)) * np.maximum(0, 1 - np.abs(u - i))).reshape(Hs, Ws)
            if psf is not None:
                kh, kw = psf.shape
                pad = np.pad(plane, ((kh // 2, kh // 2), (kw // 2, kw // 2)))
                plane = sum(float(psf[a, b]) * pad[kh - 1 - a:kh - 1 - a + Hs, kw - 1 - b:kw - 1 - b + Ws]
                            for a in range(kh) for b in range(kw))
            F[:, j * nx + i] = plane.reshape(H, ss, W, ss).mean(axis=(1, 3)).reshape(-1)
    return F


@pytest.mark.parametrize("name", ["pixels_31", "pixels_33", "stencil_curvature_3x3"])
def test_reconstruct_from_rays_is_the_dense_solve(name):
    """``reconstruct_from_rays`` in float64 against an operator written with loops, ``numpy.linalg.solve`` and the Gaussian marginal
    likelihood computed directly: per-sample rays, data and rms, a scattered mask, with and without a lens light, a PSF at
    supersample 2.  Source to 1e-9 of its largest element, evidence to 1e-9 relative."""
    c, inp, ref, _ = PC.matrix_data(name)
    (ny, nx), pix = c["n_src"], inp["pix"]
    R = PC.reg_matrix(c["reg"], c["n_src"])
    for b in range(c["B"]):
        pitch, cx, cy = (float(x) for x in inp["pose"][b])
        u = (inp["beta_x"][b].astype(np.float64) - cx) / pitch + (nx - 1) / 2
        v = (inp["beta_y"][b].astype(np.float64) - cy) / pitch + (ny - 1) / 2
        F = _dense_operator(c, u, v)[pix]
        sig, lam = inp["sigma"][b].astype(np.float64), float(inp["strength"][b, 0])
        y = inp["obs"][b].astype(np.float64) - (0 if inp["lens_light"] is None else inp["lens_light"][b].astype(np.float64)[pix])
        s = np.linalg.solve(F.T @ (F / sig[:, None] ** 2) + lam * R, F.T @ (y / sig ** 2))
        assert np.abs(ref["source"][b, 0].reshape(-1) - s).max() <= 1e-9 * np.abs(s).max()
        K = np.diag(sig ** 2) + F @ np.linalg.inv(lam * R) @ F.T
        sign, logdet = np.linalg.slogdet(K)
        want = -0.5 * y @ np.linalg.solve(K, y) - 0.5 * logdet - 0.5 * len(y) * math.log(2 * math.pi)
        assert sign > 0 and abs(ref["log_evidence"][b, 0] - want) <= 1e-9 * abs(want)
        img = np.zeros(c["frame"][0] * c["frame"][1]) if inp["lens_light"] is None else inp["lens_light"][b].astype(np.float64)
        img[pix] += F @ s
        assert np.abs(ref["model_image"][b, 0].reshape(-1) - img).max() <= 1e-9 * np.abs(img).max()


@pytest.mark.parametrize("name", ["hand_identity", "hand_curvature"])
def test_hand_placed_rays(name):
    """The rays placed by hand do what the case says, on the float64 and the float32 mapping alike; the sample whose every ray
    misses has the zero source and ``log det M = S log lambda + log det R`` (the host's closed form) in float64."""
    from gigalens_amd.simulator import LensSimulator
    c, inp, ref, f32 = PC.matrix_data(name)
    (ny, nx), S = c["n_src"], 45
    pitch, cx, cy = (float(x) for x in inp["pose"][0])
    for dtype in (torch.float64, torch.float32):
        L = PC.mapping(torch.from_numpy(inp["beta_x"][0]).to(dtype), torch.from_numpy(inp["beta_y"][0]).to(dtype), c["n_src"], pitch,
                       cx, cy).numpy()
        assert np.array_equal(L[:S - 1], np.delete(np.eye(S), 2 * nx + 4, axis=0))  # on the nodes bar (2, 4): unit rows
        assert np.all(L[:, 2 * nx + 4] == 0) and np.all(L.sum(axis=0)[np.arange(S) != 2 * nx + 4] > 1)  # node (2, 4): no ray
        edge = L[S - 1:S - 1 + 16]  # u, then v, at -2, -1, n, n + 1 and one float32 step either side of -2 and n + 1: zero rows
        assert np.all(edge == 0)
        border = L[S + 15:S + 23]  # inside (-1, 0) and (n - 1, n): the zero extension leaves one node per axis, weights 1/4 or 3/4
        assert np.all(np.count_nonzero(border, axis=1) <= 2) and np.all(border.sum(axis=1) > 0) and np.all(border.sum(axis=1) < 1)
        assert np.all(L[S + 23:S + 29] == 0) and not np.isnan(L).any()  # NaN, +inf, -inf in u, then in v
        miss = PC.mapping(torch.from_numpy(inp["beta_x"][1]).to(dtype), torch.from_numpy(inp["beta_y"][1]).to(dtype), c["n_src"],
                          pitch, cx, cy).numpy()
        assert np.all(miss == 0)
    for beta, n, c0, q0 in ((inp["beta_x"][0], nx, cx, S - 1), (inp["beta_y"][0], ny, cy, S + 7)):
        for w in (np.float32, np.float64):  # the kernel's float32 arithmetic and the reference's float64: the steps straddle the range test
            g = (beta[q0:q0 + 8].astype(w) - w(c0)) / w(pitch) + w((n - 1) / 2)
            assert g.dtype == w and np.array_equal(g[:4], [-2, -1, n, n + 1])
            assert g[4] < -2 < g[5] < -1.99999 and n + 0.99999 < g[6] < n + 1 < g[7]
        assert np.array_equal(PC.grid_coordinate(beta[q0:q0 + 8], pitch, c0, n), g.astype(np.float32))
    for out in (ref, f32):
        assert np.all(out["source"][1] == 0) and np.all(out["model_image"][1] == 0) and np.all(out["reg"][1] == 0)
    want = S * math.log(float(inp["strength"][1, 0])) + LensSimulator.log_det_regularization(c["reg"], c["n_src"])
    assert abs(ref["log_det"][1, 0] - want) <= 1e-10 * abs(want)
    assert np.abs(ref["source"][0]).max() > 0 and np.abs(ref["source"][2]).max() > 0


@pytest.mark.parametrize("name", PC.LOOPS)
def test_matrix_split_claims(name):
    """The split each host-loop case states, against the restatement of ``pix_layout`` (the GPU test asserts it on the library)."""
    PC.check_split(name, PC._case_layout(name))
    assert all(0 <= b < PC.MATRIX[name]["B"] for b in PC.alone_samples(name))


def test_layout_restatement_against_the_library():
    """``pixsrc_layout`` (the library's own ``pix_layout``) against the restatement, for every case; skipped where no model can be
    created (no GPU)."""
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    from gigalens_amd.simulator import LensSimulator
    if not torch.cuda.is_available():
        pytest.skip("a model needs a GPU")
    for name, c in PC.MATRIX.items():
        phys, cfg, psf = PC.matrix_sim_args(name)
        sim = LensSimulator(phys, cfg, bs=c["B"], supersampled_kernel=psf)
        n_used = c["n_used"] or c["frame"][0] * c["frame"][1]
        assert sim._model.pixsrc_layout(c["B"], c["L"], c["n_src"], n_used) == PC._case_layout(name), name


def test_layout_entry_validates_without_gpu():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    lib = _native.lib()
    out = (ctypes.c_int32 * 4)()
    assert lib.gl_pixsrc_layout(None, 2, 1, 4, 4, 100, out) == -1
    assert lib.gl_pixsrc_layout(None, 2, 1, 4, 4, 100, None) == -1


def test_matrix_conditions_on_the_reference():
    """Every case of the matrix: ``ok`` everywhere outside the failure case, ``cond(M) <= 1e4`` for every (sample, strength), every
    gate of the main matrix (4 x the worst float32-restatement error) <= 1e-5; the harder system has ``cond(M)`` in [1e3, 1e4]; the
    float32 restatement flags sample 0 of the failure case and not sample 1."""
    keys = PC.ARRAYS + PC.SCALARS
    worst = {k: 0.0 for k in keys}
    for name in PC.MAIN + ("hard",):
        c, inp, ref, f32 = PC.matrix_data(name)
        assert ref["ok"].all() and f32["ok"].all(), name
        assert np.all(ref["cond"] <= 1e4), (name, ref["cond"])
        assert np.all(inp["strength"] >= 10) and np.all(inp["strength"] <= 100) or name == "hard"
        assert np.all(np.isfinite(inp["sigma"])) and np.all(inp["sigma"] > 0)
        assert np.array_equal(np.unique(inp["pix"]), inp["pix"])
        assert inp["pix"][0] == 0 and inp["pix"][-1] == c["frame"][0] * c["frame"][1] - 1
        e = PC.errors(f32, ref, c["n_src"][0] * c["n_src"][1])
        print(f"float32 yardstick {name}: " + ", ".join(f"{k} {e[k]:.3e}" for k in keys)
              + f"; cond {ref['cond'].min():.3g} .. {ref['cond'].max():.3g}")
        if name != "hard":
            worst = {k: max(worst[k], e[k]) for k in keys}
    print("float32 yardstick maxima: " + ", ".join(f"{k} {worst[k]:.3e}" for k in keys))
    for k in keys:
        assert 4 * worst[k] <= 1e-5, (k, worst[k])
    assert np.all(PC.matrix_data("hard")[2]["cond"] >= 1e3)
    c, inp, ref, f32 = PC.matrix_data("pivot")
    assert f32["ok"][:, 0].tolist() == [False, True] and np.all(inp["sigma"] > 0) and np.all(np.isfinite(inp["sigma"]))
    assert {n: PC.MATRIX[n]["n_used"] for n in PC.MATRIX if n.startswith("pixels_")} == \
        {f"pixels_{n}": n for n in (5, 31, 32, 33, 64, 95, 120)}
