"""Point images in the pixel likelihood without a GPU: the identities of the float64 restatement (tests/point_image_cases.py), the
argument validation of the gl_ptimg_* entries, and the host logic of model.PointImageProbModel."""
import ctypes

import numpy as np
import pytest
import torch

from tests import point_image_cases as PI
from tests import post_cases as PO


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


INTERIOR = [(0.0, 0.0), (0.37, -0.81), (0.5, 0.25), (-0.999, 0.001)]  # offsets from the frame centre, supersampled pixels


@pytest.mark.parametrize("cam_name", ["plain9", "ss2_psf5", "ss3_psf7", "rot_even"])
def test_unit_image_keeps_the_flux_of_the_psf(cam_name):
    """sum(D) = sum(psf) whenever the 16 taps and the PSF footprint lie inside the frame (partition of unity)."""
    cam = PI.camera(cam_name)
    Hs, Ws = cam["H"] * cam["ss"], cam["W"] * cam["ss"]
    total = 1.0 if cam["psf"] is None else float(cam["psf"].astype(np.float64).sum())
    for du, dv in INTERIOR:
        D = PI.unit_image_uv(cam, torch.tensor(Ws // 2 + du, dtype=PI.F64), torch.tensor(Hs // 2 + dv, dtype=PI.F64))
        assert abs(float(D.sum()) - total) <= 1e-13, (cam_name, du, dv, float(D.sum()) - total)


@pytest.mark.parametrize("cam_name", ["plain9", "ss2_psf5", "ss3_psf7", "rot_even", "ss2_psf3_mask"])
def test_unit_image_at_a_node_is_the_post_processing_of_a_one_hot_frame(cam_name):
    cam = PI.camera(cam_name)
    ss = cam["ss"]
    Hs, Ws = cam["H"] * ss, cam["W"] * ss
    for r, c in [(Hs // 2, Ws // 2), (0, 0), (Hs - 1, 2), (1, Ws - 1)]:
        D = PI.unit_image_uv(cam, torch.tensor(float(c), dtype=PI.F64), torch.tensor(float(r), dtype=PI.F64)).numpy()
        hot = np.zeros((1, Hs, Ws))
        hot[0, r, c] = 1.0
        scale = 0.0064
        want = PO.post_fwd_f64(hot, cam["psf"], ss, scale)[0] * (ss * ss / scale)
        assert np.abs(D - want).max() <= 1e-14, (cam_name, r, c)


def test_positions_map_back_to_the_grid():
    """(u, v) is the inverse of pix2angle on the supersampled grid, T / T^T quirk included (the rotated camera is not symmetric)."""
    from oracle import ref_torch as ref
    for name in ("rot_even", "ss2_psf5", "ss3_psf7"):
        cam = PI.camera(name)
        wcs = ref.LensWCS(n=cam["cfg"].num_pix, supersample=cam["ss"], transform_pix2angle=cam["cfg"].transform_pix2angle,
                          pix_scale=PI.DELTA_PIX)
        cols, rows = np.array([0.0, 3.0, 7.0]), np.array([1.0, 5.0, 2.0])
        T = wcs.transform_pix2angle
        ra = T[0, 0] * cols + T[1, 0] * rows + wcs.radec_at_xy_0[0]   # pix2angle in float64
        dec = T[0, 1] * cols + T[1, 1] * rows + wcs.radec_at_xy_0[1]
        u, v = PI.uv_of(cam, torch.as_tensor(ra), torch.as_tensor(dec))
        assert np.abs(u.numpy() - cols).max() <= 1e-12 and np.abs(v.numpy() - rows).max() <= 1e-12, name


@pytest.mark.parametrize("name", PI.SOLVABLE)
def test_solvable_cases_are_well_conditioned(name):
    o = PI.fit_reference(name)
    print(f"{name}: cond_2(N) up to {o['cond'].max():.3g}")
    assert o["ok"].all() and o["cond"].max() <= PI.COND_MAX


@pytest.mark.parametrize("name", sorted(PI.SINGULAR))
def test_singular_cases_are_singular_in_one_sample_alone(name):
    o = PI.fit_reference(name)
    bad = PI.SINGULAR[name]
    assert o["ok"].tolist() == [b != bad for b in range(len(o["ok"]))]
    assert np.isnan(o["amplitudes"][bad]).all() and np.isfinite(np.delete(o["amplitudes"], bad, axis=0)).all()
    assert np.delete(o["cond"], bad).max() <= PI.COND_MAX


@pytest.mark.parametrize("name", ["quad", "overlap", "single", "coincident"])
def test_envelope_gradient_is_the_gradient_through_the_solve(name):
    """The amplitudes maximise log_like, so the partial derivative at fixed amplitudes equals the total derivative."""
    o = PI.fit_reference(name)
    g, gx, gy = PI.envelope_gradient(name)
    good = o["ok"]
    for got, want, what in ((g, o["grad"], "grad"), (gx, o["grad_x"], "grad_x"), (gy, o["grad_y"], "grad_y")):
        scale = np.abs(want[good]).max()
        err = np.abs(got[good] - want[good]).max() / scale
        print(f"{name} {what}: {err:.3g}")
        assert err <= 1e-9, (name, what, err)


def test_abi_validation_without_gpu(native):
    lib = native.lib()
    names = ("gl_ptimg_workspace_bytes", "gl_ptimg_render", "gl_ptimg_render_bwd", "gl_ptimg_fit")
    for n in names:
        assert n in native.SYMBOLS and getattr(lib, n).argtypes == native.SYMBOLS[n][1]
    for m in ("ptimg_render", "ptimg_render_bwd", "ptimg_fit"):
        assert callable(getattr(native.Model, m))
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    xf = (ctypes.c_double * 6)(0, 0, 1, 0, 0, 1)
    assert lib.gl_ptimg_workspace_bytes(None, 2, 4) == 0
    for J in (0, 9, -1):
        assert lib.gl_ptimg_workspace_bytes(p, 2, J) == 0
    assert lib.gl_ptimg_workspace_bytes(p, 0, 4) == 0
    render = [p, p, p, p, 2, 4, xf, p, p, 4096, None]
    render_bwd = [p, p, p, p, 2, 4, xf, p, p, p, p, p, 4096, None]
    fit = [p, p, p, 2, 4, xf, p, p, 0, p, 0, 1, p, p, p, p, p, p, p, p, 4096, None]
    for fn, full, j_at, nulls in ((lib.gl_ptimg_render, render, 5, (0, 1, 2, 3, 6, 7, 8)),
                                  (lib.gl_ptimg_render_bwd, render_bwd, 5, (0, 1, 2, 3, 6, 7, 8, 9, 10, 11)),
                                  (lib.gl_ptimg_fit, fit, 4, (0, 1, 2, 5, 6, 7, 9, 12, 13, 14, 15, 16, 17, 18, 19))):
        for at in nulls:
            args = list(full)
            args[at] = None
            assert fn(*args) == -1, at
            assert b"null argument" in lib.gl_last_error()
        for J in (0, 9):
            args = list(full)
            args[j_at] = J
            assert fn(*args) == -1
            assert b"images per sample" in lib.gl_last_error()
    args = list(fit)  # the gradient outputs may be null when they are not asked for: the call then fails on the next check
    args[11], args[17], args[18], args[4] = 0, None, None, 9
    assert lib.gl_ptimg_fit(*args) == -1 and b"images per sample" in lib.gl_last_error()


def _prior(J):
    import math
    from gigalens_amd import prior as tfd
    mass = tfd.JointDistributionNamed(dict(theta_E=tfd.LogNormal(math.log(0.18), 0.1), e1=tfd.Normal(0, 0.1), e2=tfd.Normal(0, 0.1),
                                           center_x=tfd.Normal(0, 0.02), center_y=tfd.Normal(0, 0.02)))
    shear = tfd.JointDistributionNamed(dict(gamma1=tfd.Normal(0, 0.05), gamma2=tfd.Normal(0, 0.05)))
    src = tfd.JointDistributionNamed(dict(R_sersic=tfd.LogNormal(math.log(0.06), 0.15), n_sersic=tfd.Uniform(0.5, 4),
                                          center_x=tfd.Normal(0, 0.02), center_y=tfd.Normal(0, 0.02), Ie=tfd.LogNormal(math.log(10.0), 0.3)))
    images = [tfd.JointDistributionNamed(dict(x=tfd.Normal(0.1 * (k - 1), 0.02), y=tfd.Uniform(-0.3, 0.3))) for k in range(J)]
    return tfd.JointDistributionNamed(dict(lens_mass=tfd.JointDistributionSequential([mass, shear]),
                                           source_light=tfd.JointDistributionSequential([src]),
                                           point_images=tfd.JointDistributionSequential(images)))


def test_prob_model_host_logic():
    """The prior's point_images group round-trips through bij; log_prior is the prior's density of the constrained point plus the
    bijector's log-determinant: nothing ignored, nothing added."""
    from gigalens_amd.model import PointImageProbModel
    J = 3
    prior = _prior(J)
    obs, err = np.zeros((8, 8), dtype=np.float32), np.ones((8, 8), dtype=np.float32)
    pm = PointImageProbModel(prior, obs, err, source_plane_sigma=0.01)
    assert (pm.include_pixels, pm.include_positions, pm.n_position, pm.n_images) == (True, False, 0.0, J)
    x = prior.sample(5, seed=3)
    z = pm.bij.inverse(x)
    assert tuple(z.shape) == (5, 12 + 2 * J)
    back = pm.bij.forward(z)
    assert set(back) == {"lens_mass", "source_light", "point_images"} and len(back["point_images"]) == J
    for d0, d1 in zip(x["point_images"], back["point_images"]):
        for k in ("x", "y"):
            assert torch.allclose(torch.as_tensor(d0[k]), d1[k].cpu(), rtol=1e-5, atol=1e-6)
    lp = pm.log_prior(z).cpu().double()
    want = prior.log_prob(back).cpu().double() + pm.unconstraining_bij.forward_log_det_jacobian(pm.pack_bij.forward(z)).cpu().double()
    assert torch.allclose(lp, want, rtol=1e-5, atol=1e-4)
    # ... and it does depend on the positions: moving one image changes it by that leaf's density alone
    z2 = z.clone()
    k = [i for i, path in enumerate(__import__("gigalens_amd.prior", fromlist=["nest_paths"]).nest_paths(pm.pack_bij.template))
         if path == ("point_images", 0, "x")][0]
    z2[:, k] += 0.5
    d = (pm.log_prior(z2) - pm.log_prior(z)).cpu().double()
    x0, x1 = back["point_images"][0]["x"].cpu().double(), pm.bij.forward(z2)["point_images"][0]["x"].cpu().double()
    want_d = -0.5 * ((x1 + 0.1) ** 2 - (x0 + 0.1) ** 2) / 0.02 ** 2
    assert torch.allclose(d, want_d, rtol=1e-4, atol=1e-3)
    with pytest.raises(ValueError):
        PointImageProbModel(_prior(9), obs, err)
    with pytest.raises(ValueError):
        PointImageProbModel(prior, obs, err, source_plane_sigma=0.0)
    from gigalens_amd import prior as tfd
    with pytest.raises(ValueError):
        PointImageProbModel(tfd.JointDistributionNamed(dict(lens_mass=tfd.JointDistributionSequential([]))), obs, err)


def test_tie_term_restated():
    bx = torch.tensor([[0.01, 0.03, -0.01]], dtype=PI.F64)
    by = torch.tensor([[0.0, 0.02, 0.01]], dtype=PI.F64)
    s = 0.02
    want = sum(-0.5 * ((float(bx[0, j]) - 0.01) ** 2 + (float(by[0, j]) - 0.01) ** 2) / s ** 2 for j in range(3)) - 2 * np.log(2 * np.pi * s * s)
    assert abs(float(PI.tie(bx, by, s)[0]) - want) <= 1e-12
