"""CPU-side checks of the Hessian VJP and the weak-lensing shear likelihood (gl_lens_hessian_vjp, gl_shear_loglike): the symbols are
exported and bound, the methods exist, the argument validation answers without a device, ``ShearCatalogue`` validates its
arrays; the float64 restatement of tests/shear_cases.py is pinned against the SIS closed form, a finite difference and the
continuity of g^ across |g| = 1; and every draw and case of the GPU tests meets its selection conditions and keeps 4 x its float32
yardstick under its cap -- on the reference alone."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mp_positions_cases as PC
from tests import shear_cases as SC


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


NAMES = ("gl_lens_hessian_vjp", "gl_lens_hessian_vjp_workspace_bytes", "gl_shear_loglike", "gl_shear_loglike_workspace_bytes")


def test_symbols_exported_and_bound(native):
    lib = native.lib()
    for name in NAMES:
        assert name in native.SYMBOLS
        assert getattr(lib, name).argtypes == native.SYMBOLS[name][1]
    assert callable(native.Model.lens_hessian_vjp) and callable(native.Model.shear_loglike)
    from gigalens_amd import model
    from gigalens_amd.simulator import LensSimulator
    for meth in ("hessian_vjp", "reduced_shear", "shear_log_like_and_grad"):
        assert callable(getattr(LensSimulator, meth))
    for meth in ("log_prob", "log_prob_and_grad", "log_prior", "init_centroids"):
        assert callable(getattr(model.WeakLensingProbModel, meth))
    assert callable(model.ShearCatalogue)


def test_argument_validation_without_gpu(native):
    lib = native.lib()
    GL_EINVAL = -1
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    for args in ((None, 4, 100), (p, 0, 100), (p, -1, 100), (p, 4, 0), (p, 4, -5)):
        assert lib.gl_lens_hessian_vjp_workspace_bytes(*args) == 0, args
        for want_grad in (0, 1):
            assert lib.gl_shear_loglike_workspace_bytes(*args, want_grad) == 0, args
    full = [p, p, 4, p, p, 100, 1, p, p, p, 4096, None]
    for null_at in (0, 1, 3, 4, 7, 8, 9):  # model, params, x, y, cot, grad_params, workspace
        args = list(full)
        args[null_at] = None
        assert lib.gl_lens_hessian_vjp(*args) == GL_EINVAL, null_at
        assert b"null argument" in lib.gl_last_error()
    for B, n_pts in ((0, 100), (-3, 100), (4, 0), (4, -1)):
        args = list(full)
        args[2], args[5] = B, n_pts
        assert lib.gl_lens_hessian_vjp(*args) == GL_EINVAL, (B, n_pts)
        assert b"must be positive" in lib.gl_last_error()
    full = [p, p, 4, p, p, p, p, p, p, 100, p, p, p, p, p, 4096, None]
    for null_at in (0, 1, 3, 4, 6, 7, 8, 10, 11, 14):  # model, params, x, y, e1, e2, sigma, ll, chi2, workspace
        args = list(full)
        args[null_at] = None
        assert lib.gl_shear_loglike(*args) == GL_EINVAL, null_at
        assert b"null argument" in lib.gl_last_error()
    for B, n_gal in ((0, 100), (-3, 100), (4, 0), (4, -1)):
        args = list(full)
        args[2], args[9] = B, n_gal
        assert lib.gl_shear_loglike(*args) == GL_EINVAL, (B, n_gal)
        assert b"must be positive" in lib.gl_last_error()


def test_shear_catalogue_validation():
    from gigalens_amd.model import ShearCatalogue
    x, y, e = [0.5, 1.0, -2.0], [1.0, 0.0, 0.3], [0.1, 0.0, -0.2]
    c = ShearCatalogue(x, y, e, e, 0.3)
    assert c.n == len(c) == 3 and c.scales is None
    for a in (c.x, c.y, c.e1, c.e2, c.sigma):
        assert a.dtype == np.float32 and a.shape == (3,)
    assert np.all(c.sigma == np.float32(0.3))
    c = ShearCatalogue(x, y, e, e, [0.3, 0.2, 0.1], scales=0.8)
    assert c.scales.dtype == np.float32 and np.all(c.scales == np.float32(0.8))
    bad = [dict(y=y[:2]), dict(e1=e[:1]), dict(e2=[e]), dict(sigma=[0.3, 0.2]), dict(scales=[1.0, 1.0]),
           dict(x=[0.5, np.nan, 1.0]), dict(y=[np.inf, 0.0, 1.0]), dict(e1=[0.0, 0.0, np.nan]), dict(e2=[0.0, -np.inf, 0.0]),
           dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=[0.3, np.nan, 0.3]), dict(sigma=np.inf), dict(sigma=None),
           dict(scales=0.0), dict(scales=[1.0, -1.0, 1.0]), dict(scales=[1.0, np.inf, 1.0]), dict(x=[])]
    for kw in bad:
        args = dict(x=x, y=y, e1=e, e2=e, sigma=0.3)
        args.update(kw)
        with pytest.raises(ValueError):
            ShearCatalogue(**args)


# ---- the restatement ------------------------------------------------------------------------------------------------
def _sis(theta_E=1.3, cx=0.1, cy=-0.2):
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    return PhysicalModel([SIS()], [], []), np.array([[theta_E, cx, cy]], dtype=np.float64)


def test_restatement_matches_the_sis_closed_form():
    """kappa = theta_E / (2 r), |gamma| = kappa and tangential: g_t = kappa / (1 - kappa) outside the Einstein radius, 1/g* inside."""
    theta_E, cx, cy = 1.3, 0.1, -0.2
    phys, rows = _sis(theta_E, cx, cy)
    r = np.array([0.3, 0.55, 0.9, 1.2, 1.5, 2.5, 5.0])  # kappa > 1, 1/2 < kappa < 1, and the weak branch
    phi = np.linspace(0.2, 5.9, r.size)
    scale = np.float32(0.75)
    x, y = (cx + r * np.cos(phi)).astype(np.float32), (cy + r * np.sin(phi)).astype(np.float32)
    rr, ph = np.hypot(np.float64(x) - cx, np.float64(y) - cy), np.arctan2(np.float64(y) - cy, np.float64(x) - cx)
    kappa = np.float64(scale) * theta_E / (2 * rr)
    gt = np.where(kappa <= 0.5, kappa / (1 - kappa), (1 - kappa) / kappa)
    assert (kappa > 1).any() and ((kappa > 0.5) & (kappa < 1)).any() and (kappa < 0.5).any()
    _, lp = PC.leaf(dict(phys=phys), SC.F64, packed=rows)
    with torch.enable_grad():
        h1, h2, k, ng = SC.shear_fields(phys, lp, x, y, np.full(r.size, scale), SC.F64)
    np.testing.assert_allclose(k.detach().numpy()[:, 0], kappa, rtol=1e-12)
    np.testing.assert_allclose(ng.detach().numpy()[:, 0], kappa / np.abs(1 - kappa), rtol=1e-12)
    np.testing.assert_allclose(h1.detach().numpy()[:, 0], -gt * np.cos(2 * ph), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(h2.detach().numpy()[:, 0], -gt * np.sin(2 * ph), rtol=1e-11, atol=1e-13)


def test_reduced_shear_is_continuous_across_unit_modulus():
    theta_E = 1.3
    phys, rows = _sis(theta_E, 0.0, 0.0)
    _, lp = PC.leaf(dict(phys=phys), SC.F64, packed=rows)
    eps = 1e-9
    rr = torch.tensor([[theta_E * (1 - eps)], [theta_E * (1 + eps)]], dtype=SC.F64)  # |g| = 1 at r = theta_E for c = 1
    x, y = rr * np.cos(0.7), rr * np.sin(0.7)
    f = SC.hessian(phys, lp, x, y)
    # (shear_fields takes float32 points; the two sides of the branch need float64 ones)
    kappa, g1, g2 = (f[0] + f[3]) / 2, (f[0] - f[3]) / 2, f[1]
    r1, r2 = g1 / (1 - kappa), g2 / (1 - kappa)
    n2 = (r1 * r1 + r2 * r2).detach().numpy()[:, 0]
    assert n2[0] > 1 > n2[1]
    h = np.stack([(r1.detach().numpy()[:, 0]) / np.where(n2 > 1, n2, 1.0), (r2.detach().numpy()[:, 0]) / np.where(n2 > 1, n2, 1.0)])
    assert np.abs(h[:, 0] - h[:, 1]).max() <= 1e-7
    assert abs(np.hypot(*h[:, 0]) - 1) <= 1e-7


@pytest.mark.parametrize("name", ["epl_shear|sie", "dpis|sie"])
def test_autograd_gradient_matches_a_finite_difference(name):
    c, cat = SC.ll_case(name), SC.catalogue(name, 65)
    rows = np.asarray(c["rows"], dtype=np.float64)
    ref = SC.loglike_grad(c["phys"], rows, cat, SC.F64)
    h = 1e-6
    fd = np.zeros_like(ref["grad"])
    for k in range(rows.shape[1]):  # every sample's row at once: log_like[b] depends on row b alone
        up, dn = rows.copy(), rows.copy()
        up[:, k] += h
        dn[:, k] -= h
        fd[:, k] = (SC.loglike_grad(c["phys"], up, cat, SC.F64)["log_like"] - SC.loglike_grad(c["phys"], dn, cat, SC.F64)["log_like"]) / (2 * h)
    scale = np.abs(ref["grad"]).max(axis=0, keepdims=True)
    assert (np.abs(fd - ref["grad"]) / scale).max() <= 1e-6


# ---- the draws and cases of the GPU tests, on the reference alone ---------------------------------------------------------
@pytest.mark.parametrize("label", sorted(SC.DRAWS))
def test_vjp_draw_keeps_its_yardstick_under_the_cap(label):
    kind, rows, x, y, cot, ref = SC.vjp_data(label)
    _, _, r_min, _ = SC.DRAWS[label]
    if kind not in ("SHEAR", "catalogue"):
        kw = [SC.row_to_kwargs(kind, p) for p in rows]
        r = np.hypot(x - np.float32([k["center_x"] for k in kw])[None, :], y - np.float32([k["center_y"] for k in kw])[None, :])
        assert r.min() >= r_min - 1e-6
    assert np.all(cot != 0) and np.all(np.isfinite(cot))
    for n in SC.N_PTS:
        g64, yard = ref[n]
        assert np.all(np.isfinite(g64)), (label, n)
        print(f"hessian_vjp draw {label} n_pts={n}: float32 yardstick {yard:.3g}")
        assert 4 * yard <= SC.YARD_CAP, (label, n, yard)  # the draw, not the cap, is what changes if this fails


@pytest.mark.parametrize("name", SC.LL_CASES)
def test_likelihood_case_meets_its_conditions(name):
    for n in SC.N_GAL:
        c, cat, ref, yard = SC.ll_data(name, n)
        r, dg, dk, ng = SC.margins(c, cat["x"], cat["y"], cat["scales"])
        assert r.min() >= SC.MIN_R and dg.min() >= SC.MIN_G and dk.min() >= SC.MIN_K, (name, n)
        strong = int((ng > 1).any(axis=1).sum())
        print(f"shear case {name} N={n}: yardsticks {yard}; {strong} galaxies with |g| > 1 in a sample, "
              f"{int((ng > 1).all(axis=1).sum())} in all three")
        if n >= 64:
            assert strong >= 1, (name, n)
        assert all(np.all(np.isfinite(v)) for v in ref.values())
        assert np.all(cat["sigma"] > 0) and all(v.dtype == np.float32 and v.shape == (n,) for v in cat.values())
        assert 4 * yard["grad"] <= SC.GATE_CAP, (name, n, yard)
