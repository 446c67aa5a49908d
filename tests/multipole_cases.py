"""Models, inputs and float64 expectations of the multipole tests (tests/test_multipole_host.py, tests/test_gpu_multipole.py).

The reference of ``profiles.mass.Multipole`` is the formula itself, restated here with ``atan2`` / ``cos`` / ``sin`` (the kernels use
none of them: they raise the unit vector of the point to the m-th power, csrc/gl_multipole.h): with ``dx = x - center_x``,
``dy = y - center_y``, ``r = |(dx, dy)|``, ``phi = atan2(dy, dx)``, ``C = cos(m (phi - phi_m))``, ``S = sin(m (phi - phi_m))`` and
``k = a_m / (1 - m^2)``::

    psi     = k r C
    alpha_x = k (cos(phi) C + m sin(phi) S)
    alpha_y = k (sin(phi) C - m cos(phi) S)

and exact zeros at ``r = 0``.  It composes with the oracle's primitives (oracle/ref_torch.py, unchanged) the way
tests/interpmass_cases.py does: a ``RefSimulator`` whose ``beta`` sends a multipole to the restatement and every other lens to
``mass_deriv``; images, pixel statistics and the linear solve as tests/interp_cases.py forms them; Hessians and gradients by torch
autograd on that float64 composition.  Run with float32 tensors, the same code is the float32 yardstick of the value tolerances."""
import ctypes
import os
import subprocess
import types
from ctypes import POINTER, c_double, c_int

import numpy as np
import torch

from tests import helpers as H
from tests import interp_cases as IC

ROOT = IC.ROOT
F64, F32 = torch.float64, torch.float32
NAME = "MULTIPOLE"
_SO = None


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _polar(x, y, center_x, center_y):
    dt = x.dtype
    cx, cy = torch.as_tensor(center_x, dtype=dt), torch.as_tensor(center_y, dtype=dt)
    dx, dy = x - cx, y - cy
    z = (dx == 0) & (dy == 0)  # the centre itself: evaluated one unit away and replaced by exact zeros
    dxs = torch.where(z, torch.ones_like(dx), dx)
    r = torch.sqrt(dxs * dxs + dy * dy)
    return z, r, torch.atan2(dy, dxs)


def deflection(x, y, m, a_m, phi_m, center_x, center_y):
    """``(alpha_x, alpha_y)`` of the formula above at ``(x, y)`` (any shape; parameters broadcast on the last axis), in ``x.dtype``."""
    dt = x.dtype
    a, p = torch.as_tensor(a_m, dtype=dt), torch.as_tensor(phi_m, dtype=dt)
    z, _, phi = _polar(x, y, center_x, center_y)
    k = a / (1 - m * m)
    C, S = torch.cos(m * (phi - p)), torch.sin(m * (phi - p))
    ax = k * (torch.cos(phi) * C + m * torch.sin(phi) * S)
    ay = k * (torch.sin(phi) * C - m * torch.cos(phi) * S)
    return torch.where(z, torch.zeros_like(ax), ax), torch.where(z, torch.zeros_like(ay), ay)


def potential(x, y, m, a_m, phi_m, center_x, center_y):
    dt = x.dtype
    a, p = torch.as_tensor(a_m, dtype=dt), torch.as_tensor(phi_m, dtype=dt)
    z, r, phi = _polar(x, y, center_x, center_y)
    psi = a / (1 - m * m) * r * torch.cos(m * (phi - p))
    return torch.where(z, torch.zeros_like(psi), psi)


def hessian_closed(x, y, m, a_m, phi_m, center_x, center_y):
    """``(f_xx, f_xy, f_yx, f_yy) = (a_m C / r) t t^T`` with ``t = (-sin phi, cos phi)`` (away from the centre)."""
    dt = x.dtype
    a, p = torch.as_tensor(a_m, dtype=dt), torch.as_tensor(phi_m, dtype=dt)
    _, r, phi = _polar(x, y, center_x, center_y)
    w = a * torch.cos(m * (phi - p)) / r
    tx, ty = -torch.sin(phi), torch.cos(phi)
    return w * tx * tx, w * tx * ty, w * ty * tx, w * ty * ty


def lens_deriv(lens, x, y, **kw):
    from oracle import ref_torch as ref
    if lens.name == NAME:
        return deflection(x, y, lens.m, **kw)
    return ref.mass_deriv(lens, x, y, **kw)


def lens_potential(lens, x, y, **kw):
    """psi of one lens: the multipole's closed form; the others from the oracle's deflection -- SIS and SIE are homogeneous of
    degree 1 and the EPL of degree 3 - gamma about their centres (Euler: psi = x' . alpha / degree), the shear is quadratic."""
    if lens.name == NAME:
        return potential(x, y, lens.m, **kw)
    fx, fy = lens_deriv(lens, x, y, **kw)
    if lens.name == "SHEAR":
        return 0.5 * (x * fx + y * fy)
    deg = {"SIS": 1.0, "SIE": 1.0, "EPL": None}[lens.name]
    if deg is None:
        deg = 3.0 - kw["gamma"]
    return ((x - kw["center_x"]) * fx + (y - kw["center_y"]) * fy) / deg


def _beta(self, x, y, lens_params):
    mp = getattr(self.phys_model, "multiplane", None)
    if mp is not None:  # lens planes: the trace below to the plane of the (one) source
        bx, by, _ = trace(self.phys_model, mp, lens_params, x, y, mp.source_scales[:, 0])
        return bx, by
    bx, by = x, y
    for lens, p in zip(self.phys_model.lenses, lens_params):
        fx, fy = lens_deriv(lens, x, y, **p)
        bx, by = bx - fx, by - fy
    return bx, by


def ref_sim(wl, bs, dtype=F64, psf=None, grid_shift=None):
    """The oracle's simulator with ``beta`` replaced by the sum above."""
    rs = IC.ref_sim(wl, bs, dtype, psf, grid_shift)
    rs.beta = types.MethodType(_beta, rs)
    return rs


def lens_dicts(phys, rows):
    k, out = 0, []
    for lens in phys.lenses:
        out.append({n: rows[:, k + i] for i, n in enumerate(lens.params)})
        k += len(lens.params)
    return out


def maps_of(phys, rows, xs, ys):
    """beta, the Hessian (autograd of the deflection) and psi at ``xs, ys`` [n, B] (requiring grad) for lens rows [B, P_lens]."""
    ax, ay, psi = 0, 0, 0
    for lens, p in zip(phys.lenses, lens_dicts(phys, rows)):
        fx, fy = lens_deriv(lens, xs, ys, **p)
        ax, ay = ax + fx, ay + fy
        psi = psi + lens_potential(lens, xs, ys, **p)
    fxx, fxy = torch.autograd.grad(ax.sum(), [xs, ys], create_graph=True)
    fyx, fyy = torch.autograd.grad(ay.sum(), [xs, ys], create_graph=True)
    return xs - ax, ys - ay, (fxx, fxy, fyx, fyy), psi


def _pts(v, dtype, B):
    return torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype).reshape(-1, 1).repeat(1, B)


def lens_maps(phys, packed_lens, x, y, dtype=F64):
    """``[7, n_pts, B]``: beta_x, beta_y, f_xx, f_xy, f_yx, f_yy, psi at the points ``(x, y)`` ([n_pts]) for the lens rows [B, P_lens]."""
    B = packed_lens.shape[0]
    xs, ys = _pts(x, dtype, B).requires_grad_(True), _pts(y, dtype, B).requires_grad_(True)
    bx, by, h, psi = maps_of(phys, packed_lens.to(dtype), xs, ys)
    return torch.stack([bx, by, *h, psi]).detach()


def solve_images(phys, row, src, radius=1.0, n_seeds=24, iters=60):
    """The images of the source ``src`` behind the one-plane lens ``row`` [P_lens]: float64 Newton on the lens equation of this
    composition from ``n_seeds`` starts on the circle of ``radius``; the distinct converged roots, sorted by angle, as float32."""
    ang = 2 * np.pi * (np.arange(n_seeds) + 0.25) / n_seeds
    x, y = radius * np.cos(ang), radius * np.sin(ang)
    r64 = torch.as_tensor(np.asarray(row, dtype=np.float64))[None, :]
    for _ in range(iters):
        m = lens_maps(phys, r64, x, y)[:, :, 0].numpy()
        rx, ry = m[0] - src[0], m[1] - src[1]
        a, b, c, d = 1 - m[2], -m[3], -m[4], 1 - m[5]
        det = a * d - b * c
        dx, dy = -(d * rx - b * ry) / det, -(-c * rx + a * ry) / det
        step = np.minimum(1.0, 0.3 / np.maximum(np.hypot(dx, dy), 1e-30))
        x, y = x + step * dx, y + step * dy
    m = lens_maps(phys, r64, x, y)[:, :, 0].numpy()
    ok = (np.hypot(m[0] - src[0], m[1] - src[1]) < 1e-6) & (np.hypot(x, y) > 0.2)  # (lens_maps holds its points in float32)
    roots = []
    for xi, yi in zip(x[ok], y[ok]):
        if all(np.hypot(xi - u, yi - v) > 1e-4 for u, v in roots):
            roots.append((xi, yi))
    roots.sort(key=lambda p: np.arctan2(p[1], p[0]))
    return np.float32([p[0] for p in roots]), np.float32([p[1] for p in roots])


def point_family(phys, rows, src=(0.06, -0.04)):
    """One image family for the point likelihoods: the images of ``src`` behind the MEAN of the rows (float32) -- no sample sits at
    the optimum of the position term, where its gradient would be rounding alone --, position errors, fluxes ``3 |mu_j| PATTERN_j``
    with 5 % errors and arrival times ``-100 phi_j PATTERN_j`` of row 0 (the data of flux_cases / tdelay_cases)."""
    fx, fy = solve_images(phys, rows.double().mean(dim=0).numpy(), src)
    k = fx.size
    fam = dict(x=fx, y=fy, ex=np.full(k, 0.01, np.float32), ey=np.full(k, 0.0125, np.float32), T=np.ones(1))
    m = lens_maps(phys, rows[:1].double(), fx, fy)[:, :, 0].numpy()
    det = (1 - m[2]) * (1 - m[5]) - m[3] * m[4]
    fam["flux"] = (3.0 / np.abs(det) * np.asarray([1.12, 0.9, 1.05, 0.85, 1.2, 1.0][:k])).astype(np.float32)
    fam["flux_err"] = (np.float32(0.05) * fam["flux"]).astype(np.float32)
    phi0 = fermat(phys, lens_dicts(phys, rows[:1].double()), fam, 1)[:, 0].numpy()
    fam["delay"] = (-100.0 * phi0 * np.asarray([1.02, 0.97, 1.01, 0.99, 1.03, 1.0][:k])).astype(np.float32)
    fam["delay_err"] = np.asarray([1.0, 0.8, 1.2, 0.9, 1.1, 1.0][:k], dtype=np.float32)
    return fam


def trace(phys, mp, lp, x, y, T):
    """``mp_positions_cases.trace`` on this composition: ``(beta_x, beta_y, [A_xx, A_xy, A_yx, A_yy])`` of the target with couplings
    ``T`` for rays leaving the observer at ``x, y`` ([n, B]); ``mp`` None: one plane, ``T`` its deflection scale."""
    dt = x.dtype
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    K = 1 if mp is None else mp.K
    C = None if mp is None else torch.as_tensor(np.asarray(mp.lens_scales, dtype=np.float32)).to(dt)
    Tt = torch.as_tensor(np.asarray(T, dtype=np.float32)).to(dt).reshape(-1)
    a, G = [], []
    for j in range(K):
        if float(Tt[j]) == 0.0:
            break
        xj, yj, D = x, y, [one, zero, zero, one]
        for i in range(j):
            xj, yj = xj - C[i, j] * a[i][0], yj - C[i, j] * a[i][1]
            D = [d - C[i, j] * g for d, g in zip(D, G[i])]
        if not xj.requires_grad:  # (autograd differentiates a deflection with respect to the position it is given)
            xj, yj = xj.clone().requires_grad_(True), yj.clone().requires_grad_(True)
        ax, ay, g = zero, zero, [zero, zero, zero, zero]
        for l, lens in enumerate(phys.lenses):
            if mp is None or int(mp.plane_of_lens[l]) == j:
                fx, fy = lens_deriv(lens, xj, yj, **lp[l])
                # the Hessian at the ray, as a function of the parameters: closed form for the multipole, autograd otherwise
                if lens.name == NAME:
                    hxx, hxy, hyx, hyy = hessian_closed(xj, yj, lens.m, **lp[l])
                else:
                    hxx, hxy = torch.autograd.grad(fx.sum(), [xj, yj], create_graph=True)
                    hyx, hyy = torch.autograd.grad(fy.sum(), [xj, yj], create_graph=True)
                ax, ay = ax + fx, ay + fy
                g = [g[0] + hxx * D[0] + hxy * D[2], g[1] + hxx * D[1] + hxy * D[3],
                     g[2] + hyx * D[0] + hyy * D[2], g[3] + hyx * D[1] + hyy * D[3]]
        a.append((ax, ay))
        G.append(g)
    bx, by, A = x, y, [one, zero, zero, one]
    for i in range(len(a)):
        bx, by = bx - Tt[i] * a[i][0], by - Tt[i] * a[i][1]
        A = [v - Tt[i] * g for v, g in zip(A, G[i])]
    return bx, by, A


def stats_positions(phys, mp, rows, fams, dtype=F64):
    """tf/model.py:103-124 per family on ``trace``: ``(log_like [B], d log_like / d rows)``; ``fams`` = ``[dict(x, y, ex, ey, T)]``."""
    r = rows.detach().to(dtype).clone().requires_grad_(True)
    B, lp, ll = r.shape[0], lens_dicts(phys, r), 0.0
    for fam in fams:
        bx, by, A = trace(phys, mp, lp, _pts(fam["x"], dtype, B), _pts(fam["y"], dtype, B), fam["T"])
        mag = 1.0 / (A[0] * A[3] - A[1] * A[2])
        e_x, e_y = _pts(fam["ex"], dtype, 1) / mag, _pts(fam["ey"], dtype, 1) / mag
        chi2 = (((bx - bx.mean(0, keepdim=True)) / e_x) ** 2 + ((by - by.mean(0, keepdim=True)) / e_y) ** 2).sum(0)
        ll = ll - 0.5 * (chi2 + (torch.log(2 * np.pi * e_x ** 2) + torch.log(2 * np.pi * e_y ** 2)).sum(0))
    (g,) = torch.autograd.grad(ll.sum(), r)
    return ll.detach().double().numpy(), g.double().numpy()


def stats_fluxes(phys, rows, fams, dtype=F64):
    """``flux_cases.family_term`` on the determinants of this composition (one plane): ``(log_like [B], gradient)``."""
    from tests import flux_cases as FC
    r = rows.detach().to(dtype).clone().requires_grad_(True)
    B, lp, ll = r.shape[0], lens_dicts(phys, r), 0.0
    for fam in fams:
        _, _, A = trace(phys, None, lp, _pts(fam["x"], dtype, B), _pts(fam["y"], dtype, B), fam["T"])
        ll = ll + FC.family_term(A[0] * A[3] - A[1] * A[2], fam["flux"], fam["flux_err"])[0]
    (g,) = torch.autograd.grad(ll.sum(), r)
    return ll.detach().double().numpy(), g.double().numpy()


def fermat(phys, lp, fam, B, dtype=F64):
    """``phi [J, B] = |theta - mean beta|^2 / 2 - psi(theta)`` of the images of one family (one plane, the reference plane)."""
    cx, cy = _pts(fam["x"], dtype, B), _pts(fam["y"], dtype, B)
    bx, by, psi = cx, cy, 0.0
    for lens, p in zip(phys.lenses, lp):
        fx, fy = lens_deriv(lens, cx, cy, **p)
        bx, by, psi = bx - fx, by - fy, psi + lens_potential(lens, cx, cy, **p)
    return 0.5 * ((cx - bx.mean(0, keepdim=True)) ** 2 + (cy - by.mean(0, keepdim=True)) ** 2) - psi


def stats_time_delays(phys, rows, fams, dtype=F64):
    """``tdelay_cases.family_term`` (profiled scale) on the Fermat potentials of this composition: ``(log_like [B], gradient)``."""
    from tests import tdelay_cases as TC
    r = rows.detach().to(dtype).clone().requires_grad_(True)
    B, lp, ll = r.shape[0], lens_dicts(phys, r), 0.0
    for fam in fams:
        ll = ll + TC.family_term(fermat(phys, lp, fam, B, dtype), fam["delay"], fam["delay_err"], np.nan)[0]
    (g,) = torch.autograd.grad(ll.sum(), r)
    return ll.detach().double().numpy(), g.double().numpy()


def loglike_and_grad(wl, packed, obs, dtype=F64, psf=None, grid_shift=None, mask=None):
    """``(log_like, red_chi2, d log_like / d packed, image)`` of the composition in ``dtype`` (numpy arrays).  ``mask`` [H, W] bool:
    pixels left out of the statistics (the image keeps them)."""
    rs = ref_sim(wl, packed.shape[0], dtype, psf, grid_shift)
    if mask is not None:
        rs.img_region = rs.img_region * torch.as_tensor(~mask).to(rs.img_region.dtype)
    p = packed.detach().cpu().to(dtype).clone().requires_grad_(True)
    ll, red, im = IC.expected_stats(rs, H.struct_from_packed(wl.phys_model, p), obs, wl.background_rms, wl.exp_time)
    (g,) = torch.autograd.grad(ll.sum(), p)
    return ll.detach().numpy(), red.detach().numpy(), g.numpy(), im.detach().numpy()


def image_vjp(wl, packed, cot, dtype=F64, psf=None, grid_shift=None):
    """``(image, d sum(image * cot) / d packed)`` of the composition."""
    rs = ref_sim(wl, packed.shape[0], dtype, psf, grid_shift)
    p = packed.detach().cpu().to(dtype).clone().requires_grad_(True)
    im = IC.expected_image(rs, H.struct_from_packed(wl.phys_model, p))
    (g,) = torch.autograd.grad((im * torch.as_tensor(cot).to(dtype)).sum(), p)
    return im.detach().numpy(), g.numpy()


def lstsq(wl, packed, obs, err, dtype=F64, psf=None):
    """``(coefficients [B, depth], image)`` of ``interp_cases.expected_lstsq`` on this composition."""
    rs = ref_sim(wl, packed.shape[0], dtype, psf)
    co, im = IC.expected_lstsq(rs, H.struct_from_packed(wl.phys_model, packed.detach().cpu().to(dtype)), obs, err)
    return co.detach().numpy(), im.detach().numpy()


def conditioning_bound(wl, grad_fn, g_o, S, seed=0):
    """``interp_cases.conditioning_bound`` (float32 rounding of the grid alone) measured on THIS composition."""
    return IC.conditioning_bound(wl, grad_fn, g_o, S, seed)


def observation(wl, packed, psf=None, seed=4):
    """A noisy float32 image of the model's own scale: the float64 expectation of the first row plus noise of the likelihood's rms."""
    rs = ref_sim(wl, 1, F64, psf)
    img = IC.expected_image(rs, H.struct_from_packed(wl.phys_model, packed[:1].double()))[0].detach().numpy()
    r = np.random.default_rng(seed)
    return (img + r.normal(size=img.shape) * np.sqrt(wl.background_rms ** 2 + np.clip(img, 0, None) / wl.exp_time)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = {"33x31": ((33, 31), 0.1), "16x16": ((16, 16), 0.2)}  # (num_pix, delta_pix): both fields reach +-1.6 arcsec, theta_E ~ 1
A_MAX = 0.05


def lenses_of(model, m=4):
    from gigalens_amd.profiles.mass import Multipole
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    return {"ESM": lambda: [EPL(), Shear(), Multipole(m)], "SMM": lambda: [SIE(), Multipole(3), Multipole(4)],
            "EM": lambda: [EPL(), Multipole(m)], "SM": lambda: [SIS(), Multipole(m)], "M": lambda: [Multipole(m)]}[model]()


def lens_row(lenses, r, node=None):
    """One row of lens parameters: theta_E ~ 1, |a_m| <= 0.05 of either sign, |phi_m| up to beyond pi, every centre at an irrational
    offset of a few hundredths of an arcsec (``node``: the multipoles' centre, exactly, instead)."""
    row = []
    for lens in lenses:
        c = [float(np.sqrt(2.0) * r.uniform(-0.04, 0.04)), float(np.sqrt(3.0) * r.uniform(-0.04, 0.04))]
        if lens.name == NAME:
            a = r.uniform(0.015, A_MAX) * (1 if r.uniform() < 0.6 else -1)
            row += [a, r.uniform(-4.0, 4.0)] + (c if node is None else list(node))
        elif lens.name == "EPL":
            row += [r.uniform(0.95, 1.1), r.uniform(1.8, 2.2), r.normal(0, 0.08), r.normal(0, 0.08)] + c
        elif lens.name == "SIE":
            row += [r.uniform(0.95, 1.1), r.normal(0, 0.08), r.normal(0, 0.08)] + c
        elif lens.name == "SIS":
            row += [r.uniform(0.95, 1.1)] + c
        else:
            row += [r.normal(0, 0.03), r.normal(0, 0.03)]
    return row


def case(model, grid, B=3, m=4, supersample=1, node=None, use_lstsq=False, seed=0):
    """``(workload, packed rows [B, P] float32 on the CPU)`` of one parity case.  Models: "ESM" EPL + Shear + Multipole(m) |
    SersicEllipse, "SMM" SIE + Multipole(3) + Multipole(4) | Sersic + Shapelets(n_max 4)."""
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.light.shapelets import Shapelets
    from gigalens_amd.simulator import SimulatorConfig
    n, delta = GRIDS[grid]
    lenses = lenses_of(model, m)
    if model == "ESM":
        sources = [SersicEllipse(use_lstsq=use_lstsq)]
    else:
        sources = [Sersic(use_lstsq=use_lstsq), Shapelets(4, use_lstsq=use_lstsq, interpolate=False)]
    phys = PhysicalModel(lenses, [], sources)
    cfg = SimulatorConfig(delta_pix=delta, num_pix=n, supersample=supersample)
    wl = workloads.Workload(f"MP-{model}{m}-{grid}-B{B}", phys, None, cfg, B)
    r = np.random.default_rng(101 + seed + sum(map(ord, model)) + 7 * m + n[0] + B)
    rows = []
    for b in range(B):
        row = lens_row(lenses, r, node)
        for src in sources:
            sc = [r.normal(0, 0.08), r.normal(0, 0.08)]
            if src.name == "SHAPELETS":
                row += [r.uniform(0.12, 0.18)] + sc + list(2.0 * r.normal(size=src.n_layers) / (1 + np.arange(src.n_layers)))
            elif src.name == "SERSIC_ELLIPSE":
                row += [r.uniform(0.2, 0.3), r.uniform(1.0, 2.5), r.normal(0, 0.1), r.normal(0, 0.1)] + sc + [30.0]
            else:
                row += [r.uniform(0.2, 0.3), r.uniform(1.0, 2.5)] + sc + [30.0]
        rows.append(row)
    return wl, torch.tensor(rows, dtype=torch.float32)


# name -> (model, grid, B, m, supersample, PSF): both grids, B in {1, 3, 65}, m in {2, 3, 4, 8}
PSF = IC.gauss_psf(3, 0.8)
PIXEL_CASES = {
    "ESM4-33x31-B3": ("ESM", "33x31", 3, 4, 1, None),
    "ESM2-16x16-B1": ("ESM", "16x16", 1, 2, 1, None),
    "ESM3-16x16-B65": ("ESM", "16x16", 65, 3, 1, None),
    "ESM8-33x31-B3-ss2-psf": ("ESM", "33x31", 3, 8, 2, PSF),
    "SMM-33x31-B3": ("SMM", "33x31", 3, 4, 1, None),
    "SMM-16x16-B65": ("SMM", "16x16", 65, 4, 1, None),
}
COND_CAP = 0.02  # share of a case's gradient elements that may pass through the conditioning bound alone
Z_PLANES = (0.5, 0.5, 1.0, 1.0)  # "planes": EPL + Shear in front, SIE + Multipole(4) behind, the source at Z_SOURCE
Z_SOURCE = 3.0


def planes_case():
    """Two lens planes, the multipole on the far one beside an SIE: ``(workload, rows [3, P], MultiPlane)`` on the 16 x 16 grid."""
    from gigalens_amd import workloads
    from gigalens_amd.cosmology import MultiPlane
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass import Multipole
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    n, delta = GRIDS["16x16"]
    lenses = [EPL(), Shear(), SIE(), Multipole(4)]
    mp = MultiPlane(list(Z_PLANES), [Z_SOURCE], Z_SOURCE)
    phys = PhysicalModel(lenses, [], [Sersic()], multiplane=mp)
    wl = workloads.Workload("MP-planes", phys, None, SimulatorConfig(delta_pix=delta, num_pix=n), 3)
    r = np.random.default_rng(77)
    rows = []
    for b in range(3):
        row = lens_row(lenses, r)
        row[0] *= 0.7   # two deflectors share the field: theta_E 0.7 in front,
        row[8] *= 0.5   # 0.5 behind
        rows.append(row + [r.uniform(0.2, 0.3), r.uniform(1.0, 2.5), r.normal(0, 0.08), r.normal(0, 0.08), 30.0])
    return wl, torch.tensor(rows, dtype=torch.float32), mp


def pixel_data(name):
    """Everything the pixel tests of case ``name`` compare against, computed once: workload, rows, observation, cotangent, the float64
    log-likelihood / reduced chi2 / gradient / image / image-VJP gradient and the float32 restatement's errors ``im_yard`` (of max
    |image|) and ``ll_yard`` (relative).  ``node``: ESM4 on 33 x 31 with the multipole centred exactly on the pixel node (0, 0), that
    pixel masked out of the statistics and given a zero cotangent.  ``planes``: ``planes_case``."""
    mask = mp = None
    if name == "planes":
        wl, packed, mp = planes_case()
        psf = None
    elif name == "node":
        wl, packed = case("ESM", "33x31", 3, 4, node=(0.0, 0.0))
        psf = None
    else:
        model, grid, B, m, ss, psf = PIXEL_CASES[name]
        wl, packed = case(model, grid, B, m, supersample=ss)
    if packed.shape[0] == 1:
        # one row: observed from OTHER rows of the same model, or the row would sit at the optimum of its own observation, where
        # the gradient is the noise's and a column's scale (its one element) says nothing about the model
        obs = observation(wl, case(model, grid, 3, m, supersample=ss, seed=1)[1][1:2], psf)
    else:
        obs = observation(wl, packed, psf)
    r = np.random.default_rng(3)
    cot = r.normal(size=(packed.shape[0],) + obs.shape).astype(np.float32)
    if name == "node":
        rs = ref_sim(wl, 1)
        on = ((rs.img_X[:, 0] == 0) & (rs.img_Y[:, 0] == 0)).numpy()
        assert on.sum() == 1
        mask = np.zeros(obs.shape, dtype=bool)
        mask[rs.region[on, 0], rs.region[on, 1]] = True
        cot[:, mask] = 0.0
    ll, red, g, im = loglike_and_grad(wl, packed, obs, psf=psf, mask=mask)
    ll32, _, g32, im32 = loglike_and_grad(wl, packed, obs, dtype=F32, psf=psf, mask=mask)
    _, g_img = image_vjp(wl, packed, cot, psf=psf)
    _, g_img32 = image_vjp(wl, packed, cot, dtype=F32, psf=psf)
    keep = slice(None) if mask is None else ~mask
    return dict(wl=wl, packed=packed, obs=obs, psf=psf, cot=cot, mask=mask, mp=mp, ll=ll, red=red, g=g, im=im, g_img=g_img, g32=g32,
                g_img32=g_img32, im_yard=np.abs(im32 - im)[:, keep].max() / np.abs(im).max(),
                ll_yard=(np.abs(ll32 - ll) / np.maximum(np.abs(ll), 1.0)).max())


# ---------------------------------------------------------------------------------------------------------------------
# host build of the kernels' templates (tests/hostmath/multipole_host.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def _host_sources():
    src = os.path.join(ROOT, "tests", "hostmath", "multipole_host.cpp")
    csrc = os.path.join(ROOT, "gigalens_amd", "csrc")
    return src, [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h") and not f.endswith(".hip.h")]


def host():
    """ctypes handle of tests/hostmath/multipole_host.cpp compiled with g++ (rebuilt when it or a csrc header is newer)."""
    global _SO
    if _SO is None:
        src, deps = _host_sources()
        so = os.path.join(ROOT, "tests", "hostmath", "libmultipole_host.so")
        if IC._stale(so, deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        _SO = ctypes.CDLL(so)
        dp = POINTER(c_double)
        _SO.multipole_d.argtypes = [c_int, dp, c_int] + [dp] * 10
        _SO.multipole_jet_d.argtypes = [c_int, dp, c_int, dp, dp, dp]
    return _SO


def host_program():
    """Path of the same source built as its stand-alone program with the host sanitizers (tests/hostmath/multipole_host_check)."""
    src, deps = _host_sources()
    exe = os.path.join(ROOT, "tests", "hostmath", "multipole_host_check")
    if IC._stale(exe, deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    return exe


def _dp(a):
    return a.ctypes.data_as(POINTER(c_double))


def host_eval(m, p, x, y, gx, gy):
    """The float64 instantiation of multipole_prep / fwd / pot / vjp / finalize:
    ``(ax [n], ay [n], psi [n], grad [4], gpx [n], gpy [n])``."""
    x, y, gx, gy = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y, gx, gy))
    pp = np.ascontiguousarray(p, dtype=np.float64)
    ax, ay, psi, gpx, gpy = (np.empty_like(x) for _ in range(5))
    grad = np.empty(4)
    host().multipole_d(int(m), _dp(pp), x.size, _dp(x), _dp(y), _dp(gx), _dp(gy), _dp(ax), _dp(ay), _dp(psi), _dp(grad), _dp(gpx), _dp(gpy))
    return ax, ay, psi, grad, gpx, gpy


def host_jet(m, p, x, y):
    """``[9, n]`` = alpha_x, alpha_y, f_xx, f_xy, f_yx, f_yy (Dual<double, 2> through multipole_fwd), psi, d psi / dx, d psi / dy
    (through multipole_pot)."""
    x, y = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y))
    pp = np.ascontiguousarray(p, dtype=np.float64)
    out = np.empty((9, x.size))
    host().multipole_jet_d(int(m), _dp(pp), x.size, _dp(x), _dp(y), _dp(out))
    return out
