"""Models, inputs and float64 expectations of the interpolated-light tests (tests/test_interp_host.py, tests/test_gpu_interp.py).

The reference of ``Interpolated`` is the formula itself, restated here with no table, no apron and no ``floor``: with
``dx = x - center_x``, ``dy = y - center_y``::

    u = ( dx cos(phi) + dy sin(phi)) / scale + (W - 1) / 2
    v = (-dx sin(phi) + dy cos(phi)) / scale + (H - 1) / 2
    I = amp * sum_j sum_i w(v - j) w(u - i) image[j, i]

as a dense contraction over every pixel of the (small) image, ``w`` the hat function or Keys' kernel written with ``|t|``.  It
composes with the oracle's existing primitives (oracle/ref_torch.py, unchanged) the way tests/multiplane_cases.py does:
``RefSimulator.beta`` ray-shoots, ``light_eval`` renders the parametric components, then NaN -> 0, ``psf_pool``, the conversion factor
and the formulas of ``stats_pixels``.  Gradients are torch autograd on that float64 composition (the derivative of ``|t|``-polynomials
almost everywhere).  Run with float32 tensors, the same code is the float32 yardstick of the value tolerances."""
import ctypes
import math
import os
import subprocess
from ctypes import POINTER, c_double, c_int

import numpy as np
import torch

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
_SO = None


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def weight(t, order):
    """``w(t)``: the hat function (order 1) or Keys' cubic convolution kernel with a = -1/2 (order 3)."""
    a = t.abs()
    zero = torch.zeros_like(a)
    if order == 1:
        return torch.where(a < 1, 1 - a, zero)
    inner = (1.5 * a - 2.5) * a * a + 1
    outer = ((-0.5 * a + 2.5) * a - 4) * a + 2
    return torch.where(a <= 1, inner, torch.where(a < 2, outer, zero))


def pixel_coords(x, y, shape, center_x, center_y, phi, scale):
    """``(u, v)`` of the points ``(x, y)``; parameters broadcast on the last axis."""
    Hh, Ww = shape
    cx, cy, phi, scale = (torch.as_tensor(t, dtype=x.dtype) for t in (center_x, center_y, phi, scale))
    dx, dy = x - cx, y - cy
    c, s = torch.cos(phi), torch.sin(phi)
    return (dx * c + dy * s) / scale + (Ww - 1) / 2, (-dx * s + dy * c) / scale + (Hh - 1) / 2


def interp_light(x, y, image, order, center_x, center_y, phi, scale, amp):
    """Surface brightness of the formula above at ``(x, y)`` (any shape; parameters broadcast on the last axis), in ``x.dtype``."""
    img = torch.as_tensor(np.asarray(image, dtype=np.float32)).to(x.dtype)
    Hh, Ww = img.shape
    u, v = pixel_coords(x, y, (Hh, Ww), center_x, center_y, phi, scale)
    wu = weight(u[..., None] - torch.arange(Ww, dtype=x.dtype), order)
    wv = weight(v[..., None] - torch.arange(Hh, dtype=x.dtype), order)
    return torch.as_tensor(amp, dtype=x.dtype) * torch.einsum("...j,ji,...i->...", wv, img, wu)


def light_any(profile, x, y, unit=False, **kw):
    """``light`` of any light profile: the restatement for ``Interpolated``, the oracle's ``light_eval`` / ``light_basis`` otherwise.
    ``unit``: the unit-amplitude basis stack ``(depth, ...)`` of a ``use_lstsq`` profile."""
    from oracle import ref_torch as ref
    if profile.name == "INTERPOL":
        kw = dict(kw)
        amp = 1.0 if unit else kw.pop("amp")
        kw.pop("amp", None)
        out = interp_light(x, y, profile.image, profile.order, amp=amp, **kw)
        return out[None] if unit else out
    return ref.light_basis(profile, x, y, **kw) if unit else ref.light_eval(profile, x, y, **kw)


def expected_image(rs, params, stacked=False):
    """The image of ``RefSimulator.simulate`` (tf/simulator.py:109-156) with ``light_any`` as the light evaluator and source s at
    ``theta - c_s sum alpha`` (``PhysicalModel.source_light_scales``).  ``stacked``: the basis stack ``(bs, H, W, depth)``."""
    from oracle import ref_torch as ref
    pm = rs.phys_model
    scales = getattr(pm, "source_light_scales", np.ones(len(pm.source_light)))
    b1x, b1y = rs.beta(rs.img_X, rs.img_Y, params["lens_mass"])
    ax, ay = rs.img_X - b1x, rs.img_Y - b1y
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    rr, cc = torch.from_numpy(rs.region[:, 0]), torch.from_numpy(rs.region[:, 1])
    ll_p = params.get("lens_light", [{} for _ in pm.lens_light])
    fn = (lambda *a, **k: light_any(*a, unit=True, **k)) if stacked else (lambda *a, **k: light_any(*a, **k)[None])
    chans = []
    for lm, p, c in zip(pm.lens_light, ll_p, rs._consts("lens_light_constants", len(pm.lens_light))):
        chans.append(fn(lm, rs.img_X, rs.img_Y, **p, **c))
    for lm, p, c, cs in zip(pm.source_light, params["source_light"], rs._consts("source_light_constants", len(pm.source_light)), scales):
        if float(cs) == 1.0:
            chans.append(fn(lm, b1x, b1y, **p, **c))
        else:
            chans.append(fn(lm, rs.img_X - float(cs) * ax, rs.img_Y - float(cs) * ay, **p, **c))
    flat = torch.cat(chans, dim=0)  # (depth, N, bs)
    if not stacked:
        flat = flat.sum(dim=0, keepdim=True)
    img = torch.stack([torch.zeros((Hs, Ws, rs.bs), dtype=rs.dtype).index_put((rr, cc), flat[k], accumulate=True)
                       for k in range(flat.shape[0])], dim=0)
    img = torch.where(torch.isnan(img), torch.zeros_like(img), img)
    ret = img.permute(3, 0, 1, 2)  # (bs, depth, Hs, Ws)
    ret = torch.cat([ref.psf_pool(ret[:, k:k + 1], rs.flat_kernel, rs.supersample) for k in range(ret.shape[1])], dim=1)
    if stacked:
        return ret.permute(0, 2, 3, 1)
    return ret[:, 0] * rs.conversion_factor


def expected_stats(rs, params, obs, background_rms, exp_time):
    """``stats_pixels`` (tf/model.py:89-101) on ``expected_image``: ``(log_like, red_chi2, image)``."""
    dt = rs.dtype
    im = expected_image(rs, params)
    bg = torch.as_tensor(np.float32(background_rms)).to(dt)
    et = torch.as_tensor(np.float32(exp_time)).to(dt)
    err = torch.sqrt(bg ** 2 + im / et)
    o = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(dt)
    reg = rs.img_region
    chi2 = torch.sum(((im - o) / err) ** 2 * reg, dim=(-2, -1))
    norm = torch.sum(torch.log(2 * np.pi * err ** 2) * reg, dim=(-2, -1))
    return -0.5 * (chi2 + norm), chi2 / torch.count_nonzero(reg).to(dt), im


def expected_lstsq(rs, params, obs, err):
    """``lstsq_simulate`` (tf/simulator.py:158-240) on the basis stack: ``(coeffs, image)`` by the float64 pinv."""
    dt = rs.dtype
    st = expected_image(rs, params, stacked=True).permute(0, 3, 1, 2)  # (bs, depth, H, W)
    W = 1 / torch.as_tensor(np.asarray(err, dtype=np.float32)).to(dt)
    Y = (torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(dt) * W).reshape(1, -1, 1)
    X = (st * W).reshape(rs.bs, st.shape[1], -1).permute(0, 2, 1)
    Xt = X.permute(0, 2, 1)
    coeffs = (torch.linalg.pinv(Xt @ X, rcond=1e-6) @ Xt @ Y)[..., 0]
    return coeffs, (st * coeffs[:, :, None, None]).sum(dim=1)


def ref_sim(wl, bs, dtype=F64, psf=None, grid_shift=None):
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, bs, dtype=dtype, supersampled_kernel=psf)
    if grid_shift is not None:
        rs.img_X = rs.img_X + torch.as_tensor(grid_shift[0], dtype=dtype)
        rs.img_Y = rs.img_Y + torch.as_tensor(grid_shift[1], dtype=dtype)
    return rs


def loglike_and_grad(wl, packed, obs, dtype=F64, psf=None, grid_shift=None):
    """``(log_like, red_chi2, d log_like / d packed, image)`` of the composition in ``dtype`` (numpy arrays)."""
    rs = ref_sim(wl, packed.shape[0], dtype, psf, grid_shift)
    p = packed.detach().cpu().to(dtype).clone().requires_grad_(True)
    ll, red, im = expected_stats(rs, H.struct_from_packed(wl.phys_model, p), obs, wl.background_rms, wl.exp_time)
    (g,) = torch.autograd.grad(ll.sum(), p)
    return ll.detach().numpy(), red.detach().numpy(), g.numpy(), im.detach().numpy()


def image_vjp(wl, packed, cot, dtype=F64, psf=None, grid_shift=None):
    """``(image, d sum(image * cot) / d packed)`` of the composition."""
    rs = ref_sim(wl, packed.shape[0], dtype, psf, grid_shift)
    p = packed.detach().cpu().to(dtype).clone().requires_grad_(True)
    im = expected_image(rs, H.struct_from_packed(wl.phys_model, p))
    (g,) = torch.autograd.grad((im * torch.as_tensor(cot).to(dtype)).sum(), p)
    return im.detach().numpy(), g.numpy()


def conditioning_bound(wl, grad_fn, g_o, S, seed=0):
    """``helpers.float32_conditioning_bound`` on this composition (the oracle's own ``stats_pixels`` has no interpolated light): how far
    float32 rounding of the ray-shoot alone -- the grid displaced by one float32 spacing of its largest coordinate, uniformly along
    (+,+) and (+,-) and by two draws of pixel noise of that rms -- moves each element of the float64 gradient ``g_o = grad_fn(None)``,
    relative to ``S``.  ``grad_fn(grid_shift)``: the float64 gradient on the displaced grid."""
    rs = ref_sim(wl, 1)
    d = float(np.spacing(np.float32(max(float(rs.img_X.abs().max()), float(rs.img_Y.abs().max())))))
    rng = np.random.default_rng(seed)
    n = rs.img_X.shape[0]
    shifts = [(d, d), (d, -d), (d * rng.normal(size=(n, 1)), d * rng.normal(size=(n, 1))),
              (d * rng.normal(size=(n, 1)), d * rng.normal(size=(n, 1)))]
    out = np.zeros_like(np.asarray(g_o, dtype=np.float64))
    for sh in shifts:
        g_p = grad_fn(sh)
        out = np.maximum(out, np.abs(g_p - g_o) / np.maximum(S, 1e-300))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# images, models and poses
# ---------------------------------------------------------------------------------------------------------------------
def make_image(h, w, seed=0):
    """A deliberately asymmetric positive image: a ramp along both axes plus noise, no two pixels equal."""
    r = np.random.default_rng(1000 * h + w + seed)
    jj, ii = np.mgrid[:h, :w]
    return (1.0 + 0.6 * ii + 0.25 * jj * jj + 0.3 * r.random((h, w))).astype(np.float32)


IMG_SMALL, IMG_BIG = make_image(2, 3), make_image(16, 16)
GRIDS = {"7x9": (7, 9), "33x31": (33, 31)}
DELTA_PIX = 0.1


def _phys(model, images, orders, use_lstsq=False, scales=None):
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light import Interpolated
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    interp = [Interpolated(im, order=o, use_lstsq=use_lstsq) for im, o in zip(images, orders)]
    if model == "A":  # EPL + Shear | Interpolated
        return PhysicalModel([EPL(), Shear()], [], interp[:1])
    if model == "B":  # SIE | Sersic lens light + Interpolated + Sersic
        return PhysicalModel([SIE()], [Sersic(use_lstsq=use_lstsq)], [interp[0], Sersic(use_lstsq=use_lstsq)])
    if model == "C":  # 2 NFW | 2 Interpolated with different images and orders
        return PhysicalModel([NFW(), NFW()], [], interp[:2], source_light_scales=scales)
    raise KeyError(model)


def _rows(model, half, images, r):
    """Three parameter rows in the native column order, the source poses drawn so that the lensed rays cover the image, its apron
    and the sky beyond; the LAST row's sources sit far off the field (every pixel out of range)."""
    rows = []
    for b in range(3):
        off = 0.0 if b < 2 else 40.0 * half
        def pose(im, k):
            fp = 0.55 * half / max(im.shape)  # arcsec per image pixel: the image spans about half the field
            return [r.normal(0, 0.05 * half) + off, r.normal(0, 0.05 * half) - off, r.uniform(-math.pi, math.pi),
                    fp * r.uniform(0.8, 1.2), 30.0 * r.uniform(0.7, 1.3) * (1 + k)]
        if model == "A":
            row = [0.45 * half * r.uniform(0.9, 1.1), r.uniform(1.8, 2.2), r.normal(0, 0.1), r.normal(0, 0.1), r.normal(0, 0.02 * half),
                   r.normal(0, 0.02 * half), r.normal(0, 0.03), r.normal(0, 0.03)] + pose(images[0], 0)
        elif model == "B":
            row = [0.45 * half * r.uniform(0.9, 1.1), r.normal(0, 0.1), r.normal(0, 0.1), r.normal(0, 0.02 * half), r.normal(0, 0.02 * half)]
            row += [0.5 * half, r.uniform(2, 4), r.normal(0, 0.02 * half), r.normal(0, 0.02 * half), 8.0]
            row += pose(images[0], 0)
            row += [0.15 * half, r.uniform(1, 3), r.normal(0, 0.1 * half), r.normal(0, 0.1 * half), 25.0]
        else:
            row = []
            for sgn in (-1, 1):
                row += [half * r.uniform(0.8, 1.2), 0.2 * half * r.uniform(0.8, 1.2), sgn * 0.3 * half + r.normal(0, 0.02 * half),
                        r.normal(0, 0.1 * half)]
            row += pose(images[0], 0) + pose(images[1], 1)
        rows.append(row)
    return torch.tensor(rows, dtype=torch.float32)


def case(model, grid, images=None, orders=None, supersample=1, pix_region=None, scales=None, use_lstsq=False, seed=0):
    """``(workload, packed rows [3, P] float32 on the CPU)`` of one parity case.  Without ``use_lstsq`` the rows hold every
    column; with it the amplitude columns are present too (the linear solve overwrites them)."""
    from gigalens_amd import workloads
    from gigalens_amd.simulator import SimulatorConfig
    if images is None:
        images = {"A": [IMG_SMALL], "B": [IMG_BIG], "C": [IMG_SMALL, IMG_BIG]}[model]
        if grid == "33x31" and model != "C":
            images = [IMG_BIG if images[0] is IMG_SMALL else IMG_SMALL]
    if orders is None:
        orders = {"A": [3], "B": [1], "C": [1, 3]}[model]
        if grid == "33x31" and model != "C":
            orders = [4 - orders[0]]
    n = GRIDS[grid]
    half = 0.5 * DELTA_PIX * min(n)
    phys = _phys(model, images, orders, use_lstsq, scales)
    cfg = SimulatorConfig(delta_pix=DELTA_PIX, num_pix=n, supersample=supersample, pix_region=pix_region)
    wl = workloads.Workload(f"INT-{model}-{grid}", phys, None, cfg, 3)
    r = np.random.default_rng(7 + seed + ord(model) + n[0])
    return wl, _rows(model, half, images, r)


def prior_around(wl, packed, width=0.05):
    """A prior centred on the rows' mean, one leaf per sampled parameter: LogNormal (Exp bijector) for ``scale`` and the amplitudes,
    Normal (identity) for the rest -- the fused ``log_prob`` front end sees both bijectors."""
    from gigalens_amd import prior as tfd
    mean = packed.double().mean(dim=0).numpy()
    pm = wl.phys_model
    groups, k = {}, 0
    for g, profs in zip(H.GROUPS, (pm.lenses, pm.lens_light, pm.source_light)):
        lst = []
        for p in profs:
            d = {}
            for n in p._native_params():
                if n in p.params:
                    v = float(mean[k])
                    d[n] = tfd.LogNormal(math.log(v), width) if n in ("scale", "amp", "Ie") else tfd.Normal(v, width * (abs(v) + 0.1))
                k += 1
            lst.append(tfd.JointDistributionNamed(d))
        if lst:
            groups[g] = tfd.JointDistributionSequential(lst)
    return tfd.JointDistributionNamed(groups)


def coverage(wl, packed, psf=None):
    """Per sample and interpolated source: how many rays land inside the image, in its apron ring, and outside the range."""
    rs = ref_sim(wl, packed.shape[0], F64, psf)
    params = H.struct_from_packed(wl.phys_model, packed.double())
    bx, by = rs.beta(rs.img_X, rs.img_Y, params["lens_mass"])
    ax, ay = rs.img_X - bx, rs.img_Y - by
    out = []
    pm = wl.phys_model
    for lm, p, cs in zip(pm.source_light, params["source_light"], pm.source_light_scales):
        if lm.name != "INTERPOL":
            continue
        Hh, Ww = lm.image.shape
        u, v = pixel_coords(rs.img_X - float(cs) * ax, rs.img_Y - float(cs) * ay, (Hh, Ww), p["center_x"], p["center_y"], p["phi"], p["scale"])
        inside = (u >= 0) & (u <= Ww - 1) & (v >= 0) & (v <= Hh - 1)
        rng = (u >= -2) & (u <= Ww + 1) & (v >= -2) & (v <= Hh + 1)
        out.append(torch.stack([inside.sum(0), (rng & ~inside).sum(0), (~rng).sum(0)], dim=1).numpy())
    return out


def observation(wl, packed, psf=None, seed=4):
    """A noisy float32 image of the model's own scale: the float64 expectation of the first row plus noise of the likelihood's rms."""
    rs = ref_sim(wl, 1, F64, psf)
    img = expected_image(rs, H.struct_from_packed(wl.phys_model, packed[:1].double()))[0].numpy()
    r = np.random.default_rng(seed)
    return (img + r.normal(size=img.shape) * np.sqrt(wl.background_rms ** 2 + np.clip(img, 0, None) / wl.exp_time)).astype(np.float32)


def gauss_psf(n, sigma):
    g = np.exp(-0.5 * ((np.arange(n) - (n - 1) / 2) / sigma) ** 2)
    k = np.outer(g, g).astype(np.float32)
    return k / k.sum()


# ---------------------------------------------------------------------------------------------------------------------
# float64 host build of the kernels' templates (tests/hostmath/interp_host.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def _host_sources():
    src = os.path.join(ROOT, "tests", "hostmath", "interp_host.cpp")
    csrc = os.path.join(ROOT, "gigalens_amd", "csrc")
    return src, [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h") and not f.endswith(".hip.h")]


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def interp_host():
    """ctypes handle of tests/hostmath/interp_host.cpp compiled with g++ (rebuilt when it or a csrc header is newer)."""
    global _SO
    if _SO is None:
        src, deps = _host_sources()
        so = os.path.join(ROOT, "tests", "hostmath", "libinterp_host.so")
        if _stale(so, deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        _SO = ctypes.CDLL(so)
        dp = POINTER(c_double)
        _SO.interp_light_d.argtypes = [c_int, c_int, c_int, dp, dp, c_int, dp, dp, dp, dp, dp, dp, dp]
        _SO.interp_weights_d.argtypes = [c_int, c_double, dp, dp]
    return _SO


def interp_host_program():
    """Path of the same source built as its stand-alone program (tests/hostmath/interp_host_check)."""
    src, deps = _host_sources()
    exe = os.path.join(ROOT, "tests", "hostmath", "interp_host_check")
    if _stale(exe, deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    return exe


def _dp(a):
    return a.ctypes.data_as(POINTER(c_double))


def host_light(order, image, p, x, y, gI):
    """The float64 instantiation of interp_prep / fwd / vjp / finalize: ``(I [n], grad [5], gpx [n], gpy [n])``."""
    img = np.ascontiguousarray(image, dtype=np.float64)
    x, y, gI = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y, gI))
    pp = np.ascontiguousarray(p, dtype=np.float64)
    I, gpx, gpy, grad = np.empty_like(x), np.empty_like(x), np.empty_like(x), np.empty(5)
    interp_host().interp_light_d(int(order == 1), img.shape[0], img.shape[1], _dp(img), _dp(pp), x.size, _dp(x), _dp(y), _dp(gI),
                                 _dp(I), _dp(grad), _dp(gpx), _dp(gpy))
    return I, grad, gpx, gpy


def host_weights(order, t):
    w, dw = np.empty(4), np.empty(4)
    interp_host().interp_weights_d(int(order == 1), float(t), _dp(w), _dp(dw))
    return w, dw
