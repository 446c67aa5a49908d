"""Models, inputs and float64 expectations of the multi-source-plane tests (tests/test_gpu_multiplane.py,
tests/test_multiplane_host.py): sources and image families with deflection scales c of their own behind one lens plane,
``beta_s = theta - c_s sum alpha`` and ``A_s = I - c_s H``.

The expectations are composed from the oracle's existing primitives (oracle/ref_torch.py, unchanged): ``RefSimulator.beta`` gives
sum alpha, ``light_eval`` renders each source at its own beta_s, then NaN -> 0, ``psf_pool``, the conversion factor and the formulas of
``stats_pixels``; the position term restates ``stats_positions`` with ``beta = theta - c_f alpha`` and ``lens_hessian_autodiff`` times
c_f.  Gradients come from torch autograd on the float64 composition."""
import math

import numpy as np
import torch

from tests import helpers as H

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# float64 expectations
# ---------------------------------------------------------------------------------------------------------------------
def expected_image(rs, params, scales, stacked=False):
    """The image of ``RefSimulator.simulate`` (tf/simulator.py:109-156) with source s rendered at ``theta - c_s sum alpha``.
    ``stacked``: the unit-amplitude basis stack ``(bs, H, W, depth)`` of ``lstsq_simulate`` instead."""
    from oracle import ref_torch as ref
    pm = rs.phys_model
    b1x, b1y = rs.beta(rs.img_X, rs.img_Y, params["lens_mass"])
    ax, ay = rs.img_X - b1x, rs.img_Y - b1y  # sum alpha
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    rr, cc = torch.from_numpy(rs.region[:, 0]), torch.from_numpy(rs.region[:, 1])
    ll_p = params.get("lens_light", [{} for _ in pm.lens_light])
    chans = []
    fn = ref.light_basis if stacked else (lambda *a, **k: ref.light_eval(*a, **k)[None])
    for lm, p, c in zip(pm.lens_light, ll_p, rs._consts("lens_light_constants", len(pm.lens_light))):
        chans.append(fn(lm, rs.img_X, rs.img_Y, **p, **c))
    for lm, p, c, cs in zip(pm.source_light, params["source_light"], rs._consts("source_light_constants", len(pm.source_light)), scales):
        chans.append(fn(lm, rs.img_X - float(cs) * ax, rs.img_Y - float(cs) * ay, **p, **c))
    flat = torch.cat(chans, dim=0)  # (depth, N, bs)
    if not stacked:
        flat = flat.sum(dim=0, keepdim=True)
    img = torch.zeros((flat.shape[0], Hs, Ws, rs.bs), dtype=rs.dtype)
    img = _scatter(img, rr, cc, flat)
    img = torch.where(torch.isnan(img), torch.zeros_like(img), img)
    ret = img.permute(3, 0, 1, 2)  # (bs, depth, Hs, Ws)
    ret = torch.cat([ref.psf_pool(ret[:, k:k + 1], rs.flat_kernel, rs.supersample) for k in range(ret.shape[1])], dim=1)
    if stacked:
        return ret.permute(0, 2, 3, 1)
    return ret[:, 0] * rs.conversion_factor


def _scatter(img, rr, cc, flat):
    out = []
    for k in range(flat.shape[0]):
        out.append(img[k].index_put((rr, cc), flat[k], accumulate=True))
    return torch.stack(out, dim=0)


def expected_stats_pixels(rs, params, scales, obs, background_rms=None, exp_time=None, error_map=None):
    """``stats_pixels`` (tf/model.py:89-101) on ``expected_image``: ``(log_like, red_chi2, image)``."""
    dt = rs.dtype
    im = expected_image(rs, params, scales)
    if error_map is not None:
        err = torch.as_tensor(np.asarray(error_map, dtype=np.float32)).to(dt)
    else:
        bg = torch.as_tensor(np.float32(background_rms)).to(dt)
        et = torch.as_tensor(np.float32(exp_time)).to(dt)
        err = torch.sqrt(bg ** 2 + im / et)
    o = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(dt)
    reg = rs.img_region
    chi2 = torch.sum(((im - o) / err) ** 2 * reg, dim=(-2, -1))
    norm = torch.sum(torch.log(2 * np.pi * err ** 2) * reg, dim=(-2, -1))
    return -0.5 * (chi2 + norm), chi2 / torch.count_nonzero(reg).to(dt), im


def expected_lstsq(rs, params, scales, obs, err):
    """``lstsq_simulate`` (tf/simulator.py:158-240) on the scaled basis stack: ``(coeffs, image)`` by the float64 pinv."""
    dt = rs.dtype
    st = expected_image(rs, params, scales, stacked=True)  # (bs, H, W, depth)
    st = torch.where(torch.isnan(st), torch.zeros_like(st), st).permute(0, 3, 1, 2)
    W = 1 / torch.as_tensor(np.asarray(err, dtype=np.float32)).to(dt)
    Y = (torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(dt) * W).reshape(1, -1, 1)
    X = (st * W).reshape(rs.bs, st.shape[1], -1).permute(0, 2, 1)
    Xt = X.permute(0, 2, 1)
    coeffs = (torch.linalg.pinv(Xt @ X, rcond=1e-6) @ Xt @ Y)[..., 0]
    return coeffs, (st * coeffs[:, :, None, None]).sum(dim=1)


def expected_stats_positions(rs, params, cxs, cys, exs, eys, scales):
    """``stats_positions`` (tf/model.py:103-124) with family f on its own plane: ``(log_like, red_chi2, min |det A|)``."""
    from oracle import ref_torch as ref
    dt, bs = rs.dtype, rs.bs
    chi2 = log_like = 0.0
    n_position, min_det = 0.0, math.inf
    for cx, cy, cex, cey, c in zip(cxs, cys, exs, eys, scales):
        c = float(c)
        cx = torch.as_tensor(np.asarray(cx, dtype=np.float32)).to(dt)[:, None].repeat(1, bs)
        cy = torch.as_tensor(np.asarray(cy, dtype=np.float32)).to(dt)[:, None].repeat(1, bs)
        cex = torch.as_tensor(np.asarray(cex, dtype=np.float32)).to(dt)
        cey = torch.as_tensor(np.asarray(cey, dtype=np.float32)).to(dt)
        n_position += 2.0 * cx.shape[0]
        b1x, b1y = rs.beta(cx, cy, params["lens_mass"])
        bx, by = cx - c * (cx - b1x), cy - c * (cy - b1y)
        beta = torch.stack([bx, by], dim=0).permute(2, 0, 1)
        bary = beta.mean(dim=2, keepdim=True)
        fxx, fxy, fyx, fyy = (c * t for t in ref.lens_hessian_autodiff(rs, cx, cy, params["lens_mass"]))
        det = (1 - fxx) * (1 - fyy) - fxy * fyx
        min_det = min(min_det, float(det.detach().abs().min()))
        mag = (1.0 / det).permute(1, 0)
        err = torch.stack([cex / mag, cey / mag], dim=1)
        chi2_i = (((beta - bary) / err) ** 2).sum(dim=(-2, -1))
        norm_i = torch.log(2 * np.pi * err ** 2).sum(dim=(-2, -1))
        log_like = log_like + (-0.5) * (chi2_i + norm_i)
        chi2 = chi2 + chi2_i
    return log_like, chi2 / n_position, min_det


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
PIX_SCALES = (0.6, 1.3)


def pixel_model(num_pix, batch, scales=PIX_SCALES, supersample=1, pix_region=None, use_lstsq=False):
    """SIE + Shear | SersicEllipse lens light | two SersicEllipse sources on planes of their own: the interpreter's model."""
    from gigalens_amd import prior as tfd
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    sie = J(dict(theta_E=tfd.LogNormal(math.log(1.0), 0.05), e1=tfd.Normal(0.1, 0.05), e2=tfd.Normal(-0.05, 0.05),
                 center_x=tfd.Normal(0, 0.03), center_y=tfd.Normal(0, 0.03)))
    shear = J(dict(gamma1=tfd.Normal(0, 0.03), gamma2=tfd.Normal(0, 0.03)))

    def ser(r, ie, cx):
        d = dict(R_sersic=tfd.LogNormal(math.log(r), 0.1), n_sersic=tfd.Uniform(1, 3), e1=tfd.Normal(0, 0.1), e2=tfd.Normal(0, 0.1),
                 center_x=tfd.Normal(cx, 0.05), center_y=tfd.Normal(-cx, 0.05))
        if not use_lstsq:
            d["Ie"] = tfd.LogNormal(math.log(ie), 0.2)
        return J(d)
    mk = lambda: SersicEllipse(use_lstsq=True) if use_lstsq else SersicEllipse()
    phys = PhysicalModel([SIE(), Shear()], [mk()], [mk(), mk()], source_light_scales=scales)
    prior = J(dict(lens_mass=S([sie, shear]), lens_light=S([ser(0.6, 60.0, 0.0)]),
                   source_light=S([ser(0.2, 150.0, 0.1), ser(0.15, 120.0, -0.15)])))
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=num_pix, supersample=supersample, pix_region=pix_region)
    return workloads.Workload("MP", phys, prior, cfg, batch)


def rescaled(wl, scales):
    """The workload with the same profiles, prior and camera and ``source_light_scales = scales``."""
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    ph = wl.phys_model
    phys = PhysicalModel(ph.lenses, ph.lens_light, ph.source_light, ph.lenses_constants, ph.lens_light_constants,
                         ph.source_light_constants, source_light_scales=scales)
    return workloads.Workload(wl.name, phys, wl.prior, wl.sim_config, wl.batch)


STATIC_SCALE = (0.7,)


def static_model(lens_light, num_pix=47, batch=6, scales=STATIC_SCALE):
    """EPL + Shear | [Sersic lens light] | Sersic source: the compositions the specialised pair kernels serve when unscaled
    (47 x 47 px: 2209 pixels, ragged; six samples: with GIGALENS_HIP_TAIL_N / _ROWS the unscaled model gets a tapered dispatch)."""
    from gigalens_amd import prior as tfd
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    wl = workloads.make("C2", num_pix=num_pix, batch=batch)
    if not lens_light:
        return rescaled(wl, scales)
    ll = J(dict(R_sersic=tfd.LogNormal(math.log(0.7), 0.1), n_sersic=tfd.Uniform(2, 4), center_x=tfd.Normal(0, 0.03),
                center_y=tfd.Normal(0, 0.03), Ie=tfd.LogNormal(math.log(60.0), 0.2)))
    lens, src = workloads._epl_prior(), workloads._sersic_src_prior()
    prior = J(dict(lens_mass=S([lens, workloads._shear_prior()]), lens_light=S([ll]), source_light=S([src])))
    phys = PhysicalModel(wl.phys_model.lenses, [Sersic()], wl.phys_model.source_light, source_light_scales=scales)
    return workloads.Workload("C2L", phys, prior, wl.sim_config, batch)


N_HALOS, N_SOURCES = 5, 13
CLUSTER_SCALES = tuple(np.round(np.linspace(0.5, 1.4, N_SOURCES), 4).tolist())


def cluster_model(ellipse, num_pix=23, batch=3, scales=CLUSTER_SCALES):
    """5 NFW | 13 Sersic[Ellipse] sources with 13 distinct scales: counts that are no multiples of four (neutral slots live)."""
    from gigalens_amd import prior as tfd
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.simulator import SimulatorConfig
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    halo = lambda: J(dict(Rs=tfd.LogNormal(math.log(2.0), 0.3), alpha_Rs=tfd.LogNormal(math.log(0.5), 0.3),
                          center_x=tfd.Uniform(-1.5, 1.5), center_y=tfd.Uniform(-1.5, 1.5)))
    src = dict(R_sersic=tfd.LogNormal(math.log(0.25), 0.15), n_sersic=tfd.Uniform(0.5, 4), center_x=tfd.Uniform(-1, 1),
               center_y=tfd.Uniform(-1, 1), Ie=tfd.LogNormal(math.log(150.0), 0.5))
    if ellipse:
        src.update(e1=tfd.Normal(0, 0.15), e2=tfd.Normal(0, 0.15))
    phys = PhysicalModel([NFW() for _ in range(N_HALOS)], [], [(SersicEllipse if ellipse else Sersic)() for _ in range(N_SOURCES)],
                         source_light_scales=scales)
    prior = J(dict(lens_mass=S([halo() for _ in range(N_HALOS)]), source_light=S([J(dict(src)) for _ in range(N_SOURCES)])))
    return workloads.Workload("MPC", phys, prior, SimulatorConfig(delta_pix=0.13, num_pix=num_pix), batch)


def gauss_psf(n, sigma):
    g = np.exp(-0.5 * ((np.arange(n) - (n - 1) / 2) / sigma) ** 2)
    k = np.outer(g, g).astype(np.float32)
    return k / k.sum()


def observation(wl, seed=4):
    """A noisy float32 image of the model's own scale, drawn on the host from the float64 expectation of one prior sample."""
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, 1, dtype=F64)
    x = wl.prior.sample(1, seed=seed + 100)
    x64 = {g: [{k: torch.as_tensor(v).double().cpu() for k, v in d.items()} for d in lst] for g, lst in x.items()}
    if any(getattr(p, "use_lstsq", False) for p in wl.phys_model.source_light):  # any image serves a projection: a ring and a core
        n = wl.sim_config.num_pix
        yy, xx = np.mgrid[:n, :n]
        rad = np.hypot(xx - n / 2, yy - n / 2) * wl.sim_config.delta_pix
        img = 40 * np.exp(-0.5 * ((rad - 1.0) / 0.15) ** 2) + 80 * np.exp(-0.5 * (rad / 0.5) ** 2)
    else:
        img = expected_image(rs, x64, wl.phys_model.source_light_scales)[0].numpy()
    r = np.random.default_rng(seed)
    bg, t = 0.2, 100.0
    obs = img + r.normal(size=img.shape) * np.sqrt(bg ** 2 + np.clip(img, 0, None) / t)
    return obs.astype(np.float32), bg, t


def params64(phys, packed):
    """(leaf tensor [B, P] float64 with grad, nested structure on it)."""
    p = packed.detach().cpu().double().requires_grad_(True)
    return p, H.struct_from_packed(phys, p)
