"""Float64 restatement of the flux-ratio likelihood of the image families (csrc/gl_fluxes.hip.h) and the cases of its tests:
tests/test_fluxes_host.py pins the restatement without a GPU, tests/test_gpu_fluxes.py runs the kernels against it.

The term sits on ``mp_positions_cases.trace``, which gives ``beta`` and ``A = d beta / d theta`` of every observed image on K >= 1
planes, differentiable in the packed rows: ``m_j = 1 / |det A_j|``; images with a measured flux ``F_j`` and error ``s_j`` weigh
``w_j = 1 / s_j^2`` (NaN: no measurement); the unlensed flux of the family is profiled out,

    S_f = sum w F m / sum w m^2 ,   chi2_f = sum w (F - S_f m)^2 ,   ll_f = -1/2 (chi2_f + sum log(2 pi s^2)) .

Every function takes ``dtype``: float64 is the reference, the same code in float32 on the CPU the yardstick (``data``, as
``mp_positions_cases.data``).

Deterministic data: ``F_j = (3 + f) |mu_j of sample 0 in float64| * PATTERN[j]``, ``s_j = 0.05 F_j`` -- sample 0 misses its fluxes by
the pattern alone, the other samples by their own magnifications as well.

The cases of ``mp_positions_cases`` have ``det A > 0`` at every image (their rings lie outside the critical curves) and never take the
``|mu|`` branch.  ``mixed2`` (the ``k2`` lens set) and ``single`` / ``plain`` (the same lenses on one plane, with and without
per-family scales) hold images of both parities in every sample: lattice points inside the critical curves, found by scanning for
``det A <= -MIN_DET`` in every sample and meeting ``PC.conditions`` (asserted in the host test)."""
import functools

import numpy as np
import torch

from tests import multilens_cases as MC
from tests import mp_positions_cases as PC

F64, F32 = MC.F64, MC.F32
PATTERN = (1.12, 0.9, 1.05, 0.85, 1.2)
REL_ERR = 0.05


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def dets(phys, mp, lp, fam, B, dtype=F64):
    """``det A [J_f, B]`` of the images of family ``fam``, differentiable in ``lp``."""
    cx, cy = PC._points(fam["x"], dtype, B), PC._points(fam["y"], dtype, B)
    _, _, A, _ = PC.trace(phys, mp, lp, cx, cy, fam["T"])
    return A[0] * A[3] - A[1] * A[2]


def family_term(det, flux, flux_err, detach_amplitude=False):
    """``(log_like [B], chi2 [B], S [B], model flux [J_f, B])`` of one family from ``det A [J_f, B]`` and its fluxes and errors
    (``flux`` None or all NaN: no fluxes -- exactly 0, 0 and NaN).  ``detach_amplitude``: ``S_f`` held fixed in the derivative."""
    dt = det.dtype
    m = 1.0 / det.abs()
    zero = torch.zeros(det.shape[1], dtype=dt)
    meas = None if flux is None else ~np.isnan(np.asarray(flux, dtype=np.float64))
    if meas is None or not meas.any():
        nan = torch.full_like(zero, float("nan"))
        return zero, zero, nan, nan[None, :] * m.detach()
    idx = torch.as_tensor(np.flatnonzero(meas))
    F = torch.as_tensor(np.asarray(flux, dtype=np.float64)[meas]).to(dt)[:, None]  # (the cases hold float32 values, kept exactly)
    s = torch.as_tensor(np.asarray(flux_err, dtype=np.float64)[meas]).to(dt)[:, None]
    w, mm = 1.0 / s ** 2, m[idx]
    S = (w * F * mm).sum(dim=0) / (w * mm ** 2).sum(dim=0)
    if detach_amplitude:
        S = S.detach()
    chi2 = (w * (F - S[None, :] * mm) ** 2).sum(dim=0)
    norm = torch.log(2 * np.pi * s ** 2).sum()
    return -0.5 * (chi2 + norm), chi2, S, S[None, :] * m


def stats(phys, mp, lp, fams, B, dtype=F64, detach_amplitude=False):
    """``(log_like [B], chi2 [B], S [B, F], model flux [B, J], det A [J, B])`` over the families ``fams`` =
    ``[dict(x, y, T, flux, flux_err)]``; the first two differentiable in ``lp``."""
    log_like = chi2 = 0.0
    S, model, ds = [], [], []
    for fam in fams:
        det = dets(phys, mp, lp, fam, B, dtype)
        ll_f, chi2_f, S_f, model_f = family_term(det, fam.get("flux"), fam.get("flux_err"), detach_amplitude)
        log_like, chi2 = log_like + ll_f, chi2 + chi2_f
        S.append(S_f.detach())
        model.append(model_f.detach())
        ds.append(det.detach())
    return log_like, chi2, torch.stack(S, dim=1), torch.cat(model, dim=0).T, torch.cat(ds, dim=0)


def loglike_grad(c, dtype=F64, packed=None, fams=None, detach_amplitude=False):
    """``(log_like [B], chi2 [B], d log_like / d packed [B, P], S [B, F], model flux [B, J], det A [J, B])`` of case ``c`` as float64
    numpy arrays holding ``dtype`` arithmetic."""
    p, lp = PC.leaf(c, dtype, packed)
    ll, chi2, S, model, det = stats(c["phys"], c["mp"], lp, c["fams"] if fams is None else fams, c["B"], dtype, detach_amplitude)
    if ll.requires_grad:
        (g,) = torch.autograd.grad(ll.sum(), p)
    else:  # (no family has fluxes)
        g = torch.zeros_like(p)
    n = lambda t: t.detach().double().numpy()
    return n(ll), n(chi2), n(g), n(S), n(model), n(det)


def with_fluxes(c, fams, rule=None):
    """``fams`` with the deterministic fluxes of this module: ``F_j = (3 + f) |mu_j of sample 0 in float64| PATTERN[j]``,
    ``s_j = 0.05 F_j``, as float32.  ``rule(f, j)``: False for an image without a measurement (NaN)."""
    _, lp = PC.leaf(c)
    out = []
    for f, fam in enumerate(fams):
        mu0 = 1.0 / dets(c["phys"], c["mp"], lp, fam, c["B"])[:, 0].detach().abs().numpy()
        F = ((3 + f) * mu0 * np.asarray(PATTERN[:mu0.size])).astype(np.float32)
        s = (np.float32(REL_ERR) * F).astype(np.float32)
        if rule is not None:
            keep = np.asarray([bool(rule(f, j)) for j in range(F.size)])
            F, s = np.where(keep, F, np.float32(np.nan)), np.where(keep, s, np.float32(np.nan))
        out.append(dict(fam, flux=None if np.isnan(F).all() else F, flux_err=None if np.isnan(F).all() else s))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
GRAD_CASES = ("mixed2", "k4", "zoo_a", "single", "plain")
MIXED_CASES = ("mixed2", "single", "plain")
VARIANTS = ("one_nan", "partial")
CASES = GRAD_CASES + VARIANTS
# (redshift, lattice indices of x, of y, sigma): the k2 families with two images of the far family moved inside the critical curves
_MIXED2 = [(0.8, (21, -19, 3), (4, -6, 22), 0.01), (2.0, (-24, 26, 7, -8, 8), (9, -7, -3, 25, -1), 0.01)]
# one plane: the same lenses at one redshift, the families at redshifts of their own (`single`: two distinct centroids_scales) or
# both on the reference plane (`plain`: no scales) -- rings outside the critical curves with points inside them
_SINGLE = [(0.8, (21, -19, 3, 4), (4, -6, 22, -1), 0.01), (2.0, (-24, 26, 1, -8, -2), (9, -7, -6, 25, -7), 0.01)]
_PLAIN = [(0.8, (21, -19, 3, 1), (4, -6, 22, -7), 0.01), (2.0, (-24, 26, 0, -8, -4), (9, -7, -8, 25, -7), 0.01)]


@functools.lru_cache(maxsize=None)
def case(name):
    """``dict(phys, phys_mp, mp, params, B = 3, fams, pix, scales)``: the keys of ``mp_positions_cases.case`` with ``flux`` /
    ``flux_err`` in every family.  ``mixed2``: the ``k2`` lens set, both parities; ``k4`` / ``zoo_a``: those cases; ``single``: the ``k2``
    lenses on ONE plane (``phys_mp`` None, ``scales`` = the families' deflection scales, for ``centroids_scales``); ``plain``: one plane,
    no scales; ``one_nan``: ``mixed2`` with an unmeasured image in the far family; ``partial``: ``mixed2`` with an unmeasured image in
    the near family and NO fluxes in the far one -- the lens on the second plane meets the rays of the flux-less family alone."""
    from gigalens_amd.model import PhysicalModel
    if name in ("k4", "zoo_a"):
        c = dict(PC.case(name), scales=None)
        return dict(c, fams=with_fluxes(c, c["fams"]))
    m = MC.map_case("epl_shear|sie")
    lenses, lp = m["phys"].lenses, m["lens_params"]
    params = {"lens_mass": lp, "lens_light": [], "source_light": []}
    if name in ("single", "plain"):
        mp = MC._mp([0.5, 0.5, 0.5])
        assert mp.K == 1
        fams = [PC.family(mp, z, kx, ky, s) for z, kx, ky, s in (_SINGLE if name == "single" else _PLAIN)]
        if name == "plain":  # every family on the reference plane: coupling exactly 1
            fams = [dict(fm, T=np.ones(1)) for fm in fams]
        scales = [float(np.float32(fm["T"][0])) for fm in fams] if name == "single" else None
        c = dict(phys=PhysicalModel(lenses, [], []), phys_mp=None, mp=mp, params=params, B=3, fams=fams, pix=MC.PIX, scales=scales)
        return dict(c, fams=with_fluxes(c, fams))
    mp = MC._mp([0.5, 0.5, 1.0])
    fams = [PC.family(mp, z, kx, ky, s) for z, kx, ky, s in _MIXED2]
    c = dict(phys=PhysicalModel(lenses, [], []), phys_mp=PhysicalModel(lenses, [], [], multiplane=mp), mp=mp, params=params, B=3,
             fams=fams, pix=MC.PIX, scales=None)
    rule = {"mixed2": None, "one_nan": lambda f, j: not (f == 1 and j == 2), "partial": lambda f, j: f == 0 and j != 1}[name]
    return dict(c, fams=with_fluxes(c, fams, rule))


def centroids(c):
    """The keyword arguments of ``ForwardProbModel`` that carry the families of case ``c`` with their fluxes."""
    kw = dict(centroids_x=[fm["x"] for fm in c["fams"]], centroids_y=[fm["y"] for fm in c["fams"]],
              centroids_errors_x=[fm["ex"] for fm in c["fams"]], centroids_errors_y=[fm["ey"] for fm in c["fams"]],
              centroids_fluxes=[fm["flux"] for fm in c["fams"]], centroids_fluxes_errors=[fm["flux_err"] for fm in c["fams"]])
    if c["phys_mp"] is not None:
        kw["centroids_redshifts"] = [fm["z"] for fm in c["fams"]]
    elif c["scales"] is not None:
        kw["centroids_scales"] = c["scales"]
    return kw


def n_flux(c):
    return int(sum(0 if fm["flux"] is None else np.count_nonzero(~np.isnan(fm["flux"])) for fm in c["fams"]))


def _nan_err(got, ref):
    """``MC.rel_err`` over the finite entries of ``ref``; the NaN patterns must agree."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    return MC.rel_err(got[ok], ref[ok]) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def data(name):
    """``(case, ref, yard)`` -- computed once and shared (left unchanged).  ``ref``: ``log_like``, ``chi2``, ``grad``, ``S``, ``model`` and
    ``det`` in float64; ``yard``: the float32 restatement's deviation from them -- values relative to their largest (``MC.rel_err``),
    ``grad`` in units of the gate (``PC.grad_gate``)."""
    c = case(name)
    ll, chi2, g, S, model, det = loglike_grad(c, F64)
    ll32, chi232, g32, S32, model32, _ = loglike_grad(c, F32)
    ref = dict(log_like=ll, chi2=chi2, grad=g, S=S, model=model, det=det)
    yard = dict(log_like=MC.rel_err(ll32, ll), chi2=MC.rel_err(chi232, chi2), grad=PC.grad_gate(g32, g), S=_nan_err(S32, S),
                model=_nan_err(model32, model))
    return c, ref, yard
