"""Float64 restatement of the time-delay likelihood of the image families (csrc/gl_tdelays.hip.h) and the cases of its tests:
tests/test_tdelays_host.py pins the restatement without a GPU, tests/test_gpu_tdelays.py runs the kernels against it.

The term sits on ``mp_positions_cases.trace`` (one plane, K = 1, coupling 1), which gives ``beta`` of every observed image,
differentiable in the packed rows.  The family's source is the barycentre ``mean beta`` over all its images;

    phi_j = 1/2 |theta_j - mean beta|^2 - psi(theta_j) ,   w = 1 / s^2 over the measured images,   phi~, t~: minus the w-weighted means,
    lambda = the given scale  or  sum w t~ phi~ / sum w phi~^2 ,   chi2 = sum w (t~ - lambda phi~)^2 ,
    ll = -1/2 (chi2 + sum log(2 pi s^2)) ,   T = t_bar - lambda phi_bar ,   model delay_j = lambda phi_j + T .

``psi`` of the reference does NOT come from the ``*_pot`` templates: ``psi(theta_j) - psi(anchor)`` is the composite Gauss-Legendre line
integral of the oracle's float64 deflection (``oracle.ref_torch.mass_deriv``, the functions of ``potential_cases.KINDS``, in torch, so
that autograd gives the gradient) along a polyline from ONE anchor outside the lens: chords of the circle ``|theta| = R_ANCHOR`` to the
image's polar angle, then the radius inwards (``path``).  Every segment keeps ``MIN_CENTRE`` from every profile centre (``min_centre``;
asserted in the host test).  The anchor's psi is common to a family and cancels in ``phi~``: log_like, chi2, lambda, the model delays
and the gradient are independent of the templates and of the duals.  Only ``T`` sees the additive constant of psi: its reference adds
``lambda psi(anchor)`` with the float64 host build of the templates (``potential_cases.host_psi``) at that one point.

The catalogue case (``cat``: a dPIE catalogue of 3 members beside an SIE) takes psi from the float64 host build (``host_psi`` /
``host_psi_scaled``) and its gradient from central differences in float64.

The float32 yardstick is the same restatement in float32 with psi from the float32 host build of the templates
(``potential_host().pot_mass_f``; the catalogue's psi: the float64 host value rounded to float32, which can only lower the yardstick).
``YARD_CEILING``: twice the largest yardstick measured on the CPU when the cases were fixed -- a yardstick cannot later excuse a
broken kernel.

Deterministic data: ``t_j = LAMBDA0 phi_j(sample 0, float64) PATTERN[j]`` in days as float32, ``s_j = ERRORS[j]`` about a day."""
import ctypes
import functools

import numpy as np
import torch

from tests import helpers
from tests import multilens_cases as MC
from tests import mp_positions_cases as PC
from tests import potential_cases as POT

F64, F32 = MC.F64, MC.F32
LAMBDA0 = 80.0  # days / arcsec^2: D_dt of about 2900 Mpc
PATTERN = (1.02, 0.97, 1.01, 0.99, 1.03)
ERRORS = (1.0, 0.8, 1.2, 0.9, 1.1)
R_ANCHOR, MIN_CENTRE = 4.0, 0.2
ARC_STEP = np.pi / 6
_ARC_GL, _RAD_GL = (2, 16), (12, 16)  # (panels, nodes) of a chord and of the radial segment
# twice the largest yardsticks of the cases (x86-64 host, torch CPU float32, the templates built with g++ -O2): log_like 1.2e-5 and
# chi2 2.0e-5 (tnfw), scale 1.5e-4, offset 2.4e-5 and model 3.1e-6 (tnfw_cross: the float32 quadrature of the TNFW potential)
YARD_CEILING = dict(log_like=2.4e-5, chi2=4.0e-5, scale=3.0e-4, offset=4.9e-5, model=6.1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# psi differences: the line integral of the deflection
# ---------------------------------------------------------------------------------------------------------------------
def path(x, y):
    """The polyline from the anchor ``(R_ANCHOR, 0)`` to the image ``(x, y)``: ``[(xa, ya, xb, yb, is_radial)]``."""
    th = float(np.arctan2(y, x))
    n = int(np.ceil(abs(th) / ARC_STEP))
    angles = [th * k / n for k in range(n + 1)] if n else [0.0]
    pts = [(R_ANCHOR * np.cos(a), R_ANCHOR * np.sin(a)) for a in angles]
    segs = [(pts[k][0], pts[k][1], pts[k + 1][0], pts[k + 1][1], False) for k in range(n)]
    return segs + [(pts[-1][0], pts[-1][1], float(x), float(y), True)]


def _gl(panels, nodes):
    t, w = np.polynomial.legendre.leggauss(nodes)
    edges = np.linspace(0.0, 1.0, panels + 1)
    s = ((edges[:-1, None] + edges[1:, None]) / 2 + (edges[1:, None] - edges[:-1, None]) / 2 * t[None, :]).reshape(-1)
    return s, np.repeat((edges[1:] - edges[:-1]) / 2, nodes) * np.tile(w, panels)


def _nodes(xs, ys):
    """``(px, py [N], Wx, Wy [J, N])``: the quadrature nodes of every image's path and, per image, weight times direction."""
    px, py, rows = [], [], []
    for j, (x, y) in enumerate(zip(xs, ys)):
        for xa, ya, xb, yb, radial in path(x, y):
            s, w = _gl(*(_RAD_GL if radial else _ARC_GL))
            px.append(xa + (xb - xa) * s)
            py.append(ya + (yb - ya) * s)
            rows.append((j, w * (xb - xa), w * (yb - ya)))
    N = sum(p.size for p in px)
    Wx, Wy, k = np.zeros((len(xs), N)), np.zeros((len(xs), N)), 0
    for j, wx, wy in rows:
        Wx[j, k:k + wx.size], Wy[j, k:k + wx.size] = wx, wy
        k += wx.size
    return np.concatenate(px), np.concatenate(py), Wx, Wy


def psi_delta(phys, lp, xs, ys, B):
    """``psi(theta_j) - psi(anchor)`` ``[J, B]`` in float64, summed over the lenses, differentiable in ``lp`` (float64 tensors)."""
    from oracle import ref_torch as ref
    px, py, Wx, Wy = _nodes(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64))
    X = torch.as_tensor(px)[:, None].repeat(1, B)
    Y = torch.as_tensor(py)[:, None].repeat(1, B)
    consts = MC._consts(phys, F64)
    ax = ay = 0.0
    for l, lens in enumerate(phys.lenses):
        fx, fy = ref.mass_deriv(lens, X, Y, **lp[l], **consts[l])
        ax, ay = ax + fx, ay + fy
    return torch.as_tensor(Wx) @ ax + torch.as_tensor(Wy) @ ay


def min_centre(c):
    """The smallest distance of a path segment of case ``c`` to a profile centre (catalogue members included), over the samples."""
    centres = []
    for d in c["params"]["lens_mass"]:
        if "center_x" in d:
            centres += list(zip(np.asarray(d["center_x"], dtype=np.float64).reshape(-1), np.asarray(d["center_y"], dtype=np.float64).reshape(-1)))
    if c.get("catalogue") is not None:
        centres += list(zip(np.asarray(c["catalogue"]["center_x"], np.float64), np.asarray(c["catalogue"]["center_y"], np.float64)))
    best = np.inf
    for fam in c["fams"]:
        for x, y in zip(fam["x"], fam["y"]):
            for xa, ya, xb, yb, _ in path(x, y):
                d, L2 = np.array([xb - xa, yb - ya]), (xb - xa) ** 2 + (yb - ya) ** 2
                for cx, cy in centres:
                    t = np.clip(((cx - xa) * d[0] + (cy - ya) * d[1]) / L2, 0.0, 1.0)
                    best = min(best, float(np.hypot(xa + t * d[0] - cx, ya + t * d[1] - cy)))
    return best


# ---------------------------------------------------------------------------------------------------------------------
# psi of the templates' host build (float64: the anchor's constant and the catalogue case; float32: the yardstick)
# ---------------------------------------------------------------------------------------------------------------------
def _lens_rows(phys, packed):
    """``[(lens, its columns of the packed rows)]``."""
    out, k = [], 0
    for lens in phys.lenses:
        n = len(lens._native_params())
        out.append((lens, packed[:, k:k + n]))
        k += n
    return out


def host_psi_model(c, packed, xs, ys, dtype=F64):
    """``psi [J, B]`` summed over the lenses from the host build of the ``*_pot`` templates at the points ``xs, ys`` -- float64
    (``host_psi`` / ``host_psi_scaled``) or float32 (``pot_mass_f``; a catalogue: the float64 value rounded)."""
    packed = np.asarray(packed, dtype=np.float64)
    B, J = packed.shape[0], len(xs)
    np_t = np.float64 if dtype == F64 else np.float32
    out = np.zeros((J, B), dtype=np_t)
    x32, y32 = np.ascontiguousarray(xs, dtype=np.float32), np.ascontiguousarray(ys, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for lens, rows in _lens_rows(c["phys"], packed):
        for b in range(B):
            if getattr(lens, "_kind", 0) == 9:
                base_kind, cols, table = lens._catalogue()
                psi = POT.host_psi_scaled(base_kind, cols, table, rows[b], xs, ys).astype(np_t)
            elif dtype == F64:
                psi = POT.host_psi(lens._kind, rows[b], xs, ys, iparam=getattr(lens, "niter", 50))
            else:
                p = np.ascontiguousarray(rows[b], dtype=np.float32)
                psi = np.empty(J, dtype=np.float32)
                POT.potential_host().pot_mass_f(lens._kind, int(getattr(lens, "niter", 50)), fp(p), J, fp(x32), fp(y32), fp(psi))
            out[:, b] = out[:, b] + psi
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def family_term(phi, delay, delay_err, scale, fixed=False):
    """``(log_like [B], chi2 [B], lambda [B], T [B], model delay [J_f, B])`` of one family from ``phi [J_f, B]``, its arrival times and
    errors (``delay`` None or all NaN: no delays -- exactly 0, 0 and NaN) and its scale (NaN: profiled).  ``fixed``: lambda and T held
    fixed in the derivative (the formula of the kernels)."""
    dt = phi.dtype
    zero = torch.zeros(phi.shape[1], dtype=dt)
    meas = None if delay is None else ~np.isnan(np.asarray(delay, dtype=np.float64))
    if meas is None or not meas.any():
        nan = torch.full_like(zero, float("nan"))
        return zero, zero, nan, nan, nan[None, :] * phi.detach()
    idx = torch.as_tensor(np.flatnonzero(meas))
    t = torch.as_tensor(np.asarray(delay, dtype=np.float64)[meas]).to(dt)[:, None]  # (the cases hold float32 values, kept exactly)
    s = torch.as_tensor(np.asarray(delay_err, dtype=np.float64)[meas]).to(dt)[:, None]
    w, ph = 1.0 / s ** 2, phi[idx]
    pbar, tbar = (w * ph).sum(dim=0) / w.sum(), (w * t).sum(dim=0) / w.sum()
    pc, tc = ph - pbar[None, :], t - tbar[None, :]
    if np.isnan(scale):
        lam = (w * tc * pc).sum(dim=0) / (w * pc ** 2).sum(dim=0)
    else:
        lam = torch.full_like(zero, float(np.float32(scale)))
    T = tbar - lam * pbar
    if fixed:
        lam, T = lam.detach(), T.detach()
    chi2 = (w * (t - lam[None, :] * ph - T[None, :]) ** 2).sum(dim=0)
    norm = torch.log(2 * np.pi * s ** 2).sum()
    return -0.5 * (chi2 + norm), chi2, lam, T, lam[None, :] * phi + T[None, :]


def fermat(c, p, lp, fam, dtype=F64, psi=None):
    """``phi [J_f, B]`` of family ``fam``: differentiable in ``lp`` with the line-integral psi (float64, the additive constant of
    the anchor left out) or, ``psi`` given (``[J_f, B]``, not differentiable), with that psi."""
    B = p.shape[0]
    cx, cy = PC._points(fam["x"], dtype, B), PC._points(fam["y"], dtype, B)
    bx, by, _, _ = PC.trace(c["phys"], c["mp"], lp, cx, cy, np.ones(1))
    mbx, mby = bx.mean(dim=0, keepdim=True), by.mean(dim=0, keepdim=True)
    if psi is None:
        psi = psi_delta(c["phys"], lp, fam["x"], fam["y"], B)
    return 0.5 * ((cx - mbx) ** 2 + (cy - mby) ** 2) - torch.as_tensor(psi).to(dtype)


def stats(c, p, lp, dtype=F64, fixed=False, host=False, fams=None):
    """``(log_like [B], chi2 [B], lambda [B, F], T [B, F], model delay [B, J])`` over the families of case ``c`` at the packed leaf ``p``
    with its lens dicts ``lp``.  ``host``: psi from the host build of the templates in ``dtype`` (absolute, no gradient through psi);
    else the float64 line integral, ``T`` completed by ``lambda psi(anchor)``."""
    log_like = chi2 = 0.0
    lams, Ts, models = [], [], []
    rows = p.detach().double().numpy()
    for fam in (c["fams"] if fams is None else fams):
        psi = host_psi_model(c, rows, fam["x"], fam["y"], dtype) if host else None
        phi = fermat(c, p, lp, fam, dtype, psi)
        ll_f, chi2_f, lam, T, model = family_term(phi, fam.get("delay"), fam.get("delay_err"), fam.get("scale", np.nan), fixed)
        if not host:  # the constant the line integral leaves out
            psi_a = torch.as_tensor(host_psi_model(c, rows, [R_ANCHOR], [0.0], F64))[0]
            T = T + lam * psi_a
        log_like, chi2 = log_like + ll_f, chi2 + chi2_f
        lams.append(lam.detach())
        Ts.append(T.detach())
        models.append(model.detach())
    return log_like, chi2, torch.stack(lams, dim=1), torch.stack(Ts, dim=1), torch.cat(models, dim=0).T


def _np(t):
    return t.detach().double().numpy()


def loglike_grad(c, packed=None, fixed=False, fams=None):
    """``(log_like, chi2, grad [B, P], lambda, T, model)`` of case ``c`` in float64 (numpy): autograd through the line integral, or
    for the catalogue case the host psi and central differences."""
    p, lp = PC.leaf(c, F64, packed)
    if c.get("catalogue") is None:
        ll, chi2, lam, T, model = stats(c, p, lp, F64, fixed, fams=fams)
        g = torch.autograd.grad(ll.sum(), p)[0] if ll.requires_grad else torch.zeros_like(p)
        return _np(ll), _np(chi2), _np(g), _np(lam), _np(T), _np(model)
    ll, chi2, lam, T, model = stats(c, p, lp, F64, host=True, fams=fams)
    g = np.zeros(p.shape)
    base = p.detach().clone()
    for k in range(c["lens_cols"]):
        h = 1e-5 * max(1.0, float(base[:, k].abs().max()))
        out = []
        for sgn in (1.0, -1.0):
            q = base.clone()
            q[:, k] += sgn * h
            out.append(stats(c, q, helpers.struct_from_packed(c["phys"], q)["lens_mass"], F64, host=True, fams=fams)[0].detach())
        g[:, k] = _np((out[0] - out[1]) / (2 * h))
    return _np(ll), _np(chi2), g, _np(lam), _np(T), _np(model)


def yardstick_values(c):
    """The float32 restatement: ``(log_like, chi2, lambda, T, model)`` as float64 numpy arrays holding float32 arithmetic."""
    p, lp = PC.leaf(c, F32)
    return tuple(_np(v) for v in stats(c, p, lp, F32, host=True))


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
f = MC._f32
_C = dict(center_x=f(MC.OFF, MC.PIX + MC.OFF, -MC.PIX + MC.OFF), center_y=f(-MC.PIX + MC.OFF, MC.OFF, MC.OFF))
_E = dict(e1=f(0.1, -0.05, 0.15), e2=f(-0.05, 0.1, 0.02))
_SHEAR = {"gamma1": f(0.03, -0.02, 0.05), "gamma2": f(-0.02, 0.04, 0.01)}
# a cross of four images about a ring of radius 1.1 and a second family of three; lattice indices in units of MC.PIX = 0.1 arcsec
_QUAD = ((12, -10, 2, -3), (2, 3, -11, 10))
_TRIPLE = ((14, -7, 4), (-5, -8, 9))
# a second TNFW case beside the cross (`tnfw_cross`): images at four different radii, whose Fermat potentials lie 0.3 arcsec^2 apart
_SKEW = ((15, -8, 2, -3), (2, 3, -12, 7))


def _lens_sets():
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW, NFW_ELLIPSE
    from gigalens_amd.profiles.mass.piemd import DPIE, DPIS
    from gigalens_amd.profiles.mass.piep import DPIEP
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.tnfw import TNFW
    epl = MC.map_case("epl_shear|sie")["lens_params"][0]
    te, rc, rt = f(1.0, 1.1, 0.9), f(0.1, 0.15, 0.08), f(2.0, 1.5, 2.5)
    return {
        "epl": ([EPL(), Shear()], [epl, _SHEAR]),
        "sie": ([SIE()], [dict(theta_E=te, **_E, **_C)]),
        "nfw": ([NFW(), Shear()], [dict(Rs=f(2.0, 1.5, 2.5), alpha_Rs=f(1.2, 1.0, 1.4), **_C), _SHEAR]),
        "dpis": ([DPIS()], [dict(theta_E=te, r_core=rc, r_cut=rt, **_C)]),
        "dpie": ([DPIE()], [dict(theta_E=te, r_core=rc, r_cut=rt, **_C, **_E)]),
        "dpiep": ([DPIEP()], [dict(theta_E=te, Ra=rc, Rs=rt, **_C, **_E)]),
        "nfw_ellipse": ([NFW_ELLIPSE()], [dict(Rs=f(2.0, 1.5, 2.5), alpha_Rs=f(1.2, 1.0, 1.4), **_E, **_C)]),
        "tnfw": ([TNFW()], [dict(Rs=f(2.0, 1.5, 2.5), alpha_Rs=f(1.2, 1.0, 1.4), r_trunc=f(10.0, 8.0, 12.0), **_C)]),
    }


KIND_CASES = ("sie", "nfw", "dpis", "dpie", "dpiep", "nfw_ellipse", "tnfw", "tnfw_cross")
CASES = ("quad", "quad_given", "quad_nan", "two_fams") + KIND_CASES + ("cat", "b65")


def _family(kx, ky):
    x, y = PC.lattice(*kx), PC.lattice(*ky)
    return dict(T=np.ones(1), x=x, y=y, ex=np.full(x.shape, 0.01, np.float32), ey=np.full(x.shape, 0.0125, np.float32))


def with_delays(c, fams, rule=None, given=()):
    """``fams`` with the deterministic arrival times of this module; ``rule(f, j)``: False for an image without a measurement, None
    for a family without delays; ``given``: the families whose scale is given (``LAMBDA0 (1 + 0.05 f)``) instead of profiled."""
    p, lp = PC.leaf(c)
    rows = p.detach().numpy()
    out = []
    for k, fam in enumerate(fams):
        keep = [True] * fam["x"].size if rule is None else [rule(k, j) for j in range(fam["x"].size)]
        if keep[0] is None:
            out.append(dict(fam, delay=None, delay_err=None, scale=np.nan))
            continue
        psi = host_psi_model(c, rows, fam["x"], fam["y"]) if c.get("catalogue") is not None else None
        phi0 = fermat(c, p, lp, fam, F64, psi)[:, 0].detach().numpy()
        t = (LAMBDA0 * phi0 * np.asarray(PATTERN[:phi0.size])).astype(np.float32)
        s = np.asarray(ERRORS[:phi0.size], dtype=np.float32)
        t = np.where(keep, t, np.float32(np.nan))
        out.append(dict(fam, delay=t, delay_err=s, scale=float(np.float32(LAMBDA0 * (1 + 0.05 * k))) if k in given else np.nan))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """``dict(phys, mp, params, B, fams, lens_cols, catalogue)``; every family has ``delay`` / ``delay_err`` / ``scale``.  ``quad``: EPL +
    Shear, four images with four times, lambda profiled; ``quad_given``: lambda given; ``quad_nan``: one unmeasured image;
    ``two_fams``: a second family without delays; one case per further lens kind; ``cat``: a dPIE catalogue of 3 members beside an
    SIE; ``b65``: the quad and a triple with a given scale at batch 65."""
    from gigalens_amd.model import PhysicalModel
    sets = _lens_sets()
    catalogue, B = None, 3
    key = {"quad": "epl", "quad_given": "epl", "quad_nan": "epl", "two_fams": "epl", "b65": "epl", "cat": "sie", "tnfw_cross": "tnfw"}.get(name, name)
    lenses, lp = sets[key]
    lenses, lp = list(lenses), [dict(d) for d in lp]
    if name == "cat":
        from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
        catalogue = dict(lum=f(1.0, 0.6, 1.5), center_x=f(2.13, -1.87, 0.43), center_y=f(1.57, -2.07, 2.63), e1=f(0.1, -0.05, 0.0),
                         e2=f(0.0, 0.1, -0.1))
        lenses.append(DPIESubhalo(lum_star=1.0, galaxy_catalogue=catalogue))
        lp.append(dict(theta_E=f(0.15, 0.2, 0.1), r_core=f(0.05, 0.04, 0.06), r_cut=f(1.5, 2.0, 1.2)))
    if name == "b65":  # 65 samples: the three rows in turn, each value moved by up to 2 % with a phase of its own
        B = 65
        b = np.arange(B)
        lp = [{k: (np.asarray(v, np.float64)[b % 3] * (1 + 0.02 * np.sin(0.9 * b + i))).astype(np.float32)
               for i, (k, v) in enumerate(d.items())} for d in lp]
    mp = MC._mp([0.5] * len(lenses))
    assert mp.K == 1
    phys = PhysicalModel(lenses, [], [])
    params = {"lens_mass": lp, "lens_light": [], "source_light": []}
    c = dict(phys=phys, mp=mp, params=params, B=B, catalogue=catalogue, lens_cols=sum(len(l._native_params()) for l in lenses))
    fams = [_family(*(_SKEW if name == "tnfw" else _QUAD))]
    rule, given = None, ()
    if name == "quad_given":
        given = (0,)
    elif name == "quad_nan":
        rule = lambda k, j: j != 2
    elif name == "two_fams":
        fams.append(_family(*_TRIPLE))
        rule = lambda k, j: True if k == 0 else None
    elif name == "b65":
        fams.append(_family(*_TRIPLE))
        given = (1,)
    return dict(c, fams=with_delays(dict(c, fams=fams), fams, rule, given))


def centroids(c):
    """The keyword arguments of ``ForwardProbModel`` that carry the families of case ``c`` with their delays."""
    from gigalens_amd.simulator import LensSimulator
    dist = [None if np.isnan(fm["scale"]) else fm["scale"] / LensSimulator.DAYS_PER_MPC_ARCSEC2 for fm in c["fams"]]
    return dict(centroids_x=[fm["x"] for fm in c["fams"]], centroids_y=[fm["y"] for fm in c["fams"]],
                centroids_errors_x=[fm["ex"] for fm in c["fams"]], centroids_errors_y=[fm["ey"] for fm in c["fams"]],
                centroids_time_delays=[fm["delay"] for fm in c["fams"]], centroids_time_delays_errors=[fm["delay_err"] for fm in c["fams"]],
                time_delay_distances=dist)


def n_delay(c):
    return int(sum(0 if fm["delay"] is None else np.count_nonzero(~np.isnan(fm["delay"])) for fm in c["fams"]))


def nan_err(got, ref):
    """``MC.rel_err`` over the finite entries of ``ref``; the NaN patterns must agree."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    return MC.rel_err(got[ok], ref[ok]) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def data(name):
    """``(case, ref, yard)`` -- computed once and shared (left unchanged).  ``ref``: ``log_like``, ``chi2``, ``grad``, ``scale``,
    ``offset`` and ``model`` in float64; ``yard``: the float32 restatement's deviation from them, relative to their largest value."""
    c = case(name)
    ll, chi2, g, lam, T, model = loglike_grad(c)
    ll32, chi232, lam32, T32, model32 = yardstick_values(c)
    ref = dict(log_like=ll, chi2=chi2, grad=g, scale=lam, offset=T, model=model)
    yard = dict(log_like=MC.rel_err(ll32, ll), chi2=MC.rel_err(chi232, chi2), scale=nan_err(lam32, lam), offset=nan_err(T32, T),
                model=nan_err(model32, model))
    return c, ref, yard
