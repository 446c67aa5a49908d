"""Float64 restatement of the image-plane position likelihood of image families (csrc/gl_imgplane.hip.h) and the cases of its tests:
tests/test_imgplane_host.py pins the restatement without a GPU, tests/test_gpu_imgplane.py runs the kernels against it.

The deflection is ``oracle.ref_torch.mass_deriv`` and the Hessian ``oracle.ref_torch.mass_hessian`` (the dPIS override with its
convergence excess included) summed over the lenses, on the packed leaf of ``mp_positions_cases.leaf``.  For family f with deflection
scale c_f, ``beta = theta - c_f sum alpha`` and ``A = I - c_f H``; its source beta_f is given or the barycentre of its back-traced
observed images.  The predicted image of observed image j is the root of ``beta(theta) = beta_f`` that Newton reaches from
``theta_obs_j`` -- the iteration of the kernel: steps of at most ``cap_j`` until ``|beta_f - beta| <= tol`` or ``max_iter`` of them,
then one polishing step kept when its residual is not larger -- and is lost when Newton has not converged, the point is not finite,
``|theta_pred - theta_obs_j| > cap_j`` or ``u_j`` is not finite.  With ``r_j = theta_pred_j - theta_obs_j``:

    chi2 = sum_j min(|r_j|^2, cap_j^2)/sigma_j^2,   log_like = -chi2/2 - sum_j log(2 pi sigma_j^2),
    u_j = J(theta_pred_j)^-T r_j/sigma_j^2 (0 where lost),  J = d beta / d theta = I - c_f d alpha / d theta,
    d log_like / d p = sum_j u_j . d beta/d p at theta_pred_j - (sum_{j in f} u_j) . d beta_f/d p,   d log_like / d beta_f = -sum_{j in f} u_j

(the implicit function theorem; ``torch.autograd`` differentiates ``beta`` at fixed points only).  ``A`` steers the Newton steps, as in the
solver; the gradient takes ``J``, the derivative of the deflection alone: the reference's analytic dPIS Hessian carries a convergence
excess that no deflection has, and only ``J`` makes the gradient the derivative of the value (J = A unless a dPIS takes part).  Every function takes ``dtype``:
float64 with ``tol = 1e-11`` is the reference, the same code in float32 on the CPU with the kernel's default ``tol`` is the yardstick."""
import functools

import numpy as np
import torch

from tests import mp_positions_cases as PC
from tests import multilens_cases as MC

F64, F32 = MC.F64, MC.F32
B = 3
TOL64 = 1e-11
IMAGE_TOL_EPS = 8.0  # LensSimulator.IMAGE_TOL_EPS


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def families(fam):
    """``gigalens_amd.model.ImageFamilies`` of ``fam = dict(x, y, sigma[, scales, max_shift])`` (host-side tables, no GPU)."""
    from gigalens_amd.model import ImageFamilies
    return ImageFamilies(fam["x"], fam["y"], fam["sigma"], scales=fam.get("scales"), max_shift=fam.get("max_shift"))


def default_tol(fams):
    return IMAGE_TOL_EPS * float(np.finfo(np.float32).eps) * fams.max_coordinate


def lens_eval(phys, lp, x, y, c, want_h=True):
    """``(beta_x, beta_y, A, J)`` at ``x, y`` ``[n, B]`` with scales ``c`` ``[n, 1]``; differentiable in ``lp`` (one dict of ``[B]`` tensors
    per lens), not in the points.  ``A = I - c H`` (``[xx, xy, yx, yy]``) with ``H = mass_hessian``, the Hessian of the lens maps -- the dPIS
    override with its convergence excess -- steers the Newton steps; ``J = I - c d alpha / d theta``, the derivative of ``mass_deriv``
    itself, is the Jacobian of beta that the implicit function theorem needs (J = A unless a dPIS takes part).  Both None without
    ``want_h``."""
    from oracle import ref_torch as ref
    consts = MC._consts(phys, x.dtype)
    ax, ay, H, D = 0.0, 0.0, [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]
    for lens, p, k in zip(phys.lenses, lp, consts):
        fx, fy = ref.mass_deriv(lens, x, y, **p, **k)
        ax, ay = ax + fx, ay + fy
        if want_h:
            with torch.enable_grad():
                xs, ys = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
                H = [t + h.detach() for t, h in zip(H, ref.mass_hessian(lens, xs, ys, **p, **k))]
                gx, gy = ref.mass_deriv(lens, xs, ys, **p, **k)
                d = torch.autograd.grad(gx.sum(), [xs, ys], retain_graph=True) + torch.autograd.grad(gy.sum(), [xs, ys])
                D = [t + h.detach() for t, h in zip(D, d)]
    if not want_h:
        return x - c * ax, y - c * ay, None, None
    return x - c * ax, y - c * ay, [1 - c * H[0], -c * H[1], -c * H[2], 1 - c * H[3]], [1 - c * D[0], -c * D[1], -c * D[2], 1 - c * D[3]]


def _t(v, dtype):
    return torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)


def solve(phys, lp, fams, dtype, source=None, tol=None, max_iter=30):
    """Newton from every observed image, vectorised over ``[J, nb]``: ``dict(x, y [J, nb], lost [J, nb] bool, u [2, J, nb], chi2_j
    [J, nb], det [J, nb], src [2, F, nb])`` tensors in ``dtype`` (nothing differentiable)."""
    lp = [{k: v.detach() for k, v in d.items()} for d in lp]
    nb = max(int(v.numel()) for d in lp for v in d.values())
    J, off = fams.J, fams.offsets
    ox, oy = _t(fams.x, dtype)[:, None].repeat(1, nb), _t(fams.y, dtype)[:, None].repeat(1, nb)
    c, cap, sg = _t(fams.scales, dtype)[:, None], _t(fams.max_shift, dtype)[:, None], _t(fams.sigma, dtype)[:, None]
    fam_of = np.repeat(np.arange(fams.F), fams.counts)
    with torch.no_grad():
        if source is None:
            bx, by, _, _ = lens_eval(phys, lp, ox, oy, c, want_h=False)
            src = torch.stack([torch.stack([torch.stack([v[k] for k in range(off[f], off[f + 1])]).sum(0) / float(off[f + 1] - off[f])
                                            for f in range(fams.F)]) for v in (bx, by)])  # summed in image order
        else:
            # [2, B, F] -> [2, F, B]; float32 values, as the entry holds them (a tensor is taken as it is)
            src = source if torch.is_tensor(source) else torch.as_tensor(np.asarray(source, dtype=np.float32))
            src = src.to(dtype).permute(0, 2, 1)
        sx, sy = src[0][fam_of], src[1][fam_of]
        tol = (TOL64 if dtype == F64 else default_tol(fams)) if tol is None else tol
        x, y = ox.clone(), oy.clone()
        bx, by, A, Jt = lens_eval(phys, lp, x, y, c)
        rx, ry = sx - bx, sy - by
        r2 = rx * rx + ry * ry
        done = torch.zeros_like(x, dtype=torch.bool)
        ok = torch.zeros_like(done)
        for it in range(max_iter + 1):
            conv = r2 <= tol * tol
            done = done | (~conv & (it == max_iter))
            active = ~done
            if not bool(active.any()):
                break
            det = A[0] * A[3] - A[1] * A[2]
            dx, dy = (A[3] * rx - A[1] * ry) / det, (A[0] * ry - A[2] * rx) / det
            ln = torch.sqrt(dx * dx + dy * dy)
            bad = active & ~torch.isfinite(ln)
            ok = torch.where(bad, conv, ok)
            done = done | bad
            active = active & ~bad
            f = torch.where(ln <= cap, torch.ones_like(ln), cap / ln)
            nx, ny = x + dx * f, y + dy * f
            nbx, nby, nA, nJ = lens_eval(phys, lp, torch.where(active, nx, ox), torch.where(active, ny, oy), c)
            nrx, nry = sx - nbx, sy - nby
            nr2 = nrx * nrx + nry * nry
            polish = active & conv
            take = (polish & (nr2 <= r2)) | (active & ~conv)
            x, y = torch.where(take, nx, x), torch.where(take, ny, y)
            A = [torch.where(take, n_, o_) for n_, o_ in zip(nA, A)]
            Jt = [torch.where(take, n_, o_) for n_, o_ in zip(nJ, Jt)]
            step = active & ~conv
            rx, ry, r2 = torch.where(step, nrx, rx), torch.where(step, nry, ry), torch.where(step, nr2, r2)
            ok = ok | polish
            done = done | polish
        det = Jt[0] * Jt[3] - Jt[1] * Jt[2]
        dx, dy = x - ox, y - oy
        d2 = dx * dx + dy * dy
        ux, uy = ((Jt[3] * dx - Jt[2] * dy) / det) / sg ** 2, ((Jt[0] * dy - Jt[1] * dx) / det) / sg ** 2
        good = ok & torch.isfinite(x) & torch.isfinite(y) & (d2 <= cap * cap) & torch.isfinite(ux) & torch.isfinite(uy)
        zero = torch.zeros_like(ux)
        u = torch.stack([torch.where(good, ux, zero), torch.where(good, uy, zero)])
        chi2_j = torch.where(good, torch.minimum(d2, cap * cap), (cap * cap).expand_as(d2)) / sg ** 2
    return dict(x=x, y=y, lost=~good, u=u, chi2_j=chi2_j, det=det, src=src)


def loglike_grad(phys, rows, fams, dtype=F64, source=None, tol=None, max_iter=30):
    """``dict(log_like [B], chi2 [B], n_lost [B], predicted [2, J, B] (NaN where lost), lost [J, B], grad [B, P], grad_source [2, B, F],
    det [J, B])`` as float64 numpy arrays holding ``dtype`` arithmetic."""
    p, lp = PC.leaf(dict(phys=phys), dtype, packed=rows)
    s = solve(phys, lp, fams, dtype, source=source, tol=tol, max_iter=max_iter)
    c = _t(fams.scales, dtype)[:, None]
    off = fams.offsets
    ox, oy = _t(fams.x, dtype)[:, None].expand_as(s["x"]), _t(fams.y, dtype)[:, None].expand_as(s["y"])
    px, py = torch.where(s["lost"], ox, s["x"]), torch.where(s["lost"], oy, s["y"])
    bx, by, _, _ = lens_eval(phys, lp, px, py, c, want_h=False)  # (a lost image: u = 0 at its observed point)
    tot = (s["u"][0] * bx + s["u"][1] * by).sum()
    su = torch.stack([torch.stack([s["u"][a][off[f]:off[f + 1]].sum(0) for f in range(fams.F)]) for a in range(2)])  # [2, F, B]
    if source is None:
        obx, oby, _, _ = lens_eval(phys, lp, ox, oy, c, want_h=False)
        for f in range(fams.F):
            tot = tot - (su[0][f] * obx[off[f]:off[f + 1]].mean(0) + su[1][f] * oby[off[f]:off[f + 1]].mean(0)).sum()
    (g,) = torch.autograd.grad(tot, p, allow_unused=True)
    g = torch.zeros_like(p) if g is None else g
    chi2 = s["chi2_j"].double().sum(0)
    nan = torch.full_like(s["x"], float("nan"))
    pred = torch.stack([torch.where(s["lost"], nan, s["x"]), torch.where(s["lost"], nan, s["y"])])
    n = lambda t: t.detach().double().numpy()
    return dict(log_like=n(-0.5 * chi2 - fams.norm), chi2=n(chi2), n_lost=s["lost"].sum(0).numpy(), predicted=n(pred), lost=s["lost"].numpy(),
                grad=n(g), grad_source=n(-su.permute(0, 2, 1)), det=n(s["det"]))


def loglike_only(phys, rows, fams, source=None):
    """float64 ``log_like [B]`` (numpy) of the rows: what the finite differences of tests/test_imgplane_host.py difference."""
    _, lp = PC.leaf(dict(phys=phys), F64, packed=rows)
    s = solve(phys, lp, fams, F64, source=source)
    return (-0.5 * s["chi2_j"].sum(0) - fams.norm).numpy()


def find_images(phys, row, sx, sy, c=1.0, half=2.5, n=26, tol=1e-12):
    """Every image of the source ``(sx, sy)`` behind the lenses of ONE packed row, float64: Newton from an ``n x n`` lattice of starts over
    ``[-half, half]^2``, the converged roots merged; sorted by angle.  ``[(x, y, mu)]`` numpy ``[k, 3]``."""
    _, lp = PC.leaf(dict(phys=phys), F64, packed=np.asarray(row, dtype=np.float64)[None, :])
    lp = [{k: v.detach() for k, v in d.items()} for d in lp]
    g = np.linspace(-half, half, n) + 0.0137  # (off every lens centre)
    x = torch.as_tensor(np.repeat(g, n))[:, None].clone()
    y = torch.as_tensor(np.tile(g, n))[:, None].clone()
    cc = torch.full_like(x, float(c))
    step = 2.0 * half / n
    with torch.no_grad():
        for _ in range(60):
            bx, by, _, A = lens_eval(phys, lp, x, y, cc)
            rx, ry = sx - bx, sy - by
            det = A[0] * A[3] - A[1] * A[2]
            dx, dy = (A[3] * rx - A[1] * ry) / det, (A[0] * ry - A[2] * rx) / det
            ln = torch.sqrt(dx * dx + dy * dy)
            f = torch.where(ln <= step, torch.ones_like(ln), step / ln)
            x, y = x + dx * f, y + dy * f
        bx, by, _, A = lens_eval(phys, lp, x, y, cc)
        res = torch.hypot(sx - bx, sy - by)[:, 0].numpy()
        mu = (1.0 / (A[0] * A[3] - A[1] * A[2]))[:, 0].numpy()
    x, y = x[:, 0].numpy(), y[:, 0].numpy()
    out = []
    for k in np.flatnonzero(np.isfinite(res) & (res <= tol) & (np.hypot(x, y) <= 2 * half)):
        if all(np.hypot(x[k] - o[0], y[k] - o[1]) > 1e-6 for o in out):
            out.append((x[k], y[k], mu[k]))
    out.sort(key=lambda o: np.arctan2(o[1], o[0]))
    return np.asarray(out, dtype=np.float64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
CASES = ("epl_shear_quad", "two_planes", "dpis_nfw", "catalogue")
SIGMA = 0.02
MU_MIN = 0.05   # images fainter than this (the central image of a cored lens) are no part of a family
# the floor of min |det A| at the predicted images each case states (tests/test_imgplane_host.py asserts it on the reference)
DET_FLOOR = {"epl_shear_quad": 0.05, "two_planes": 0.05, "dpis_nfw": 0.05, "catalogue": 0.05}
QUAD_IMAGES = ((1.1346, -0.4065), (0.3938, 1.1371), (-0.1350, -1.2019), (-1.1134, 0.1403))


@functools.lru_cache(maxsize=None)
def lenses(name):
    """``(phys, truth row [P] float32, sources [(x, y, scale)])``."""
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.profiles.mass.piemd import DPIS
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    if name == "epl_shear_quad":
        ls = [EPL(), Shear()]
        truth = [dict(theta_E=1.2, gamma=2.1, e1=0.2, e2=-0.1, center_x=0.02, center_y=-0.03), dict(gamma1=0.04, gamma2=-0.02)]
        srcs = [(0.04, -0.01, 1.0)]
    elif name == "two_planes":  # two families on planes of their own
        ls = [SIE(), Shear()]
        truth = [dict(theta_E=1.0, e1=0.15, e2=-0.05, center_x=0.01, center_y=0.02), dict(gamma1=0.03, gamma2=0.02)]
        srcs = [(0.05, 0.03, 1.0), (-0.02, 0.03, 0.7)]
    elif name == "dpis_nfw":  # the dPIS convergence excess in A
        ls = [DPIS(), NFW()]
        truth = [dict(theta_E=1.0, r_core=0.1, r_cut=3.0, center_x=0.0, center_y=0.0), dict(Rs=2.0, alpha_Rs=0.6, center_x=0.05, center_y=-0.03)]
        srcs = [(0.12, 0.07, 1.0)]
    elif name == "catalogue":  # a dPIE ScalingRelation population beside the main deflector
        ls = [SIE(), DPIESubhalo(lum_star=1.0, galaxy_catalogue=workloads.galaxy_catalogue(3, half_width=3.0, seed=4))]
        truth = [dict(theta_E=1.1, e1=-0.1, e2=0.08, center_x=0.02, center_y=-0.01), dict(theta_E=0.25, r_core=0.2, r_cut=2.0)]
        srcs = [(0.06, 0.04, 1.0)]
    elif name == "sis":
        ls, truth, srcs = [SIS()], [dict(theta_E=1.0, center_x=0.0, center_y=0.0)], []
    else:
        raise KeyError(name)
    phys = PhysicalModel(ls, [], [])
    row = np.asarray([d[k] for lens, d in zip(ls, truth) for k in lens.params], dtype=np.float32)
    return phys, row, srcs


def spread(name, row, nb, seed):
    """``nb`` rows around ``row``: 1 % on every parameter's scale, 0.005 on the centres, ellipticities and shears."""
    phys = lenses(name)[0]
    r = np.random.default_rng(seed)
    names = [k for lens in phys.lenses for k in lens.params]
    add = np.array([k.startswith(("center", "e1", "e2", "gamma1", "gamma2")) for k in names])
    d = r.standard_normal((nb, row.size))
    return np.where(add[None, :], row[None, :] + 0.005 * d, row[None, :] * (1 + 0.01 * d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, nb=B, noise=SIGMA):
    """``dict(phys, rows [nb, P] float32, fam, truth_images [per family (k, 3)])``: the families are the images (|mu| >= MU_MIN) of the
    case's sources behind the TRUTH row, plus N(0, noise) rounded to float32; the rows are drawn around the truth."""
    phys, row, srcs = lenses(name)
    r = np.random.default_rng(5)
    xs, ys, truth_images = [], [], []
    for sx, sy, c in srcs:
        im = find_images(phys, row, sx, sy, c)
        im = im[np.abs(im[:, 2]) >= MU_MIN]
        truth_images.append(im)
        xs.append((im[:, 0] + noise * r.standard_normal(im.shape[0])).astype(np.float32))
        ys.append((im[:, 1] + noise * r.standard_normal(im.shape[0])).astype(np.float32))
    fam = dict(x=xs, y=ys, sigma=SIGMA, scales=[c for _, _, c in srcs])
    return dict(phys=phys, rows=spread(name, row, nb, 6), fam=fam, truth_images=truth_images, truth=row)


@functools.lru_cache(maxsize=None)
def data(name, nb=B, noise=SIGMA):
    """``(case, ImageFamilies, ref, yard)`` -- computed once and shared (left unchanged).  ``ref``: the float64 ``loglike_grad``; ``yard``:
    the float32 restatement's deviation from it -- ``MC.rel_err`` for ``log_like``, ``chi2`` and ``predicted``, ``PC.grad_gate`` units for
    the gradient."""
    c = case(name, nb, noise)
    fams = families(c["fam"])
    ref = loglike_grad(c["phys"], c["rows"], fams, F64)
    r32 = loglike_grad(c["phys"], c["rows"], fams, F32)
    return c, fams, ref, yardstick(r32, ref)


def yardstick(r32, ref):
    yard = {k: MC.rel_err(np.nan_to_num(r32[k]), np.nan_to_num(ref[k])) for k in ("log_like", "chi2", "predicted")}
    yard["grad"] = PC.grad_gate(r32["grad"], ref["grad"])
    return yard


# ---- launch edges: (images, samples, families) with J B at the edges of a wave -------------------------------------------------
EDGES = {"63": (3, 21, 1), "64": (4, 16, 1), "65": (5, 13, 2), "129": (3, 43, 3)}
EDGE_CAP = 0.3


@functools.lru_cache(maxsize=None)
def edge_data(cfg):
    """``dict(case, fams, ref, yard, source)`` on the lenses of ``two_planes``, lanes = (image, sample) with the sample fastest:
    63 = one family of 3 images x 21 samples; 64 = one family of 4 x 16; 65 = families of 2 and 3 (the second on the plane of scale 0.7,
    its lanes 26 .. 64 straddle the wave boundary) x 13; 129 = three one-image families with explicit sources and ``max_shift`` given
    x 43 (the lanes 43 .. 85 of the second image straddle it).  ``source``: ``[2, nb, F]`` or None (the barycentre)."""
    J, nb, F = EDGES[cfg]
    base = case("two_planes")
    phys, row, srcs = lenses("two_planes")
    x, y = base["fam"]["x"], base["fam"]["y"]
    source = None
    if cfg == "63":
        fam = dict(x=[x[0][:3]], y=[y[0][:3]], sigma=SIGMA, scales=[1.0])
    elif cfg == "64":
        fam = dict(x=[x[0]], y=[y[0]], sigma=SIGMA, scales=[1.0])
    elif cfg == "65":
        fam = dict(x=[x[0][:2], x[1][:3]], y=[y[0][:2], y[1][:3]], sigma=[SIGMA, 1.5 * SIGMA], scales=[1.0, 0.7])
    else:
        fam = dict(x=[x[0][:1], x[0][1:2], x[1][:1]], y=[y[0][:1], y[0][1:2], y[1][:1]], sigma=SIGMA, scales=[1.0, 1.0, 0.7], max_shift=EDGE_CAP)
        r = np.random.default_rng(8)
        true = np.array([[srcs[0][0], srcs[0][0], srcs[1][0]], [srcs[0][1], srcs[0][1], srcs[1][1]]])  # [2, F]
        source = (true[:, None, :] + 0.003 * r.standard_normal((2, nb, 3))).astype(np.float32)
    c = dict(phys=phys, rows=spread("two_planes", row, nb, 9), fam=fam)
    fams = families(fam)
    ref = loglike_grad(phys, c["rows"], fams, F64, source=source)
    r32 = loglike_grad(phys, c["rows"], fams, F32, source=source)
    yard = yardstick(r32, ref)
    yard["grad_source"] = MC.rel_err(r32["grad_source"], ref["grad_source"]) if source is not None else 0.0
    return dict(case=c, fams=fams, ref=ref, yard=yard, source=source)


# ---- the singular isothermal sphere, closed form ------------------------------------------------------------------------
SIS_B, SIS_SIGMA = 0.3, 0.05
SIS_DELTA = np.array([[0.03, -0.02], [-0.025, 0.035]])  # delta_+ and delta_- (x, y)


def sis_case(b=SIS_B, nb=B, delta=SIS_DELTA):
    """theta_E = 1 at the origin, explicit source ``(b, 0)``: one family of two images observed at ``(SIS_B +- 1, 0) + delta`` (the data do
    not move with ``b``).  ``dict(phys, rows, fam, source_x, source_y [nb, 1])``; every sample is the same row."""
    phys, row, _ = lenses("sis")
    obs = (np.array([[SIS_B + 1.0, 0.0], [SIS_B - 1.0, 0.0]]) + np.asarray(delta)).astype(np.float32)
    fam = dict(x=[obs[:, 0]], y=[obs[:, 1]], sigma=SIS_SIGMA)
    return dict(phys=phys, rows=np.repeat(row[None, :], nb, axis=0), fam=fam, source_x=np.full((nb, 1), b, dtype=np.float32),
                source_y=np.zeros((nb, 1), dtype=np.float32))


def sis_source(c):
    """``[2, nb, 1]``: the explicit sources of ``sis_case`` in the layout of ``loglike_grad``."""
    return np.stack([c["source_x"], c["source_y"]])


def sis_closed_form(fams, b=SIS_B):
    """``dict(predicted [2, 2], chi2, grad [3], scale [3])`` of ``sis_case`` from the observed float32 positions, in float64 (``b`` as
    float32, as the entry holds it); ``grad`` = d log_like / d (theta_E, source_x, source_y).  With delta = theta_obs - root,
    ``chi2 = sum |delta|^2/sigma^2``, ``d log_like/d theta_E = (delta_+x - delta_-x)/sigma^2``, ``grad_source_x = (delta_+x + delta_-x)/sigma^2``,
    ``grad_source_y = sum delta_y/(sigma^2 (1 - theta_E/|b +- theta_E|))``.
    ``scale``: the sum of the absolute values of the two images' terms in each element.  The predicted positions are float32 numbers, so
    each image's term carries their rounding relative to ITSELF; where the two terms cancel (source_x: 12 - 10) the sum is held to
    the scale of its terms, not to its own."""
    b = float(np.float32(b))
    ox, oy = fams.x.astype(np.float64), fams.y.astype(np.float64)
    root = np.array([b + 1.0, b - 1.0])
    dx, dy = ox - root, oy
    w = 1.0 / float(fams.sigma[0]) ** 2
    ty = dy * w / (1.0 - 1.0 / np.abs(root))
    return dict(predicted=np.stack([root, np.zeros(2)]), chi2=float(((dx ** 2 + dy ** 2) * w).sum()),
                grad=np.array([(dx[0] - dx[1]) * w, dx.sum() * w, ty.sum()]),
                scale=np.array([np.abs(dx).sum() * w, np.abs(dx).sum() * w, np.abs(ty).sum()]))


# ---- one short MAP run on the noise-free quad ---------------------------------------------------------------------------
MAP_STEPS, MAP_LR, MAP_BS, MAP_FACTOR = 40, 1e-3, 2, 20.0
MAP_PRIOR = {"theta_E": 0.3, "gamma": 0.1, "e1": 0.1, "e2": 0.1, "center_x": 0.1, "center_y": 0.1, "gamma1": 0.05, "gamma2": 0.05}


@functools.lru_cache(maxsize=None)
def map_case():
    """``dict(phys, fams, truth [P], start [MAP_BS, P] float32, names [P])``: the noise-free images of ``epl_shear_quad`` and rows that
    start with theta_E 2 % high (and centres a little apart, so the samples differ).  The prior is Normal around the truth with the
    widths ``MAP_PRIOR`` (theta_E: LogNormal, i.e. Normal in z = log theta_E)."""
    c = case("epl_shear_quad", B, 0.0)
    phys, row, _ = lenses("epl_shear_quad")
    names = [k for lens in phys.lenses for k in lens.params]
    start = np.repeat(row[None, :].astype(np.float64), MAP_BS, axis=0)
    start[:, names.index("theta_E")] *= 1.02
    start[:, names.index("center_x")] += np.linspace(-0.004, 0.004, MAP_BS)
    return dict(phys=phys, fams=families(c["fam"]), truth=row, start=start.astype(np.float32), names=names)


@functools.lru_cache(maxsize=None)
def map_reference():
    """``(chi2 at the start [MAP_BS], chi2 after MAP_STEPS steps [MAP_BS])`` of the float64 restatement under ``gigalens_amd.inference.Adam``
    on the CPU: z = the packed row with log theta_E, loss = mean(-log_prob / (2 J)) as ``ModellingSequence.MAP`` forms it, log_prob =
    log_like + the Normal prior in z."""
    from gigalens_amd.inference import Adam
    m = map_case()
    k_te = m["names"].index("theta_E")
    mu = m["truth"].astype(np.float64).copy()
    mu[k_te] = np.log(mu[k_te])
    sd = np.array([MAP_PRIOR[k] for k in m["names"]])
    z = torch.as_tensor(m["start"].astype(np.float64))
    z[:, k_te] = torch.log(z[:, k_te])
    opt = Adam(lr=MAP_LR)
    denom = 2.0 * m["fams"].J * MAP_BS
    chi2 = []
    for step in range(MAP_STEPS + 1):
        p = z.numpy().copy()
        p[:, k_te] = np.exp(p[:, k_te])
        r = loglike_grad(m["phys"], p, m["fams"], F64)
        chi2.append(r["chi2"])
        if step == MAP_STEPS:
            break
        g = r["grad"].copy()
        g[:, k_te] *= p[:, k_te]
        g -= (z.numpy() - mu) / sd ** 2
        opt.step(z, torch.as_tensor(g), -1.0 / denom)
    return chi2[0], chi2[-1]
