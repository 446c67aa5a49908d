"""Float64 restatement of the Hessian VJP and of the weak-lensing reduced-shear likelihood (csrc/gl_hessian_vjp.hip.h) and the cases
of their tests: tests/test_shear_host.py pins the restatement without a GPU, tests/test_gpu_hessian_vjp.py and tests/test_gpu_shear.py
run the kernels against it.

The Hessian is ``oracle.ref_torch.mass_hessian`` summed over the lenses -- ``lens.hessian`` as the reference resolves it, the dPIS
override with its convergence excess included -- on the packed leaf of ``mp_positions_cases.leaf``, so that ``torch.autograd``
differentiates with respect to the packed parameters.  With the conventions of ``LensSimulator.convergence`` / ``.shear`` and a
deflection scale ``c`` per galaxy:

    kappa = c (f_xx + f_yy)/2,  gamma1 = c (f_xx - f_yy)/2,  gamma2 = c f_xy,  g = (gamma1 + i gamma2)/(1 - kappa),
    g^ = g where |g|^2 <= 1, g/|g|^2 (= 1/g*) otherwise,
    chi2 = sum [(e1 - g^1)^2 + (e2 - g^2)^2]/s^2,  log_like = -1/2 (chi2 + 2 sum log(2 pi s^2)).

Every function takes ``dtype``: float64 is the reference, the same code in float32 on the CPU is the yardstick."""
import functools

import numpy as np
import torch

from tests import helpers as H
from tests import mp_positions_cases as PC
from tests import multilens_cases as MC
from tests.potential_cases import KINDS, points_away, row_to_kwargs

F64, F32 = MC.F64, MC.F32
B = 3
YARD_CAP = 5e-2          # on 4 x the float32 yardstick of a Hessian-VJP draw (tests/test_gpu_beta_vjp.py)
GATE_CAP = 100.0         # the same cap on the likelihood's gradient, in units of PC.grad_gate (5e-2 / PC.GRAD_RTOL)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def hessian(phys, lp, x, y):
    """``[f_xx, f_xy, f_yx, f_yy]`` summed over the lenses of ``phys`` at ``x, y`` (``(n, B)`` tensors; their dtype is the arithmetic's);
    ``lp``: one dict of ``[B]`` tensors per lens, differentiable."""
    from oracle import ref_torch as ref
    consts = MC._consts(phys, x.dtype)
    tot = [0.0, 0.0, 0.0, 0.0]
    for lens, p, c in zip(phys.lenses, lp, consts):
        xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)  # (mass_hessian differentiates the deflection in them)
        tot = [t + h for t, h in zip(tot, ref.mass_hessian(lens, xs, ys, **p, **c))]
    return tot


def _pts(v, dtype, nb=B):
    t = torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)
    return t[:, None].repeat(1, nb) if t.dim() == 1 else t


def hessian_vjp(phys, rows, x, y, cot, dtype=F64):
    """``[B, P]`` (float64 numpy holding ``dtype`` arithmetic): the gradient of ``sum_pt cot . (f_xx, f_xy, f_yx, f_yy)`` with respect to the
    packed rows ``rows``; ``x, y`` ``[n]`` or ``[n, B]`` and ``cot`` ``[4, n, B]`` float32 values."""
    nb = np.asarray(rows).shape[0]
    p, lp = PC.leaf(dict(phys=phys), dtype, packed=rows)
    f = hessian(phys, lp, _pts(x, dtype, nb), _pts(y, dtype, nb))
    ct = torch.as_tensor(np.asarray(cot, dtype=np.float32)).to(dtype)
    tot = sum((ct[k] * f[k]).sum() for k in range(4))
    (g,) = torch.autograd.grad(tot, p)
    return g.double().numpy()


def shear_fields(phys, lp, x, y, scales, dtype):
    """``(g^1, g^2, kappa, |g|)`` ``[N, nb]`` tensors at the galaxies ``x, y`` ``[N]`` with scales ``[N]`` (differentiable in ``lp``)."""
    nb = max([int(v.numel()) for d in lp for v in d.values()] + [1])
    f = hessian(phys, lp, _pts(x, dtype, nb), _pts(y, dtype, nb))
    c = torch.as_tensor(np.asarray(scales, dtype=np.float32)).to(dtype)[:, None]
    kappa, g1, g2 = c * (f[0] + f[3]) / 2, c * (f[0] - f[3]) / 2, c * f[1]
    r1, r2 = g1 / (1 - kappa), g2 / (1 - kappa)
    n2 = r1 * r1 + r2 * r2
    weak = n2 <= 1
    n2s = torch.where(weak, torch.ones_like(n2), n2)  # (the branch not taken must not divide by |g|^2 = 0)
    return torch.where(weak, r1, r1 / n2s), torch.where(weak, r2, r2 / n2s), kappa, torch.sqrt(n2)


def loglike(phys, lp, cat, dtype=F64):
    """``(log_like [nb], chi2 [nb], g^ [2, N, nb])`` tensors of the catalogue ``cat = dict(x, y, e1, e2, sigma, scales)``."""
    h1, h2, _, _ = shear_fields(phys, lp, cat["x"], cat["y"], cat["scales"], dtype)
    t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)[:, None]
    s = t(cat["sigma"])
    chi2 = (((t(cat["e1"]) - h1) ** 2 + (t(cat["e2"]) - h2) ** 2) / s ** 2).sum(dim=0)
    norm = 2 * torch.log(2 * np.pi * s ** 2).sum()
    return -0.5 * (chi2 + norm), chi2, torch.stack([h1, h2])


def loglike_grad(phys, rows, cat, dtype=F64):
    """``dict(log_like [B], chi2 [B], model_g [2, N, B], grad [B, P])`` as float64 numpy arrays holding ``dtype`` arithmetic."""
    p, lp = PC.leaf(dict(phys=phys), dtype, packed=rows)
    ll, chi2, g = loglike(phys, lp, cat, dtype)
    (grad,) = torch.autograd.grad(ll.sum(), p)
    return dict(log_like=ll.detach().double().numpy(), chi2=chi2.detach().double().numpy(), model_g=g.detach().double().numpy(),
                grad=grad.double().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# Hessian-VJP draws
# ---------------------------------------------------------------------------------------------------------------------
N_PTS = [1, 63, 64, 65, 257, 4161]  # one lane; the edges of a wave; several workgroups; more than 64 partials for the sum
# label -> (kind, Rs range or None, r_min, seed).  The NFW family is drawn in two regimes: every point well inside the scale radius,
# and every point outside it -- where a point meets the X = 1 branch the float32 oracle is useless as a yardstick.
DRAWS = {
    "EPL": ("EPL", None, 0.2, 31),
    "SIE": ("SIE", None, 0.2, 31),
    "SHEAR": ("SHEAR", None, 0.2, 31),
    "SIS": ("SIS", None, 0.2, 31),
    "dPIS": ("dPIS", None, 0.2, 33),
    "dPIE": ("dPIE", None, 0.2, 31),
    "dPIEP": ("dPIEP", None, 0.2, 33),
    "NFW inside": ("NFW", (14.0, 25.0), 1.0, 32),
    "NFW outside": ("NFW", (0.3, 0.45), 1.5, 32),
    "NFW_ELLIPSE inside": ("NFW_ELLIPSE", (14.0, 25.0), 1.0, 32),
    "NFW_ELLIPSE outside": ("NFW_ELLIPSE", (0.3, 0.45), 1.5, 31),
    # (seed 35 was replaced: its float32 yardstick at one point is 7.4e-3 on one host CPU and 2.0e-2 on another, over the cap)
    "TNFW inside": ("TNFW", (14.0, 25.0), 1.0, 37),
    "TNFW outside": ("TNFW", (0.3, 0.45), 1.5, 32),
    # (seeds 31 and 32 were replaced: float32 yardsticks of 0.035 and 3.1e-3 at 4161 points -- the analytic dPIE Hessian of the
    # nearly round members cancels in float32 -- over the cap, or under it by less than the spread between host CPUs)
    "catalogue": ("catalogue", None, 0.2, 40),
}


def kind_lenses(kind):
    from gigalens_amd import workloads
    from gigalens_amd.profiles.mass import epl, nfw, piemd, piep, shear, sie, sis, tnfw
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    if kind == "catalogue":  # a dPIE catalogue (GL_SCALED) of 3 members, as tests/test_gpu_beta_vjp.py
        return [DPIESubhalo(lum_star=1.0, galaxy_catalogue=workloads.galaxy_catalogue(3, half_width=3.0, seed=4))]
    cls = {"EPL": epl.EPL, "SIE": sie.SIE, "NFW": nfw.NFW, "SHEAR": shear.Shear, "SIS": sis.SIS, "dPIS": piemd.DPIS,
           "dPIE": piemd.DPIE, "dPIEP": piep.DPIEP, "NFW_ELLIPSE": nfw.NFW_ELLIPSE, "TNFW": tnfw.TNFW}[kind]
    return [cls()]


def kind_phys(kind):
    from gigalens_amd.model import PhysicalModel
    return PhysicalModel(kind_lenses(kind), [], [])


def draw(kind, rs_range, r_min, seed, n=max(N_PTS)):
    """``(rows [B, n_par], x [n, B], y [n, B], cot [4, n, B])`` float32."""
    r = np.random.default_rng(seed)
    if kind == "catalogue":
        rows = np.stack([r.uniform(0.2, 0.35, B), r.uniform(0.15, 0.25, B), r.uniform(1.5, 2.5, B)], 1).astype(np.float32)
        centres = [(0.0, 0.0)] * B
    else:
        rows = np.array([KINDS[kind][2](r) for _ in range(B)], dtype=np.float32)
        if rs_range is not None:
            rows[:, 0] = r.uniform(rs_range[0], rs_range[1], B)
        kws = [row_to_kwargs(kind, p) for p in rows]
        centres = [(kw.get("center_x", 0.0), kw.get("center_y", 0.0)) for kw in kws]
    q = np.random.default_rng(seed + 100)
    if kind == "catalogue":  # the centres are the members': the same points for every sample, r_min from each member
        cat = kind_lenses(kind)[0].galaxy_cat
        cand = q.uniform(-6.0, 6.0, (2 * n, 2))
        far = np.all([np.hypot(cand[:, 0] - cx, cand[:, 1] - cy) >= r_min for cx, cy in zip(cat["center_x"], cat["center_y"])], axis=0)
        cand = cand[far][:n]
        assert cand.shape[0] == n
        pts = [(cand[:, 0], cand[:, 1])] * B
    else:
        pts = [points_away(q, n, c, r_min=r_min) for c in centres]
    x = np.stack([p[0] for p in pts], 1).astype(np.float32)
    y = np.stack([p[1] for p in pts], 1).astype(np.float32)
    cot = q.standard_normal((4, n, B)).astype(np.float32)
    return rows, x, y, cot


@functools.lru_cache(maxsize=None)
def vjp_data(label):
    """``(kind, rows, x, y, cot, {n_pts: (float64 gradient [B, L], float32 yardstick)})`` -- computed once and shared (left unchanged)."""
    kind, rs_range, r_min, seed = DRAWS[label]
    rows, x, y, cot = draw(kind, rs_range, r_min, seed)
    phys = kind_phys(kind)
    ref = {}
    for n in N_PTS:
        g64 = hessian_vjp(phys, rows, x[:n], y[:n], cot[:, :n], F64)
        g32 = hessian_vjp(phys, rows, x[:n], y[:n], cot[:, :n], F32)
        ref[n] = (g64, float(H.grad_col_err(g32, g64).max()))
    return kind, rows, x, y, cot, ref


# ---------------------------------------------------------------------------------------------------------------------
# likelihood cases
# ---------------------------------------------------------------------------------------------------------------------
LL_CASES = ("epl_shear|sie", "dpis|sie", "cluster")
N_GAL = [1, 64, 65, 4161]
MIN_R, MIN_G, MIN_K = 0.3, 0.05, 0.05
CAT_SEED = 7


@functools.lru_cache(maxsize=None)
def ll_case(name):
    """``dict(phys, lenses, rows [B, L] float32, centres)``: the lens rows of ``MC.map_case`` on one plane, or the cluster -- one wide
    NFW halo and a 3-member dPIE catalogue.  ``centres``: ``[(x [B], y [B])]`` of everything that has a centre, catalogue members
    included."""
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    from gigalens_amd.profiles.mass.nfw import NFW
    f = MC._f32
    if name == "cluster":
        cat = workloads.galaxy_catalogue(3, half_width=3.0, seed=4)
        epl = MC.map_case("epl_shear|sie")["lens_params"][0]
        lenses = [NFW(), DPIESubhalo(lum_star=1.0, galaxy_catalogue=cat)]
        lp = [{"Rs": f(18, 20, 22), "alpha_Rs": f(3, 4, 5), "center_x": epl["center_x"], "center_y": epl["center_y"]},
              {"theta_E": f(.25, .3, .2), "r_core": f(.2, .15, .25), "r_cut": f(2, 1.5, 2.5)}]
        extra = [(np.full(B, cx, np.float32), np.full(B, cy, np.float32)) for cx, cy in zip(cat["center_x"], cat["center_y"])]
    else:
        c = MC.map_case(name)
        lenses, lp, extra = c["phys"].lenses, c["lens_params"], []
    phys = PhysicalModel(lenses, [], [])
    rows = np.stack([np.asarray(d[k], dtype=np.float32) for lens, d in zip(lenses, lp) for k in lens.params], axis=1)
    centres = [(d["center_x"], d["center_y"]) for d in lp if "center_x" in d] + extra
    return dict(phys=phys, lenses=lenses, rows=rows, centres=centres)


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def margins(c, x, y, scales):
    """``(r, | |g| - 1 |, |1 - kappa|, |g|)`` ``[n, B]`` float64 numpy: the distance to the nearest lens centre and the margins of the
    branch and of the pole of g, in every sample."""
    _, lp = PC.leaf(dict(phys=c["phys"]), F64, packed=c["rows"])
    with torch.enable_grad():
        _, _, kappa, ng = shear_fields(c["phys"], lp, x, y, scales, F64)
    kappa, ng = kappa.detach().numpy(), ng.detach().numpy()
    r = np.full(kappa.shape, np.inf)
    for cx, cy in c["centres"]:
        r = np.minimum(r, np.hypot(_f64(x)[:, None] - _f64(cx)[None, :], _f64(y)[:, None] - _f64(cy)[None, :]))
    return r, np.abs(ng - 1), np.abs(1 - kappa), ng


@functools.lru_cache(maxsize=None)
def catalogue(name, n):
    """The catalogue of ``n`` galaxies of case ``name``: ``dict(x, y, e1, e2, sigma, scales)`` float32 ``[n]``."""
    c = ll_case(name)
    cand = np.random.default_rng(CAT_SEED).uniform(-6, 6, (6 * n + 64, 2)).astype(np.float32)
    scales = (0.6 + 0.1 * (np.arange(cand.shape[0]) % 5)).astype(np.float32)
    r, dg, dk, _ = margins(c, cand[:, 0], cand[:, 1], scales)
    keep = np.flatnonzero(((r >= MIN_R) & (dg >= MIN_G) & (dk >= MIN_K)).all(axis=1))[:n]
    assert keep.size == n, (name, n, keep.size)
    x, y, scales = cand[keep, 0].copy(), cand[keep, 1].copy(), scales[keep].copy()
    j = np.arange(n)
    sigma = (0.25 + 0.05 * (j % 3)).astype(np.float32)
    _, lp = PC.leaf(dict(phys=c["phys"]), F64, packed=c["rows"])
    with torch.enable_grad():
        h1, h2, _, _ = shear_fields(c["phys"], lp, x, y, scales, F64)
    e1 = (h1.detach().numpy()[:, 0] + 0.25 * np.sin(1.7 * j)).astype(np.float32)
    e2 = (h2.detach().numpy()[:, 0] + 0.25 * np.cos(2.3 * j)).astype(np.float32)
    return dict(x=x, y=y, e1=e1, e2=e2, sigma=sigma, scales=scales)


def permuted(cat, seed=5):
    p = np.random.default_rng(seed).permutation(cat["x"].size)
    return {k: v[p].copy() for k, v in cat.items()}


@functools.lru_cache(maxsize=None)
def ll_data(name, n):
    """``(case, catalogue, ref, yard)`` -- computed once and shared (left unchanged).  ``ref``: ``log_like``, ``chi2``, ``model_g``, ``grad`` in
    float64; ``yard``: the float32 restatement's deviation from them -- ``MC.rel_err`` for the values, ``PC.grad_gate`` units for the
    gradient."""
    c, cat = ll_case(name), catalogue(name, n)
    ref = loglike_grad(c["phys"], c["rows"], cat, F64)
    r32 = loglike_grad(c["phys"], c["rows"], cat, F32)
    yard = {k: MC.rel_err(r32[k], ref[k]) for k in ("log_like", "chi2", "model_g")}
    yard["grad"] = PC.grad_gate(r32["grad"], ref["grad"])
    return c, cat, ref, yard
