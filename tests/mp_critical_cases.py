"""float64 references of the critical curves on lens planes (gl_multiplane_critical_curves;
``LensSimulator.critical_curves / einstein_radius(source_redshifts=...)``).  tests/test_mp_critical_host.py pins them without a GPU,
tests/test_gpu_mp_critical.py runs the kernels against them.

Nothing of the contouring is restated here: ``critical_cases.contour64`` contours any ``fields(x, y) -> (D, beta_x, beta_y, 1 - kappa)``.
The fields of a target plane come from the float64 recursion of tests/multilens_cases.py (``plane_sums`` + ``target_beta`` on the float32
couplings the library receives) with the Jacobian ``A_t = d beta_t / d theta`` from autograd: ``D = det A_t`` of the NON-symmetric
Jacobian and ``1 - kappa := tr A_t / 2`` (on D = 0 the eigenvalues of A_t are 0 and tr A_t).  They are evaluated on the float64 points
they are handed -- ``multilens_cases.maps`` rounds its points to float32, which would stall the 1e-13 bisection of ``contour64``.

The closed form: one SIS (theta_E, centre c) on plane 1 and one Shear (matrix G) on plane 2, the source behind both.  With
``alpha_1 = theta_E rhat`` about c and ``theta_2 = theta - C_12 alpha_1``:
    beta = theta - T_1 alpha_1 - T_2 G theta_2 = M theta - N alpha_1,    M = I - T_2 G,    N = T_1 I - T_2 C_12 G,
    A    = M - N H_SIS,    H_SIS = (theta_E / r) t t^T,    t = (-sin phi, cos phi),
    det A = det M (1 - (theta_E / r) t^T M^-1 N t)          (matrix determinant lemma),
so the single critical curve is ``r(phi) = theta_E t^T M^-1 N t`` about c, tangential (``tr A = tr M - (theta_E / r) t^T N t`` ~ 1 there),
the caustic is ``M theta - N theta_E rhat`` on it and the enclosed area ``1/2 int r^2 dphi``.  C_12 enters the curve through N."""
import functools
import math

import numpy as np
import torch

from tests import critical_cases as CC
from tests import multilens_cases as MC

EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------------------------------------------------
# fields of the recursion
# ---------------------------------------------------------------------------------------------------------------------
def recursion_fields(phys, mp, lens_params, b, target):
    """``fields`` of ``contour64`` for sample b of ``lens_params`` (a list of dicts of [B] float32 arrays) on the plane with couplings
    ``target``; ``fields.hessian(x, y) -> (beta_x, beta_y, 1 - A_xx, -A_xy, -A_yx, 1 - A_yy)``."""
    lp = [{k: v[b] for k, v in d.items()} for d in MC._tensors({"lens_mass": lens_params}, MC.F64)["lens_mass"]]

    def jacobian(x, y):
        shape = np.shape(x)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).reshape(-1).clone().requires_grad_(True)
        yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64)).reshape(-1).clone().requires_grad_(True)
        bx, by = MC.target_beta(MC.plane_sums(phys, mp, lp, xt, yt), xt, yt, target)
        # every point is its own function of its own (x, y): the gradient of the sum holds each point's row of the Jacobian
        axx, axy = torch.autograd.grad(bx.sum(), [xt, yt], retain_graph=True, allow_unused=True)
        ayx, ayy = torch.autograd.grad(by.sum(), [xt, yt], allow_unused=True)
        z = torch.zeros_like(xt)
        return tuple((z if t is None else t).detach().numpy().reshape(shape) for t in (bx, by, axx, axy, ayx, ayy))

    def fields(x, y):
        bx, by, axx, axy, ayx, ayy = jacobian(x, y)
        return axx * ayy - axy * ayx, bx, by, 0.5 * (axx + ayy)

    def hessian(x, y):
        bx, by, axx, axy, ayx, ayy = jacobian(x, y)
        return bx, by, 1 - axx, -axy, -ayx, 1 - ayy
    fields.hessian = hessian
    return fields


def maps_fields(maps, phys, mp, lens_params, b, target, dtype=MC.F64):
    """The same fields from ``multilens_cases.maps`` / ``maps_hessian`` in ``dtype`` arithmetic, at the float32 values of the points."""
    lp = [{k: v[b:b + 1] for k, v in d.items()} for d in lens_params]

    def fields(x, y):
        shape = np.shape(x)
        m = maps(phys, mp, lp, np.ravel(x), np.ravel(y), target, dtype)[:, :, 0]
        bx, by, axx, axy, ayx, ayy = (v.reshape(shape) for v in m)
        return axx * ayy - axy * ayx, bx, by, 0.5 * (axx + ayy)
    return fields


def grad_D32(fields, x, y, step=2.0 ** -10):
    """|grad D| by central differences for fields that read their points as float32 values (``maps_fields``): the step is a power of
    two far above the float32 spacing of the coordinates, so the shifted points are float32 values (to one spacing: 1e-4 of the step)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    gx = (fields(x + np.float32(step), y)[0] - fields(x - np.float32(step), y)[0]) / (2 * step)
    gy = (fields(x, y + np.float32(step))[0] - fields(x, y - np.float32(step))[0]) / (2 * step)
    return np.hypot(gx, gy)


def crossing_edges(D):
    """The set of crossing grid edges of a vertex plane ``D`` [n+1, n+1] (ids as ``contour64`` numbers them)."""
    n = D.shape[0] - 1
    fin, neg = np.isfinite(D), np.nan_to_num(D, nan=1.0) < 0
    hz = fin[:, :-1] & fin[:, 1:] & (neg[:, :-1] != neg[:, 1:])
    vt = fin[:-1, :] & fin[1:, :] & (neg[:-1, :] != neg[1:, :])
    return set(np.flatnonzero(hz.ravel()).tolist()) | set(((n + 1) * n + np.flatnonzero(vt.ravel())).tolist())


def vertex_plane(fields, window, n):
    """D at the (n+1)^2 vertices of the FLOAT32 grid of the kernel (x_lo + c * hx in float32), from ``fields``."""
    x_lo, x_hi, y_lo, y_hi = (np.float32(v) for v in window)
    hx, hy = (x_hi - x_lo) / np.float32(n), (y_hi - y_lo) / np.float32(n)
    xs, ys = x_lo + np.arange(n + 1, dtype=np.float32) * hx, y_lo + np.arange(n + 1, dtype=np.float32) * hy
    X, Y = np.meshgrid(xs, ys)
    D = fields(X.ravel(), Y.ravel())[0].reshape(n + 1, n + 1)
    return np.where(np.isfinite(D), D, np.nan)


# ---------------------------------------------------------------------------------------------------------------------
# the general cases: lens sets of multilens_cases.map_case, three samples
# ---------------------------------------------------------------------------------------------------------------------
# name -> (source redshifts, window, cells).  Windows of about 6 arcsec a side; the vertices are multiples of the cell side off a
# corner that is no multiple of PIX, so none sits on a lens centre (k PIX + 0.37 PIX).  tests/test_mp_critical_host.py asserts that
# every float64 reference is closed, unflagged and free of ambiguous cells, and that the float32 recursion crosses the same edges.
# The windows of the first, second and fourth were moved by a quarter (0.4) of a cell off (-3, 3)^2, where a small radial loop
# beside a secondary lens left an ambiguous cell.
GENERAL = {
    "epl_shear|sie": ((2.0, 0.8), (-3.0, 3.0, -3.03125, 2.96875), 48),    # (0.8: between the planes)
    "nfw|dpie|sis": ((1.1, 2.5), (-2.95, 3.05, -2.96875, 3.03125), 48),   # K = 3; 1.1 lies in front of the last plane
    "nfw|dpie|sis>": ((2.5,), (-3.1, 2.9, -2.9, 3.1), 40),
    "shared": ((1.8,), (-3.0, 3.0, -3.03125, 2.96875), 48),
}
DPIS = ("dpis|sie", (2.0,), (-3.0, 3.0, -3.0, 3.0), 48)


def general_targets(name):
    c = MC.map_case(name)
    z = GENERAL[name][0] if name in GENERAL else DPIS[1]
    return z, [c["mp"].target_scales(v) for v in z]


@functools.lru_cache(maxsize=None)
def general_reference(name, b, s):
    """``(fields, contour64 result)`` of sample b, source s of a general case -- computed once and shared (left unchanged)."""
    c = MC.map_case(name)
    _, T = general_targets(name)
    _, window, n = GENERAL[name]
    f = recursion_fields(c["phys"], c["mp"], c["lens_params"], b, T[s])
    return f, CC.contour64(f, window, n)


def four_plane_reference():
    from tests import mp_images_cases as IC
    phys, _, mp, lp = IC.four_plane_case()
    f = recursion_fields(phys, mp, lp, 0, mp.target_scales(2.0))
    return f, CC.contour64(f, FOUR_WINDOW, FOUR_CELLS)


FOUR_WINDOW, FOUR_CELLS = (-3.0, 3.0, -3.0, 3.0), 48


# ---------------------------------------------------------------------------------------------------------------------
# closed form: SIS | Shear
# ---------------------------------------------------------------------------------------------------------------------
CF_WINDOW, CF_CELLS = (-3.0, 3.0, -3.0, 3.0), 48
CF_Z = 2.0


@functools.lru_cache(maxsize=None)
def sis_shear_case():
    """``dict(phys, phys_mp, mp, lens_params, target)``: an SIS on plane 1 (z = 0.4, centres 0.37 PIX off the lattice) and a Shear on plane
    2 (z = 1.0), three samples, the source at z = 2."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    mp = MC._mp([0.4, 1.0])
    lp = [{"theta_E": MC._f32(1.2, 0.9, 1.5), "center_x": MC._f32(MC.OFF, MC.PIX + MC.OFF, -2 * MC.PIX + MC.OFF),
           "center_y": MC._f32(-MC.PIX + MC.OFF, MC.OFF, MC.PIX + MC.OFF)},
          {"gamma1": MC._f32(0.08, -0.05, 0.03), "gamma2": MC._f32(-0.04, 0.07, 0.09)}]
    lenses = [SIS(), Shear()]
    return dict(phys=PhysicalModel(lenses, [], []), phys_mp=PhysicalModel(lenses, [], [], multiplane=mp), mp=mp, lens_params=lp,
                target=mp.target_scales(CF_Z))


def sis_shear_closed_form(b, n_phi=4096):
    """Sample b of ``sis_shear_case``: ``dict(centre, radius(phi), caustic(phi), area, perimeter, M, N, theta_E)`` on the float32 couplings
    and parameters; area and perimeter by the trapezoid rule on ``n_phi`` angles (spectrally accurate on a periodic integrand)."""
    c = sis_shear_case()
    lp, mp = c["lens_params"], c["mp"]
    C12, T1, T2 = (float(np.float32(v)) for v in (mp.lens_scales[0, 1], c["target"][0], c["target"][1]))
    tE = float(lp[0]["theta_E"][b])
    centre = np.array([float(lp[0]["center_x"][b]), float(lp[0]["center_y"][b])])
    G = MC.shear_matrix(float(lp[1]["gamma1"][b]), float(lp[1]["gamma2"][b]))
    M, N = np.eye(2) - T2 * G, T1 * np.eye(2) - T2 * C12 * G
    Q = np.linalg.solve(M, N)

    def radius(phi):
        t = np.stack([-np.sin(phi), np.cos(phi)])
        return tE * np.einsum("i...,ij,j...->...", t, Q, t)

    def point(phi):
        return centre[:, None] + radius(phi) * np.stack([np.cos(phi), np.sin(phi)])

    def caustic(phi):
        rhat = np.stack([np.cos(phi), np.sin(phi)])
        return M @ point(phi) - tE * (N @ rhat)
    phi = np.arange(n_phi) * (2 * math.pi / n_phi)
    r = radius(phi)
    p = point(np.append(phi, 2 * math.pi))
    return dict(centre=centre, radius=radius, point=point, caustic=caustic, area=0.5 * float(np.sum(r * r)) * (2 * math.pi / n_phi),
                perimeter=float(np.sum(np.hypot(*np.diff(p, axis=1)))), M=M, N=N, theta_E=tE, C12=C12)
