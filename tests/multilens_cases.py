"""Restatement of multi-plane ray tracing (lenses at several redshifts; csrc/gl_multiplane.hip.h) and the cases of its tests
(tests/test_multilens_host.py pins the restatement without a GPU, tests/test_gpu_multilens.py runs the kernels against it).

The recursion is written from its definition -- planes in redshift order, ``theta_j = theta - sum_{i<j} C_ij a_i``, ``a_i`` the sum of
the deflections of the lenses on plane i at ``theta_i``, ``beta_t = theta - sum_i T_i a_i`` -- and composed from the oracle's ``*_deriv``
primitives (``oracle.ref_torch.mass_deriv``, unchanged); ``A_t = d beta_t / d theta`` comes from ``torch.autograd`` on that composition,
the way tests/multiplane_cases.py composes the scaled plane.  Renders push ``light_eval`` at every source's own ``beta_s`` through NaN -> 0,
``psf_pool``, the conversion factor and the formulas of ``stats_pixels``.  Every function takes ``dtype``: float64 is the reference, the
same code in float32 on the CPU is the yardstick of the value gates (the kernel must stay within 4 x it, the factor of
tests/pixsrc_cases.py).  Couplings enter as the float32 values the library receives."""
import functools
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
Z_REF = 3.0


def _f32(*v):
    return np.asarray(v, dtype=np.float32)


def _tensors(params, dtype):
    return {g: [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype) for k, v in d.items()} for d in lst]
            for g, lst in params.items()}


def _consts(phys, dtype):
    return [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype) for k, v in d.items()} for d in phys.lenses_constants]


# ---------------------------------------------------------------------------------------------------------------------
# the recursion
# ---------------------------------------------------------------------------------------------------------------------
def plane_sums(phys, mp, lens_params, x, y):
    """``[(a_x, a_y)]`` per plane for rays that leave the observer at ``(x, y)`` (``(n, B)`` tensors; their dtype is the arithmetic's)."""
    from oracle import ref_torch as ref
    dt = x.dtype
    C = torch.as_tensor(np.asarray(mp.lens_scales, dtype=np.float32)).to(dt)
    consts = _consts(phys, dt)
    sums = []
    for j in range(mp.K):
        xj, yj = x, y
        for i in range(j):
            xj, yj = xj - C[i, j] * sums[i][0], yj - C[i, j] * sums[i][1]
        ax = ay = 0
        for l, lens in enumerate(phys.lenses):
            if int(mp.plane_of_lens[l]) == j:
                fx, fy = ref.mass_deriv(lens, xj, yj, **lens_params[l], **consts[l])
                ax, ay = ax + fx, ay + fy
        sums.append((ax, ay))
    return sums


def target_beta(sums, x, y, target_scales):
    T = torch.as_tensor(np.asarray(target_scales, dtype=np.float32)).to(x.dtype)
    bx, by = x, y
    for i, (ax, ay) in enumerate(sums):
        if float(T[i]) != 0.0:  # a plane at or behind the target is not part of its ray
            bx, by = bx - T[i] * ax, by - T[i] * ay
    return bx, by


def maps(phys, mp, lens_params, x, y, target_scales, dtype=F64):
    """``beta_x, beta_y, A_xx, A_xy, A_yx, A_yy`` ``[6, n, B]`` (numpy, float64 holding ``dtype`` arithmetic) at the points ``x, y``
    (``[n]`` or ``[n, B]`` float32 values), ``lens_params`` a list of dicts of ``[B]`` float32 arrays."""
    lp = _tensors({"lens_mass": lens_params}, dtype)["lens_mass"]
    B = max([int(np.size(v)) for d in lens_params for v in d.values()] + [1])
    xt = torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float32)).to(dtype)
    if xt.dim() == 1:
        xt, yt = xt[:, None].repeat(1, B), yt[:, None].repeat(1, B)
    xt, yt = xt.clone().requires_grad_(True), yt.clone().requires_grad_(True)
    bx, by = target_beta(plane_sums(phys, mp, lp, xt, yt), xt, yt, target_scales)
    # every point is its own function of its own (x, y): the gradient of the sum holds each point's row of the Jacobian
    axx, axy = torch.autograd.grad(bx.sum(), [xt, yt], retain_graph=True)
    ayx, ayy = torch.autograd.grad(by.sum(), [xt, yt])
    return np.stack([t.detach().double().numpy() for t in (bx, by, axx, axy, ayx, ayy)])


def maps_hessian(phys, mp, lens_params, x, y, target_scales, dtype=F64):
    """The same six maps from the recursion of the Jacobian itself, with every lens's Hessian as the reference resolves it
    (``oracle.ref_torch.mass_hessian``: autodiff of ``deriv``, and the analytic overrides -- the dPIS one is NOT the derivative of
    its deflection, it carries a convergence excess):
    ``D_j = d theta_j / d theta = I - sum_{i<j} C_ij G_i``, ``G_i = sum_{l on i} H_l(theta_i) D_i``, ``A_t = I - sum_i T_i G_i``.
    For lens sets without an override that differs it equals ``maps`` (asserted in tests/test_multilens_host.py); with a dPIS lens it
    is the reference, and ``maps`` differs from it by the excess."""
    from oracle import ref_torch as ref
    lp = _tensors({"lens_mass": lens_params}, dtype)["lens_mass"]
    B = max([int(np.size(v)) for d in lens_params for v in d.values()] + [1])
    xt = torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dtype)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float32)).to(dtype)
    if xt.dim() == 1:
        xt, yt = xt[:, None].repeat(1, B), yt[:, None].repeat(1, B)
    C = torch.as_tensor(np.asarray(mp.lens_scales, dtype=np.float32)).to(dtype)
    T = torch.as_tensor(np.asarray(target_scales, dtype=np.float32)).to(dtype)
    consts = _consts(phys, dtype)
    one, zero = torch.ones_like(xt), torch.zeros_like(xt)
    a, G = [], []
    for j in range(mp.K):
        xj, yj, D = xt, yt, [one, zero, zero, one]
        for i in range(j):
            xj, yj = xj - C[i, j] * a[i][0], yj - C[i, j] * a[i][1]
            D = [d - C[i, j] * g for d, g in zip(D, G[i])]
        ax, ay, g = zero, zero, [zero, zero, zero, zero]
        for l, lens in enumerate(phys.lenses):
            if int(mp.plane_of_lens[l]) == j:
                fx, fy = ref.mass_deriv(lens, xj, yj, **lp[l], **consts[l])
                hxx, hxy, hyx, hyy = (h.detach() for h in ref.mass_hessian(lens, xj, yj, **lp[l], **consts[l]))
                ax, ay = ax + fx.detach(), ay + fy.detach()
                g = [g[0] + hxx * D[0] + hxy * D[2], g[1] + hxx * D[1] + hxy * D[3],
                     g[2] + hyx * D[0] + hyy * D[2], g[3] + hyx * D[1] + hyy * D[3]]
        a.append((ax, ay))
        G.append(g)
    bx, by, A = xt, yt, [one, zero, zero, one]
    for i in range(mp.K):
        if float(T[i]) != 0.0:
            bx, by = bx - T[i] * a[i][0], by - T[i] * a[i][1]
            A = [v - T[i] * g for v, g in zip(A, G[i])]
    return np.stack([t.detach().double().numpy() for t in (bx, by, *A)])


def image(phys, cfg, psf, mp, params, bs, dtype=F64, parts=7):
    """The image ``[bs, H, W]`` of ``LensSimulator.simulate`` on the planes of ``mp`` (``parts``: 1 deflect, 2 lens light, 4 sources) as a
    torch tensor in ``dtype``, and the ``RefSimulator`` it was rendered on."""
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(phys, cfg, bs, dtype=dtype, supersampled_kernel=psf)
    pt = _tensors(params, dtype)
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    rr, cc = torch.from_numpy(rs.region[:, 0]), torch.from_numpy(rs.region[:, 1])
    img = torch.zeros((Hs, Ws, bs), dtype=dtype)
    if parts & 2:
        for lm, p, c in zip(phys.lens_light, pt.get("lens_light", []), rs._consts("lens_light_constants", len(phys.lens_light))):
            img = img.index_put((rr, cc), ref.light_eval(lm, rs.img_X, rs.img_Y, **p, **c), accumulate=True)
    if parts & 4:
        sums = plane_sums(phys, mp, pt["lens_mass"], rs.img_X, rs.img_Y) if parts & 1 else None
        for s, (lm, p, c) in enumerate(zip(phys.source_light, pt["source_light"],
                                           rs._consts("source_light_constants", len(phys.source_light)))):
            bx, by = (target_beta(sums, rs.img_X, rs.img_Y, mp.source_scales[:, s]) if parts & 1 else (rs.img_X, rs.img_Y))
            img = img.index_put((rr, cc), ref.light_eval(lm, bx, by, **p, **c), accumulate=True)
    img = torch.where(torch.isnan(img), torch.zeros_like(img), img)
    ret = ref.psf_pool(img.permute(2, 0, 1)[:, None], rs.flat_kernel, rs.supersample)[:, 0]
    return ret * rs.conversion_factor, rs


def stats_pixels(im, rs, obs, background_rms, exp_time):
    """``stats_pixels`` (tf/model.py:89-101) on the image ``im``: ``(log_like, red_chi2)`` ``[bs]``."""
    dt = im.dtype
    bg = torch.as_tensor(np.float32(background_rms)).to(dt)
    et = torch.as_tensor(np.float32(exp_time)).to(dt)
    err = torch.sqrt(bg ** 2 + im / et)
    o = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(dt)
    reg = rs.img_region
    chi2 = torch.sum(((im - o) / err) ** 2 * reg, dim=(-2, -1))
    norm = torch.sum(torch.log(2 * np.pi * err ** 2) * reg, dim=(-2, -1))
    return -0.5 * (chi2 + norm), chi2 / torch.count_nonzero(reg).to(dt)


# ---------------------------------------------------------------------------------------------------------------------
# errors and gates
# ---------------------------------------------------------------------------------------------------------------------
MAP_KEYS = ("beta_x", "beta_y", "A_xx", "A_xy", "A_yx", "A_yy")


def map_errors(got, ref, x, y, a_scale=None):
    """Largest error of each of the six maps over every point and sample.  ``beta`` is a float32 difference of numbers of the size of
    the coordinates, so its scale is the largest ``|theta|`` of the case; the four entries of A come out of one chain of operations on
    numbers of the size of A's largest entry, which is their common scale (an off-diagonal entry near zero is not held to its own
    size).  ``got`` / ``ref``: ``[6, n, B]`` with ``A`` in rows 2..5; ``x, y`` and ``a_scale`` (default: from ``ref``) give the scales, so that a
    subset of a case's points is held to the scales of the case."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    s_beta = max(float(np.abs(x).max()), float(np.abs(y).max()))
    s_A = float(np.abs(ref[2:]).max()) if a_scale is None else float(a_scale)
    return {k: float(np.abs(got[i] - ref[i]).max()) / (s_beta if i < 2 else s_A) for i, k in enumerate(MAP_KEYS)}


def as_jacobian(native):
    """The library's ``[6, ...]`` = beta_x, beta_y, f_xx, f_xy, f_yx, f_yy with ``f = I - A`` as beta and the entries of A."""
    m = np.array(native, dtype=np.float64)
    m[2], m[5] = 1.0 - m[2], 1.0 - m[5]
    m[3], m[4] = -m[3], -m[4]
    return m


def closed_form_yardstick(yard, keys):
    """The yardstick of the closed-form cases (two Shear planes, two SIS planes) for a group of maps -- ``beta_x, beta_y``, or the
    four entries of A.  Their maps are constants or one short chain of float32 operations repeated at every point, so an entry's
    float32 deviation is a single draw, not a distribution (for some entries the handful of roundings cancel exactly).  The
    entries of a group share their scale and their chain of operations, so the group's worst entry is the yardstick of each."""
    return max(yard[k] for k in keys)


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# lens-map cases
# ---------------------------------------------------------------------------------------------------------------------
PIX = 0.1          # pitch of the point lattices: lens centres sit 0.37 of it off every evaluated point and plane image
OFF = 0.37 * PIX


def points(n):
    """``n`` points of a PIX lattice around the origin (row-major from the lower left of a 10-wide block): exact float32 multiples."""
    k = np.arange(n)
    return ((k % 10 - 4.0) * PIX * 3).astype(np.float32), ((k // 10 - 3.0) * PIX * 3).astype(np.float32)


def _mp(z_lenses, z_sources=()):
    from gigalens_amd.cosmology import MultiPlane
    return MultiPlane(z_lenses, z_sources, Z_REF)


@functools.lru_cache(maxsize=None)
def map_case(name):
    """``dict(phys, mp, z_target, lens_params)`` with three samples of lens parameters (B = 1 uses the first).  Lens centres are
    multiples of PIX plus OFF = 0.37 PIX: no lattice point sits on one, and the rays' positions on the later planes (displaced by
    deflections of order 1 arcsec, irrational in PIX) stay off them as well -- asserted by ``min_centre_distance``."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.profiles.mass.piemd import DPIE, DPIS
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    epl = {"theta_E": _f32(1.1, 1.0, 1.25), "gamma": _f32(2.1, 1.9, 2.3), "e1": _f32(0.1, -0.05, 0.2), "e2": _f32(-0.05, 0.1, 0.0),
           "center_x": _f32(OFF, PIX + OFF, -PIX + OFF), "center_y": _f32(-PIX + OFF, OFF, OFF)}
    shear = {"gamma1": _f32(0.03, -0.02, 0.05), "gamma2": _f32(-0.02, 0.04, 0.01)}
    sie = {"theta_E": _f32(0.4, 0.5, 0.3), "e1": _f32(-0.1, 0.15, 0.05), "e2": _f32(0.08, -0.02, 0.1),
           "center_x": _f32(3 * PIX + OFF, -2 * PIX + OFF, PIX + OFF), "center_y": _f32(2 * PIX + OFF, PIX + OFF, -3 * PIX + OFF)}
    nfw = {"Rs": _f32(2.0, 1.5, 2.5), "alpha_Rs": _f32(0.6, 0.5, 0.8), "center_x": _f32(-PIX + OFF, OFF, PIX + OFF),
           "center_y": _f32(OFF, -PIX + OFF, 2 * PIX + OFF)}
    dpie = {"theta_E": _f32(0.5, 0.6, 0.4), "r_core": _f32(0.05, 0.08, 0.03), "r_cut": _f32(1.5, 2.0, 1.2),
            "center_x": _f32(2 * PIX + OFF, -PIX + OFF, OFF), "center_y": _f32(-2 * PIX + OFF, OFF, PIX + OFF),
            "e1": _f32(0.1, -0.1, 0.05), "e2": _f32(0.0, 0.08, -0.1)}
    sis = {"theta_E": _f32(0.3, 0.25, 0.35), "center_x": _f32(-3 * PIX + OFF, 2 * PIX + OFF, OFF),
           "center_y": _f32(PIX + OFF, -2 * PIX + OFF, -PIX + OFF)}
    dpis = {"theta_E": _f32(0.8, 0.9, 0.7), "r_core": _f32(0.1, 0.15, 0.08), "r_cut": _f32(2.0, 1.5, 2.5),
            "center_x": _f32(-PIX + OFF, OFF, PIX + OFF), "center_y": _f32(OFF, PIX + OFF, -PIX + OFF)}
    hessian_ref = False
    if name == "dpis|sie":           # the dPIS convergence excess on plane 1 and its way into d theta_2 / d theta
        lenses, zl, zt, lp, hessian_ref = [DPIS(), SIE()], [0.4, 0.9], 2.0, [dpis, sie], True
    elif name == "epl_shear|sie":      # K = 2: the main deflector with its shear, a second galaxy behind it
        lenses, zl, zt, lp = [EPL(), Shear(), SIE()], [0.5, 0.5, 1.0], 2.0, [epl, shear, sie]
    elif name == "nfw|dpie|sis":     # K = 3; the target lies between planes 2 and 3: the last plane does not deflect it
        lenses, zl, zt, lp = [NFW(), DPIE(), SIS()], [0.3, 0.7, 1.4], 1.1, [nfw, dpie, sis]
    elif name == "nfw|dpie|sis>":    # ... and behind all three
        lenses, zl, zt, lp = [NFW(), DPIE(), SIS()], [0.3, 0.7, 1.4], 2.5, [nfw, dpie, sis]
    elif name == "shared":           # two lenses share the nearer plane and are NOT adjacent in the model's order
        lenses, zl, zt, lp = [SIE(), SIS(), Shear()], [0.4, 0.9, 0.4], 1.8, [sie, sis, shear]
    else:
        raise KeyError(name)
    mp = _mp(zl)
    return dict(phys=PhysicalModel(lenses, [], []), phys_mp=PhysicalModel(lenses, [], [], multiplane=mp), mp=mp, z_target=zt,
                target=mp.target_scales(zt), lens_params=lp, maps=maps_hessian if hessian_ref else maps)


MAP_CASES = ("epl_shear|sie", "nfw|dpie|sis", "nfw|dpie|sis>", "shared", "dpis|sie")


def sample_rows(lens_params, B):
    return [{k: v[:B] for k, v in d.items()} for d in lens_params]


def min_centre_distance(phys, mp, lens_params, x, y):
    """Smallest distance between a ray's position on a plane and the centre of a lens on that plane, over every point and sample."""
    lp = _tensors({"lens_mass": lens_params}, F64)["lens_mass"]
    B = max(int(np.size(v)) for d in lens_params for v in d.values())
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64))[:, None].repeat(1, B)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64))[:, None].repeat(1, B)
    sums = plane_sums(phys, mp, lp, xt, yt)
    C = np.asarray(mp.lens_scales, dtype=np.float32).astype(np.float64)
    best = math.inf
    for l, d in enumerate(lp):
        if "center_x" not in d:
            continue
        j = int(mp.plane_of_lens[l])
        xj, yj = xt, yt
        for i in range(j):
            xj, yj = xj - C[i, j] * sums[i][0], yj - C[i, j] * sums[i][1]
        best = min(best, float(torch.hypot(xj - d["center_x"], yj - d["center_y"]).min()))
    return best


@functools.lru_cache(maxsize=None)
def map_data(name, n_pts, B):
    """``(case, x, y, reference [6, n, B] float64, yardstick dict)`` -- computed once and shared (left unchanged)."""
    c = map_case(name)
    x, y = points(n_pts)
    lp = sample_rows(c["lens_params"], B)
    ref = c["maps"](c["phys"], c["mp"], lp, x, y, c["target"], F64)
    yard = map_errors(c["maps"](c["phys"], c["mp"], lp, x, y, c["target"], F32), ref, x, y)
    return c, x, y, ref, yard


# ---------------------------------------------------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------------------------------------------------
def shear_matrix(g1, g2):
    """``Gamma`` with ``alpha = Gamma theta`` of a Shear lens (shear.py: f_x = g1 x + g2 y, f_y = g2 x - g1 y)."""
    return np.array([[g1, g2], [g2, -g1]], dtype=np.float64)


def two_shear_case():
    """Two Shear planes, gamma_2 only on plane 1 and gamma_1 only on plane 2: ``(phys, mp, lens_params [B = 1], target, A closed form)``
    with ``A = I - C_1t G1 - C_2t G2 (I - C_12 G1)`` on the float32 couplings.  ``G1`` and ``G2`` are symmetric, ``G2 G1 = g1 g2 [[0, 1],
    [-1, 0]]`` is not: the rotation ``(A_xy - A_yx) / 2 = C_2t C_12 g1 g2`` (g1 of plane 2, g2 of plane 1) is positive."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.shear import Shear
    mp = _mp([0.4, 1.0])
    lp = [{"gamma1": _f32(0.0), "gamma2": _f32(0.08)}, {"gamma1": _f32(0.06), "gamma2": _f32(0.0)}]
    T = mp.target_scales(2.0)
    C12, T1, T2 = (float(np.float32(v)) for v in (mp.lens_scales[0, 1], T[0], T[1]))
    G1, G2 = shear_matrix(0.0, float(np.float32(0.08))), shear_matrix(float(np.float32(0.06)), 0.0)
    A = np.eye(2) - T1 * G1 - T2 * G2 @ (np.eye(2) - C12 * G1)
    return PhysicalModel([Shear(), Shear()], [], []), PhysicalModel([Shear(), Shear()], [], [], multiplane=mp), mp, lp, T, A


def two_sis_case():
    """Two coaxial SIS planes at the origin and points on the positive x axis beyond both Einstein radii and their plane images:
    ``theta_2 = x - C_12 tE1`` and ``beta = x - C_1t tE1 - C_2t tE2 sign(theta_2)`` (float32 couplings).  Returns
    ``(phys, phys_mp, mp, lens_params, target, x, y, theta_2, beta)``; the points are 0.37 PIX off the lattice, like every centre."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    mp = _mp([0.4, 1.0])
    # C_12 tE1 = 6 PIX + 2 OFF: the plane images theta_2 = (k - 6) PIX - OFF stay 0.37 PIX off the second centre as well
    tE1, tE2 = np.float32((6 * PIX + 2 * OFF) / np.float32(mp.lens_scales[0, 1])), np.float32(0.5)
    lp = [{"theta_E": _f32(tE1), "center_x": _f32(0.0), "center_y": _f32(0.0)},
          {"theta_E": _f32(tE2), "center_x": _f32(0.0), "center_y": _f32(0.0)}]
    T = mp.target_scales(2.0)
    C12, T1, T2 = (float(np.float32(v)) for v in (mp.lens_scales[0, 1], T[0], T[1]))
    x = (np.arange(1, 13) * PIX + OFF).astype(np.float32)  # 0.137 .. 1.237: theta_2 takes both signs
    y = np.zeros_like(x)
    th2 = x.astype(np.float64) - C12 * float(tE1)
    beta = x.astype(np.float64) - T1 * float(tE1) - T2 * float(tE2) * np.sign(th2)
    return (PhysicalModel([SIS(), SIS()], [], []), PhysicalModel([SIS(), SIS()], [], [], multiplane=mp), mp, lp, T, x, y, th2, beta)


# ---------------------------------------------------------------------------------------------------------------------
# render cases
# ---------------------------------------------------------------------------------------------------------------------
def gauss_psf(n, sigma):
    g = np.exp(-0.5 * ((np.arange(n) - (n - 1) / 2) / sigma) ** 2)
    k = np.outer(g, g).astype(np.float32)
    return k / k.sum()


RENDER_CASES = ("plain16", "psf12ss2", "region", "core11")
BG, TEXP = 0.2, 100.0


@functools.lru_cache(maxsize=None)
def render_case(name):
    """SIE + Shear on plane 1 (z = 0.5), an SIS on plane 2 (z = 1.0) | a Sersic lens light | a SersicEllipse source BETWEEN the planes
    (z = 0.8: lensed by plane 1 only) and a Sersic source behind both (z = 2.0).  Three samples.  Lens centres are 0.37 of a
    (supersampled) pixel off the pixel centres."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import CoreSersic, Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import SimulatorConfig
    if name == "plain16":
        num_pix, ss, psf, region = 16, 1, None, None
    elif name == "psf12ss2":
        num_pix, ss, psf, region = 12, 2, gauss_psf(5, 1.1), None
    elif name == "region":  # an L-shaped corner and one inner pixel left out; odd size
        num_pix, ss, psf = 13, 1, None
        region = np.ones((13, 13), dtype=np.float32)
        region[:4, :5] = 0
        region[:7, :2] = 0
        region[8, 9] = 0
    elif name == "core11":  # a CoreSersic lens light in place of the Sersic; odd size, one block with a tail
        num_pix, ss, psf, region = 11, 1, None, None
    else:
        raise KeyError(name)
    delta = 0.2
    sub = delta / ss
    # pixel centres of an even grid lie at odd multiples of sub / 2; of an odd one at multiples of sub: 0.37 sub off either
    off = 0.37 * sub + (sub / 2 if (num_pix * ss) % 2 == 0 else 0.0)
    mp = _mp([0.5, 0.5, 1.0], [0.8, 2.0])
    lenses = [SIE(), Shear(), SIS()]
    lights = ([Sersic()], [SersicEllipse(), Sersic()])
    params = {
        "lens_mass": [{"theta_E": _f32(1.0, 0.9, 1.1), "e1": _f32(0.1, -0.05, 0.15), "e2": _f32(-0.05, 0.1, 0.0),
                       "center_x": _f32(off, sub + off, -sub + off), "center_y": _f32(-sub + off, off, off)},
                      {"gamma1": _f32(0.03, -0.02, 0.04), "gamma2": _f32(-0.02, 0.03, 0.01)},
                      {"theta_E": _f32(0.35, 0.3, 0.4), "center_x": _f32(2 * sub + off, -sub + off, off),
                       "center_y": _f32(sub + off, -2 * sub + off, 3 * sub + off)}],
        "lens_light": [{"R_sersic": _f32(0.6, 0.5, 0.7), "n_sersic": _f32(2.5, 3.0, 2.0), "center_x": _f32(0.02, 0.0, -0.03),
                        "center_y": _f32(-0.01, 0.03, 0.0), "Ie": _f32(30.0, 25.0, 40.0)}],
        "source_light": [{"R_sersic": _f32(0.25, 0.3, 0.2), "n_sersic": _f32(1.5, 1.0, 2.0), "e1": _f32(0.1, -0.1, 0.0),
                          "e2": _f32(0.05, 0.0, -0.1), "center_x": _f32(0.15, -0.1, 0.2), "center_y": _f32(-0.1, 0.2, 0.05),
                          "Ie": _f32(120.0, 150.0, 100.0)},
                         {"R_sersic": _f32(0.2, 0.15, 0.25), "n_sersic": _f32(1.0, 2.0, 1.5), "center_x": _f32(-0.2, 0.1, 0.0),
                          "center_y": _f32(0.1, -0.15, 0.2), "Ie": _f32(150.0, 110.0, 130.0)}],
    }
    if name == "core11":
        lights = ([CoreSersic()], lights[1])
        params["lens_light"] = [{"R_sersic": _f32(0.6, 0.5, 0.7), "n_sersic": _f32(2.5, 3.0, 2.0), "Rb": _f32(0.15, 0.2, 0.1),
                                 "alpha": _f32(2.0, 3.0, 2.5), "gamma": _f32(0.2, 0.1, 0.3), "e1": _f32(0.05, -0.1, 0.0),
                                 "e2": _f32(-0.05, 0.0, 0.1), "center_x": _f32(0.02, 0.0, -0.03), "center_y": _f32(-0.01, 0.03, 0.0),
                                 "Ie": _f32(30.0, 25.0, 40.0)}]
    cfg = SimulatorConfig(delta_pix=delta, num_pix=num_pix, supersample=ss, pix_region=region)
    return dict(phys=PhysicalModel(lenses, *lights), phys_mp=PhysicalModel(lenses, *lights, multiplane=mp), mp=mp, cfg=cfg, psf=psf,
                params=params, B=3)


@functools.lru_cache(maxsize=None)
def render_data(name):
    """``(case, obs [H, W] float32, reference dict, yardstick dict)``: the float64 image, log-likelihood and reduced chi^2 of the
    three samples against a seeded noisy observation of the first, and the float32 restatement's relative deviation from them."""
    c = render_case(name)
    im64, rs64 = image(c["phys"], c["cfg"], c["psf"], c["mp"], c["params"], c["B"], F64)
    r = np.random.default_rng(11)
    clean = im64[0].numpy()
    obs = (clean + r.normal(size=clean.shape) * np.sqrt(BG ** 2 + np.clip(clean, 0, None) / TEXP)).astype(np.float32)
    ll64, red64 = stats_pixels(im64, rs64, obs, BG, TEXP)
    im32, rs32 = image(c["phys"], c["cfg"], c["psf"], c["mp"], c["params"], c["B"], F32)
    ll32, red32 = stats_pixels(im32, rs32, obs, BG, TEXP)
    ref = dict(image=im64.numpy(), log_like=ll64.numpy(), red_chi2=red64.numpy())
    yard = dict(image=rel_err(im32.numpy(), ref["image"]), log_like=rel_err(ll32.numpy(), ref["log_like"]),
                red_chi2=rel_err(red32.numpy(), ref["red_chi2"]))
    return c, obs, ref, yard
