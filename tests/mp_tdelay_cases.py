"""Cases and float64 references of the arrival times on lens planes (gl_multiplane_fermat; ``LensSimulator.time_delays(source_redshifts=...)``,
``fermat_potential(source_redshift=...)``).  tests/test_mp_tdelays_host.py pins
them without a GPU, tests/test_gpu_mp_tdelays.py runs the kernel against them.

Two float64 evaluations of

    T(theta; beta_s) = sum_{i < Ks} [ g_i |theta_i - theta_next(i)|^2 / 2 - v_i psi_i(theta_i) ]        (MultiPlane.delay_weights)

* ``reference_T``: composed from parts that other tests already pin -- the rays' positions theta_i from the float64 recursion of
  tests/multilens_cases.py (``plane_sums``: the oracle's deflections, on the float32 couplings the library receives) and psi_i from
  ``potential_cases.host_psi`` (the float64 host build of the ``*_pot`` templates, pinned to the oracle's deflection by
  tests/test_potential_host.py); the sum above is written out in numpy.
* ``host_T``: tests/hostmath/multiplane_fermat_host.cpp, the kernel's own thread body compiled with g++ on double.  The kernel must
  agree with it to ``KERNEL_GATE`` of the sum of the magnitudes of the summands of T: the code and the arithmetic are the same and
  only the math library differs, so the gate sits 1e3 above double rounding and 1e2 below float32 rounding.

``HOST_CEILING``: the host build against the composed reference for every lens set, measured on the CPU when the cases were fixed,
times two (the pattern of ``tdelay_cases.YARD_CEILING``); tests/test_mp_tdelays_host.py asserts it, so no GPU number enters."""
import ctypes
import functools
import os
import subprocess
from ctypes import POINTER, c_double, c_float, c_int

import numpy as np
import torch

from tests import multilens_cases as MC
from tests import mp_images_cases as MI
from tests import potential_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXK = 4
KERNEL_GATE = 1e-10
F32_OUT = 1e-6  # float32 rounding of a returned delay (6e-8) with room for the subtraction of the earliest image
N_LATTICE = 30
# largest |host_T - reference_T| / terms over the lattice of each lens set, measured (x86-64, g++ -O2, torch CPU float64): 8.2e-16
# (epl_shear|sie), 1.7e-11 (both nfw|dpie|sis: the NFW templates against the oracle's NFW), 1.5e-16 (shared), 4.2e-16 (dpis|sie),
# 4.8e-16 (four_planes: K = 4, four sources behind 1, 2, 3 and 4 planes).  The
# ceiling is twice that, and no less than 32 eps: where the two agree to rounding the measured figure is a single draw of a few
# ulp of the up to eight summands of T, each the end of tens of double operations whose last bits belong to the math library
ROUNDING_FLOOR = 32 * 2.0 ** -53
HOST_CEILING = {k: max(2 * v, ROUNDING_FLOOR) for k, v in {"epl_shear|sie": 8.2e-16, "nfw|dpie|sis": 1.7e-11, "nfw|dpie|sis>": 1.7e-11,
                                                           "shared": 1.5e-16, "dpis|sie": 4.2e-16, "four_planes": 4.8e-16}.items()}

_SO = None


def fermat_host():
    """ctypes handle of tests/hostmath/multiplane_fermat_host.cpp compiled with g++ (rebuilt when it or a csrc header is newer)."""
    global _SO
    if _SO is None:
        src = os.path.join(ROOT, "tests", "hostmath", "multiplane_fermat_host.cpp")
        so = os.path.join(ROOT, "tests", "hostmath", "libmultiplane_fermat_host.so")
        csrc = os.path.join(ROOT, "gigalens_amd", "csrc")
        deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h") and not f.endswith(".hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
        _SO = ctypes.CDLL(so)
        _SO.mp_fermat_host.argtypes = ([c_int] + [POINTER(c_int)] * 6 + [POINTER(c_float)] * 2 + [c_int] * 4 + [POINTER(c_float)] * 4
                                       + [POINTER(c_double)] * 2 + [c_int] + [POINTER(c_double)] * 2)
        _SO.mp_fermat_host.restype = None
    return _SO


def weights(mp, z_sources):
    """``(geom [S, K], pot [K])`` float64 of ``MultiPlane.delay_weights`` for the sources.  The potential weight is a constant of the
    plane, which a source's own row holds for the planes in front of it alone: ``pot`` is the row of the farthest source."""
    w = [mp.delay_weights(z) for z in z_sources]
    return np.stack([g for g, _ in w], axis=0), w[int(np.argmax(np.asarray(z_sources, dtype=np.float64)))][1]


def packed_rows(phys, lens_params, B):
    """The native ``[B, P]`` float32 rows of the lens parameters (``_Packing``: the order the library holds them in)."""
    lp = [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)) for k, v in d.items()} for d in lens_params]
    return phys._packing().pack({"lens_mass": lp}, B, "cpu").numpy()


def _ip(a):
    return a.ctypes.data_as(POINTER(c_int))


def host_T(phys, mp, lens_params, x, y, sx, sy, geom, pot):
    """``(T, terms)`` ``[B, S, M]`` float64 of the host build at the float32 points ``x, y`` ``[B, S, M]`` for the sources ``sx, sy`` ``[B, S]``."""
    x, y, sx, sy = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, sx, sy))
    B, S, M = x.shape
    comps = [lens._component() for lens in phys.lenses]
    n_par = np.asarray([len(lens._native_params()) for lens in phys.lenses], dtype=np.int32)
    kind = np.asarray([c[0] for c in comps], dtype=np.int32)
    iparam = np.asarray([c[1] for c in comps], dtype=np.int32)
    p_off = np.concatenate([[0], np.cumsum(n_par)[:-1]]).astype(np.int32)
    plane = np.ascontiguousarray(mp.plane_of_lens, dtype=np.int32)
    order = np.argsort(plane, kind="stable").astype(np.int32)
    scale = np.zeros((MAXK, MAXK), dtype=np.float32)
    scale[:mp.K, :mp.K] = np.asarray(mp.lens_scales, dtype=np.float32)
    rows = np.ascontiguousarray(packed_rows(phys, lens_params, B), dtype=np.float32)
    g, v = np.ascontiguousarray(geom, dtype=np.float64), np.ascontiguousarray(pot, dtype=np.float64)
    assert g.shape == (S, mp.K) and v.shape == (mp.K,) and sx.shape == (B, S) and rows.shape[1] == int(n_par.sum())
    out, terms = np.empty((B, S, M)), np.empty((B, S, M))
    fp, dp = (lambda a: a.ctypes.data_as(POINTER(c_float))), (lambda a: a.ctypes.data_as(POINTER(c_double)))
    fermat_host().mp_fermat_host(len(comps), _ip(kind), _ip(iparam), _ip(n_par), _ip(p_off), _ip(plane), _ip(order), fp(scale), fp(rows),
                                 rows.shape[1], B, S, M, fp(x), fp(y), fp(sx), fp(sy), dp(g), dp(v), mp.K, dp(out), dp(terms))
    return out, terms


def exact_plane_sums(phys, mp, lens_params, x, y):
    """``multilens_cases.plane_sums`` on the float64 couplings of ``mp`` instead of their float32 values: the same statements."""
    from oracle import ref_torch as ref
    C = torch.as_tensor(np.asarray(mp.lens_scales, dtype=np.float64))
    consts = MC._consts(phys, x.dtype)
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


def plane_positions_and_psi(phys, mp, lens_params, x, y, exact=False):
    """``(theta [K] of (x, y), psi [K])``, each ``[n, B]`` float64 numpy: the ray's position on every plane (``multilens_cases.plane_sums``)
    and the potential of the plane's lenses there (``potential_cases.host_psi``) for rays that leave at ``x, y`` ``[n, B]`` float64.
    ``exact``: on the float64 couplings (``exact_plane_sums``) -- the physics; the default float32 values are what the library holds."""
    B = x.shape[1]
    lp = MC._tensors({"lens_mass": lens_params}, MC.F64)["lens_mass"]
    xt, yt = torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(y, dtype=np.float64))
    with torch.no_grad():
        sums = (exact_plane_sums if exact else MC.plane_sums)(phys, mp, lp, xt, yt)
    C = np.asarray(mp.lens_scales, dtype=np.float64) if exact else np.asarray(mp.lens_scales, dtype=np.float32).astype(np.float64)
    rows = packed_rows(phys, lens_params, B).astype(np.float64)
    n_par = [len(lens._native_params()) for lens in phys.lenses]
    p_off = np.concatenate([[0], np.cumsum(n_par)]).astype(int)
    theta, psi = [], []
    for j in range(mp.K):
        xj, yj = np.asarray(x, dtype=np.float64).copy(), np.asarray(y, dtype=np.float64).copy()
        for i in range(j):
            xj, yj = xj - C[i, j] * sums[i][0].numpy(), yj - C[i, j] * sums[i][1].numpy()
        pj = np.zeros_like(xj)
        for l, lens in enumerate(phys.lenses):
            if int(mp.plane_of_lens[l]) == j:
                kind, iparam, _ = lens._component()
                for b in range(B):
                    pj[:, b] += PC.host_psi(kind, rows[b, p_off[l]:p_off[l + 1]], xj[:, b], yj[:, b], iparam=iparam)
        theta.append((xj, yj))
        psi.append(pj)
    return theta, psi


def reference_T(phys, mp, lens_params, x, y, sx, sy, geom, pot, exact=False):
    """``(T, terms)`` ``[B, S, M]`` float64 of the composed reference at the points ``x, y`` ``[B, S, M]`` (float32 or float64 values).
    ``exact``: the rays on the float64 couplings (``plane_positions_and_psi``)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    sx, sy = np.asarray(sx, dtype=np.float64), np.asarray(sy, dtype=np.float64)
    B, S, M = x.shape
    theta, psi = plane_positions_and_psi(phys, mp, lens_params, x.reshape(B, S * M).T, y.reshape(B, S * M).T, exact)
    back = lambda a: a.T.reshape(B, S, M)
    T, terms = np.zeros((B, S, M)), np.zeros((B, S, M))
    for s in range(S):
        ks = int(np.count_nonzero(geom[s]))
        assert ks >= 1 and np.all(geom[s][:ks] > 0) and np.all(geom[s][ks:] == 0)
        for i in range(ks):
            tix, tiy = back(theta[i][0])[:, s], back(theta[i][1])[:, s]
            if i + 1 < ks:
                nx, ny = back(theta[i + 1][0])[:, s], back(theta[i + 1][1])[:, s]
            else:
                nx, ny = sx[:, s, None], sy[:, s, None]
            geo = geom[s, i] * 0.5 * ((tix - nx) ** 2 + (tiy - ny) ** 2)
            grav = pot[i] * back(psi[i])[:, s]
            T[:, s] += geo - grav
            terms[:, s] += np.abs(geo) + np.abs(grav)
    return T, terms


# ---- the lattice cases: every lens set of multilens_cases.MAP_CASES, one source between the last two planes and one behind all ------
LATTICE_SRC_X = np.asarray([[0.05, -0.04], [0.02, 0.07], [-0.06, 0.03]], dtype=np.float32)  # [B, S]
LATTICE_SRC_Y = np.asarray([[-0.03, 0.07], [0.06, -0.02], [0.04, -0.05]], dtype=np.float32)


def lattice_redshifts(mp):
    """A source between the last two planes and one behind every plane (and behind the reference plane)."""
    return 0.5 * (mp.z_planes[-2] + mp.z_planes[-1]), MC.Z_REF + 0.5


# K = 4 = MP_MAXK (mp_images_cases.four_plane_case, one sample): S = 4 sources behind 1, 2, 3 and 4 planes in one call
FOUR_PLANES = "four_planes"
FOUR_PLANES_SRC_X = np.asarray([[0.05, -0.04, 0.02, 0.07]], dtype=np.float32)  # [B = 1, S = 4]
FOUR_PLANES_SRC_Y = np.asarray([[-0.03, 0.07, 0.06, -0.02]], dtype=np.float32)


def four_plane_redshifts(mp):
    """One source behind each plane: between every two planes, and behind all (and behind the reference plane)."""
    zp = mp.z_planes
    return tuple(0.5 * (a + b) for a, b in zip(zp[:-1], zp[1:])) + (MC.Z_REF + 0.5,)


@functools.lru_cache(maxsize=None)
def lattice_data(name, B=3):
    """``dict(case, z [S], x, y [B, S, N_LATTICE], sx, sy [B, S], geom, pot, host=(T, terms), ref=(T, terms))`` -- computed once and
    shared.  S = 2 for the lens sets of ``multilens_cases.MAP_CASES``; ``FOUR_PLANES``: B = 1, S = 4."""
    if name == FOUR_PLANES:
        phys, phys_mp, mp, lp = MI.four_plane_case()
        c, B = dict(phys=phys, phys_mp=phys_mp, mp=mp, lens_params=lp), 1
        z, sx, sy = four_plane_redshifts(mp), FOUR_PLANES_SRC_X, FOUR_PLANES_SRC_Y
    else:
        c = MC.map_case(name)
        z, sx, sy = lattice_redshifts(c["mp"]), LATTICE_SRC_X[:B], LATTICE_SRC_Y[:B]
    S = len(z)
    px, py = MC.points(N_LATTICE)
    x = np.ascontiguousarray(np.broadcast_to(px, (B, S, N_LATTICE)))
    y = np.ascontiguousarray(np.broadcast_to(py, (B, S, N_LATTICE)))
    geom, pot = weights(c["mp"], z)
    lp = MC.sample_rows(c["lens_params"], B)
    return dict(case=c, z=z, x=x, y=y, sx=sx, sy=sy, geom=geom, pot=pot, lens_params=lp,
                host=host_T(c["phys"], c["mp"], lp, x, y, sx, sy, geom, pot),
                ref=reference_T(c["phys"], c["mp"], lp, x, y, sx, sy, geom, pot))


def relative_to_terms(got, ref, terms):
    """Largest ``|got - ref| / terms`` (NaN where both are NaN does not count; a NaN on one side alone is infinite)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    both = np.isnan(got) & np.isnan(ref)
    err = np.where(both, 0.0, np.abs(got - ref) / np.where(both, 1.0, terms))
    return float(np.nan_to_num(err, nan=np.inf).max())


# ---- Fermat's principle on the general cases of the solver ------------------------------------------------------------------------
# The images are the stationary points of T when the weights and the couplings describe ONE geometry: g_i C_i,next(i) = v_i.  The
# weights are float64; on the float32 values of the couplings (what the library and ``reference_T`` hold) the identity is off by
# 6e-8, and the gradient of T at an image by 6e-8 g |alpha| -- 8e-8 measured on ``epl_shear|sie``, 2e-6 of the gradient a cell away,
# a property of that rounding and not of the formula.  So the principle is checked with ``exact=True``: images and T on the float64
# couplings (measured: 5e-9 of the gradient a cell away and less).
def exact_deriv64(name, b, z):
    """float64 deflection ``(x, y) -> (x - beta_x, y - beta_y)`` of a source at redshift z behind sample b of ``map_case(name)``, on
    the float64 couplings: ``mp_images_cases.deriv64`` without the float32 rounding of ``C`` and ``T``."""
    c = MC.map_case(name)
    phys, mp = c["phys"], c["mp"]
    lp = [{k: v[b] for k, v in d.items()} for d in MC._tensors({"lens_mass": c["lens_params"]}, MC.F64)["lens_mass"]]
    T = mp.target_scales(z)

    def f(x, y):
        sums = exact_plane_sums(phys, mp, lp, x, y)
        ax = sum(float(T[i]) * sums[i][0] for i in range(mp.K) if T[i] != 0.0)
        ay = sum(float(T[i]) * sums[i][1] for i in range(mp.K) if T[i] != 0.0)
        return ax, ay
    return f


def polished_images(name, b, s, tol=1e-12):
    """The float64 images (``images_cases._solve64`` at twice the general grid) of source s of sample b of
    ``mp_images_cases.GENERAL[name]`` on the float64 couplings, Newton-polished to a residual <= tol: ``[n, 2]``."""
    from tests import images_cases as IC
    z, srcx, srcy = MI.general_sources(name)
    deriv = exact_deriv64(name, b, z[s])
    sx, sy = float(srcx[b, s]), float(srcy[b, s])
    ref = IC._solve64(deriv, sx, sy, MI.GENERAL_WINDOW, 2 * MI.GENERAL_CELLS)
    x, y = torch.as_tensor(ref[:, 0].copy()), torch.as_tensor(ref[:, 1].copy())
    for _ in range(8):
        bx, by, fxx, fxy, fyx, fyy = IC._beta_jac(deriv, x, y)
        rx, ry = sx - bx, sy - by
        if float(torch.hypot(rx, ry).max()) <= tol:
            break
        a00, a01, a10, a11 = 1 - fxx, -fxy, -fyx, 1 - fyy
        det = a00 * a11 - a01 * a10
        x, y = x + (a11 * rx - a01 * ry) / det, y + (a00 * ry - a10 * rx) / det
    res = IC._residual64(deriv, x.numpy(), y.numpy(), sx, sy)
    assert np.all(res <= tol), (name, b, s, res)
    return np.stack([x.numpy(), y.numpy()], axis=1)


def reference_gradient(name, b, s, x, y, h=1e-6, exact=True):
    """Central-difference gradient in theta of the composed reference T of sample b, source s of ``GENERAL[name]`` at the float64 points
    ``x, y`` ``[n]``: ``[n, 2]``."""
    c = MC.map_case(name)
    z, srcx, srcy = MI.general_sources(name)
    geom, pot = weights(c["mp"], [z[s]])
    lp = [{k: v[b:b + 1] for k, v in d.items()} for d in c["lens_params"]]
    sx, sy = srcx[b:b + 1, s:s + 1], srcy[b:b + 1, s:s + 1]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    px = np.concatenate([x + h, x - h, x, x])[None, None, :]
    py = np.concatenate([y, y, y + h, y - h])[None, None, :]
    T = reference_T(c["phys"], c["mp"], lp, px, py, sx, sy, geom, pot, exact)[0][0, 0].reshape(4, -1)
    return np.stack([(T[0] - T[1]) / (2 * h), (T[2] - T[3]) / (2 * h)], axis=1)


# ---- the closed form: an SIS on plane 1, a Shear with gamma = 0 on plane 2, a source on the reference plane ---------------------------
SIS_THETA_E, SIS_BETA = np.float32(1.0), np.float32(0.3)
SIS_WINDOW = (-2.0 + MC.OFF, 2.0 + MC.OFF, -2.0 + MC.OFF, 2.0 + MC.OFF)  # 16 cells of 0.25: no vertex on the centre
SIS_CELLS = 16


def sis_case():
    """``(phys, phys_mp, mp, lens_params [B = 1])``.  The empty second plane leaves theta_2 = theta - C_12 alpha_1 a point on the straight
    line from theta_1 to beta (for a source at z_ref, where T_s = (1, 1)), so T is the single-plane D_dt phi with g_1 = D_dt H0 / c of
    the first plane and the source: images at ``beta +- theta_E`` and ``T(-) - T(+) = g_1 2 theta_E beta``, whatever lies on plane 2."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    mp = MC._mp([0.4, 1.0])
    lp = [{"theta_E": MC._f32(SIS_THETA_E), "center_x": MC._f32(0.0), "center_y": MC._f32(0.0)},
          {"gamma1": MC._f32(0.0), "gamma2": MC._f32(0.0)}]
    lenses = [SIS(), Shear()]
    return PhysicalModel(lenses, [], []), PhysicalModel(lenses, [], [], multiplane=mp), mp, lp


def sis_closed_form(mp):
    """``g_1 2 theta_E beta`` with the one-plane weight of plane 1 and a source at z_ref."""
    from gigalens_amd.cosmology import comoving_distance
    c1, cs = float(comoving_distance(mp.z_planes[0], mp.omega_m)), float(comoving_distance(mp.z_ref, mp.omega_m))
    return c1 * cs / (cs - c1) * 2.0 * float(SIS_THETA_E) * float(SIS_BETA)
