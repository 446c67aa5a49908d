"""Cases and float64 references of the lens-equation solver on lens planes (gl_multiplane_image_positions;
``LensSimulator.image_positions(source_redshifts=...)``).  tests/test_mp_images_host.py pins the references against closed forms
without a GPU, tests/test_gpu_mp_images.py runs the kernels against them.

Nothing is restated here: the reference deflection of a target plane is ``deriv(x, y) = (x - beta_x, y - beta_y)`` from the float64
recursion of tests/multilens_cases.py (``plane_sums`` + ``target_beta``, on the float32 couplings the library receives), and it is fed
to the float64 solver and residual of tests/images_cases.py (``_solve64``, ``_residual64``).  ``check_against_f64`` applies the gates of
``images_cases._check_against_f64`` -- residual <= 2 tol, position <= max(5e-5, 2e-6 |mu|), mu to 1e-3 below |mu| = 30, images below
|mu| = 0.02 not compared, a pair with two reference images closer than two cells left to the fold rule -- to a call with
``source_redshifts``."""
import functools
import math

import numpy as np
import torch

from tests import images_cases as IC
from tests import multilens_cases as MC

MU_MIN, FOLD_CELLS = 0.02, 2.0


def deriv64(phys, mp, lens_params, b, target):
    """float64 deflection of the target plane with couplings ``target`` for sample b of ``lens_params`` (a list of dicts of [B]
    float32 arrays): ``(x, y) -> (x - beta_x, y - beta_y)`` on flat float64 tensors."""
    lp = [{k: v[b] for k, v in d.items()} for d in MC._tensors({"lens_mass": lens_params}, MC.F64)["lens_mass"]]

    def f(x, y):
        bx, by = MC.target_beta(MC.plane_sums(phys, mp, lp, x, y), x, y, target)
        return x - bx, y - by
    return f


def solve64(phys, mp, lens_params, b, target, sx, sy, window, n):
    """``images_cases._solve64`` on the target plane: [K, 3] (x, y, mu) sorted by x."""
    return IC._solve64(deriv64(phys, mp, lens_params, b, target), float(sx), float(sy), window, n)


def hessian_mu(maps, phys, mp, lens_params, b, target, ref):
    """``ref`` [K, 3] with its magnifications taken from ``maps`` (``multilens_cases.maps_hessian``) at the reference images.  The
    solver's A_t carries the dPIS convergence excess (as gl_multiplane_maps does), which the derivative of the deflection -- the mu
    of ``solve64`` -- does not: for a lens set with a dPIS the reference mu is that of ``maps_hessian``; the images are the same.
    (``maps`` reads its points as float32 values: that moves mu by |d mu / d theta| 1e-7, far below the gate of 1e-3.)"""
    if maps is None or len(ref) == 0:
        return ref
    m = maps(phys, mp, [{k: v[b:b + 1] for k, v in d.items()} for d in lens_params], ref[:, 0], ref[:, 1], target)[:, :, 0]
    out = ref.copy()
    out[:, 2] = 1.0 / (m[2] * m[5] - m[3] * m[4])
    return out


def fold_pair(ref, window, n_cells):
    """The fold rule of ``_check_against_f64``: two reference images closer than FOLD_CELLS cells."""
    if len(ref) < 2:
        return False
    d = np.hypot(ref[:, None, 0] - ref[None, :, 0], ref[:, None, 1] - ref[None, :, 1]) + np.eye(len(ref)) * 1e9
    return bool(d.min() < FOLD_CELLS * (window[1] - window[0]) / n_cells)


def compare_images(got, ref, tag):
    """The position and magnification gates on one (sample, source) pair; returns the number of images compared."""
    ref_m, got_m = ref[np.abs(ref[:, 2]) >= MU_MIN], got[np.abs(got[:, 2]) >= MU_MIN]
    assert len(ref_m) == len(got_m), (tag, ref, got)
    for r in ref_m:
        j = np.argmin(np.hypot(got_m[:, 0] - r[0], got_m[:, 1] - r[1]))
        dist = math.hypot(got_m[j, 0] - r[0], got_m[j, 1] - r[1])
        print(f"{tag}: image ({r[0]:+.5f}, {r[1]:+.5f}) mu {r[2]:+.4f}: position error {dist:.2e}, "
              f"mu error {abs(got_m[j, 2] - r[2]) / abs(r[2]):.2e}")
        assert dist <= max(5e-5, 2e-6 * abs(r[2])), (tag, r, got_m[j])
        if abs(r[2]) < 30:
            assert abs(got_m[j, 2] - r[2]) <= 1e-3 * abs(r[2]), (tag, r, got_m[j])
    return len(ref_m)


def check_against_f64(sim, phys, mp, lens_params, z_sources, srcx, srcy, window, n_cells, maps=None, **solver):
    """``sim.image_positions(..., source_redshifts=z_sources)`` against the float64 solver at ``2 n_cells``; returns (pairs compared,
    images compared in each).  ``lens_params``: list of dicts of [B] float32 arrays; ``srcx, srcy``: [B, S] float32 arrays;
    ``maps``: where the reference mu comes from when not from the derivative of the deflection (``hessian_mu``)."""
    lt = [{k: torch.as_tensor(v) for k, v in d.items()} for d in lens_params]
    B, S = srcx.shape
    x, y, mu, n = sim.image_positions(lt, torch.as_tensor(srcx), torch.as_tensor(srcy), window=window, num_cells=n_cells,
                                      source_redshifts=z_sources, **solver)
    x, y, mu, n = (t.cpu().numpy() for t in (x, y, mu, n))
    tol = IC._default_tol(window)
    compared, counts = 0, []
    for b in range(B):
        for s in range(S):
            T = mp.target_scales(np.broadcast_to(np.asarray(z_sources, dtype=np.float64), (S,))[s])
            deriv = deriv64(phys, mp, lens_params, b, T)
            sx, sy = float(srcx[b, s]), float(srcy[b, s])
            ref = hessian_mu(maps, phys, mp, lens_params, b, T, IC._solve64(deriv, sx, sy, window, 2 * n_cells))
            k = int(n[b, s])
            got = np.stack([x[b, s, :k], y[b, s, :k], mu[b, s, :k]], axis=1).astype(np.float64)
            assert np.all(np.isfinite(got)) and np.all(np.isnan(x[b, s, k:]))
            res = IC._residual64(deriv, got[:, 0], got[:, 1], sx, sy)
            print(f"b={b} s={s}: {k} image(s), largest residual {res.max() if k else 0.0:.2e} (gate {2 * tol:.2e})")
            assert np.all(res <= 2 * tol), (b, s, res, tol)
            if fold_pair(ref, window, n_cells):
                continue
            counts.append(compare_images(got, ref, f"b={b} s={s}"))
            compared += 1
    return compared, counts


# ---- the general cases: lens sets of multilens_cases.map_case, three samples, two sources at two redshifts ----------------------------
# window: 32 cells of 0.15 -- vertices at multiples of 0.05, never on a lens centre (k PIX + 0.37 PIX)
GENERAL_WINDOW = (-2.4, 2.4, -2.4, 2.4)
GENERAL_CELLS = 32
# name -> (source redshifts, source_x [B, S], source_y [B, S]).  The sources were picked on the CPU (tests/test_mp_images_host.py
# asserts it) so that the float64 solver leaves at most a quarter of the pairs to the fold rule and sees three or more images
# somewhere, and so that no image sits on the cell of a singular lens centre (``singular_centre_cells`` below).
GENERAL = {
    "epl_shear|sie": ((0.8, 2.0), [[0.05, 0.12], [0.12, 0.1], [0.1, -0.06]], [[0.03, -0.07], [-0.08, 0.02], [-0.04, 0.09]]),
    "nfw|dpie|sis": ((1.1, 2.5), [[0.04, 0.1], [-0.06, 0.05], [0.08, -0.05]], [[-0.05, 0.06], [0.03, -0.08], [0.07, 0.04]]),
    # the other three lens sets of multilens_cases.MAP_CASES; first redshift between the last two planes, second behind all
    "shared": ((0.7, 1.8), [[0.14, 0.07], [0.01, -0.07], [-0.1, 0.14]], [[0.0, -0.12], [0.04, 0.08], [0.03, 0.13]]),
    "dpis|sie": ((0.6, 2.0), [[-0.05, 0.13], [-0.01, 0.06], [-0.12, -0.12]], [[-0.09, 0.12], [0.05, 0.1], [0.04, -0.03]]),
    "nfw|dpie|sis>": ((1.1, 2.5), [[0.12, 0.03], [-0.01, 0.08], [-0.14, 0.06]], [[-0.04, -0.12], [0.05, 0.13], [-0.09, 0.04]]),
}


def reference_maps(name):
    """``maps`` of ``check_against_f64`` / ``hessian_mu`` for a lens set: ``maps_hessian`` where ``map_case`` names it, else None."""
    m = MC.map_case(name)["maps"]
    return m if m is MC.maps_hessian else None


def general_sources(name):
    z, sx, sy = GENERAL[name]
    return z, np.asarray(sx, dtype=np.float32), np.asarray(sy, dtype=np.float32)


SINGULAR = ("EPL", "SIE", "SIS")  # deflections that are not differentiable at the centre


def singular_centre_cells(name, b, target, x, y, window=None, n_cells=None):
    """Distance, in cells of the grid in use (``window``, ``n_cells``; default: the general grid), between the ray from ``(x, y)`` and the nearest centre of an EPL / SIE / SIS of sample
    b on a plane in front of the target (``target[plane] != 0``), each measured on the lens's own plane.  The solver promises an
    image only where the map is not folded more finely than a cell (include/gigalens_hip.h): the cell that holds such a centre is folded onto itself however fine the grid, so the triangles
    around it are no affine neighbourhood of an image -- the float64 restatement of the scan (``images_cases.scan64``) misses an
    image half a cell from an EPL centre on this grid just as the kernel does.  The general cases therefore keep every compared
    image at least one cell away from those centres; that is a condition on the chosen sources, asserted on the float64 reference."""
    c = MC.map_case(name)
    return singular_centre_cells_of(c["phys"], c["mp"], c["lens_params"], b, target, x, y, window, n_cells)


def singular_centre_cells_of(phys, mp, lens_params, b, target, x, y, window=None, n_cells=None):
    """``singular_centre_cells`` for any lens set (``lens_params``: list of dicts of [B] float32 arrays)."""
    lp = [{k: v[b:b + 1] for k, v in d.items()} for d in MC._tensors({"lens_mass": lens_params}, MC.F64)["lens_mass"]]
    xt, yt = (torch.as_tensor(np.asarray([[v]], dtype=np.float64)) for v in (x, y))
    sums = MC.plane_sums(phys, mp, lp, xt, yt)
    Cij = np.asarray(mp.lens_scales, dtype=np.float32).astype(np.float64)
    best = math.inf
    for l, lens in enumerate(phys.lenses):
        if type(lens).__name__ not in SINGULAR:
            continue
        j = int(mp.plane_of_lens[l])
        if float(target[j]) == 0.0:
            continue
        xj, yj = xt, yt
        for i in range(j):
            xj, yj = xj - Cij[i, j] * sums[i][0], yj - Cij[i, j] * sums[i][1]
        best = min(best, float(torch.hypot(xj - lp[l]["center_x"], yj - lp[l]["center_y"]).min()))
    window, n_cells = window or GENERAL_WINDOW, n_cells or GENERAL_CELLS
    # (the larger side of a rectangular cell: "one cell away" in either direction)
    return best / (max(window[1] - window[0], window[3] - window[2]) / n_cells)


@functools.lru_cache(maxsize=None)
def general_reference(name):
    """``{(b, s): [K, 3]}`` of the float64 solver at ``2 GENERAL_CELLS`` -- computed once and shared."""
    c = MC.map_case(name)
    z, sx, sy = general_sources(name)
    T = [c["mp"].target_scales(v) for v in z]
    return {(b, s): hessian_mu(reference_maps(name), c["phys"], c["mp"], c["lens_params"], b, T[s],
                               solve64(c["phys"], c["mp"], c["lens_params"], b, T[s], sx[b, s], sy[b, s], GENERAL_WINDOW,
                                       2 * GENERAL_CELLS)) for b in range(3) for s in range(2)}


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
SHEAR_WINDOW = (-1.0, 1.0, -1.0, 1.0)
SHEAR_THETA = np.array([[0.3, -0.2], [-0.55, 0.4], [1.7, 0.3]])  # the roots; the last lies outside the window


def two_shear_sources():
    """``(case, source_x, source_y [1, 3] float32, roots [3, 2], mu)``: beta_s = A theta rounded to float32, and the closed-form root
    ``A^-1 beta_s`` of those float32 values with ``mu = 1 / det A`` (A on the float32 couplings, ``multilens_cases.two_shear_case``)."""
    case = MC.two_shear_case()
    A = case[5]
    beta = (SHEAR_THETA @ A.T).astype(np.float32)
    roots = np.linalg.solve(A, beta.astype(np.float64).T).T
    return case, beta[None, :, 0].copy(), beta[None, :, 1].copy(), roots, 1.0 / np.linalg.det(A)


# window of the coaxial SIS planes: 16 cells of 0.25 from -2 + 0.37 PIX -- no vertex on the axis' centre on either plane
SIS_WINDOW = (-2.0 + MC.OFF, 2.0 + MC.OFF, -2.0 + MC.OFF, 2.0 + MC.OFF)
SIS_CELLS = 16
SIS_BETA = np.array([0.05, 0.2, -0.1], dtype=np.float32)  # sources on the axis


def two_sis_closed_form(beta):
    """The outer images of a source at ``(beta, 0)`` behind both coaxial SIS planes: ``x = beta +- (T_1 tE1 + T_2 tE2)`` where the ray
    passes both centres on the same side (``|x| > C_12 tE1``, so theta_2 has the sign of x).  Returns ``(case, [x+, x-] or fewer)``."""
    case = MC.two_sis_case()
    mp, lp, T = case[2], case[3], case[4]
    C12, T1, T2 = (float(np.float32(v)) for v in (mp.lens_scales[0, 1], T[0], T[1]))
    tE1, tE2 = float(lp[0]["theta_E"][0]), float(lp[1]["theta_E"][0])
    E = T1 * tE1 + T2 * tE2
    return case, [x for x in (float(beta) + E, float(beta) - E) if abs(x) > C12 * tE1 and np.sign(x) == np.sign(x - float(beta))]


def four_plane_case():
    """K = 4 (MP_MAXK): SIS | Shear | SIS | Shear on planes of their own, one sample; the source lies behind all four."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    mp = MC._mp([0.3, 0.6, 0.9, 1.2])
    lp = [{"theta_E": MC._f32(0.9), "center_x": MC._f32(MC.OFF), "center_y": MC._f32(-MC.PIX + MC.OFF)},
          {"gamma1": MC._f32(0.04), "gamma2": MC._f32(-0.03)},
          {"theta_E": MC._f32(0.3), "center_x": MC._f32(2 * MC.PIX + MC.OFF), "center_y": MC._f32(MC.PIX + MC.OFF)},
          {"gamma1": MC._f32(-0.02), "gamma2": MC._f32(0.05)}]
    lenses = [SIS(), Shear(), SIS(), Shear()]
    return PhysicalModel(lenses, [], []), PhysicalModel(lenses, [], [], multiplane=mp), mp, lp
