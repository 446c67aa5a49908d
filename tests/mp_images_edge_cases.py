"""Cases and float64 references of the lens-equation solver on lens planes at its plane, grid and list edges
(tests/test_gpu_mp_images_edges.py runs the kernels of gl_multiplane_images.hip.h against them; tests/test_mp_images_edges_host.py asserts
without a GPU every condition that the cases put on their own inputs).

Nothing is restated that exists: the scan is ``images_cases.scan64``, fed ``plane_beta`` -- the float64 recursion of
tests/multilens_cases.py (``plane_sums`` + ``target_beta``) on one sample and one coupling row; the solver is ``mp_images_cases.solve64``.
New here:

* the FLAG RULE of the map kernel per plane (``plane_beta(..., flags=True)``): a vertex value is NaN where the ray sits bit for bit on the
  centre of an SIS / SIE / EPL ON THAT LENS'S OWN PLANE (``theta_j``, not ``theta``), for a plane with ``T_j != 0``; the ray is then not
  finite on every later plane, so every later plane with ``T != 0`` inherits the NaN; a plane with ``T_j == 0`` (at or behind the
  source) never flags.  (The oracle's SIS returns 0 on its centre, so the rule is stated on the positions, not left to a 0 / 0.)
* EXACT LINEAR MAPS: Shear lenses on planes of their own with dyadic shears, dyadic couplings ``C_ij`` (``MultiPlane.lens_scales`` is
  replaced before the simulator is built: the library takes any finite, positive, strictly upper triangular matrix) and dyadic target
  rows passed natively.  ``d theta_j = I - sum_{i<j} C_ij G_i d theta_i`` and ``A_t = I - sum_i T_i G_i d theta_i`` in closed form
  (``linear_jacobian``; ``multilens_cases.two_shear_case`` is its K = 2).  On the quarter-cell lattices below every source
  ``A_t theta`` is a float32 number and every product and sum of the scan is exact in float32 and float64 alike."""
import functools

import numpy as np
import torch

from tests import images_cases as IC
from tests import mp_images_cases as C
from tests import multilens_cases as MC

SQUARE, RECT = (-2.0, 2.0, -2.0, 2.0), (-1.0, 3.0, -1.5, 0.5)
LATTICES = [(SQUARE, 4), (SQUARE, 8), (RECT, 8)]
Z_PLANES = [0.3, 0.6, 0.9, 1.2]  # (redshifts only order the planes here: the couplings are replaced)


# ---- the float64 map of one sample on one coupling row ---------------------------------------------------------------------------------
def sample_params(lens_params, b):
    """Sample b of a list of dicts of [B] float32 arrays, as float64 scalars tensors."""
    return [{k: v[b] for k, v in d.items()} for d in MC._tensors({"lens_mass": lens_params}, MC.F64)["lens_mass"]]


def plane_positions(mp, sums, x, y):
    """``[(theta_jx, theta_jy)]`` of the rays on every plane from the plane sums (the recursion of ``multilens_cases.plane_sums``)."""
    Cij = torch.as_tensor(np.asarray(mp.lens_scales, dtype=np.float32)).to(x.dtype)
    out = []
    for j in range(mp.K):
        xj, yj = x, y
        for i in range(j):
            xj, yj = xj - Cij[i, j] * sums[i][0], yj - Cij[i, j] * sums[i][1]
        out.append((xj, yj))
    return out


def plane_beta(phys, mp, lens_params, b, target, flags=True):
    """``beta(X, Y) -> (bx, by)`` on float64 numpy arrays for ``images_cases.scan64``: sample b on the coupling row ``target``, with
    the flag rule of the module docstring when ``flags``."""
    lp = sample_params(lens_params, b)
    T = np.asarray(target, dtype=np.float32).astype(np.float64)

    def beta(X, Y):
        shape = np.shape(X)
        x = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64)).reshape(-1)
        y = torch.as_tensor(np.ascontiguousarray(Y, dtype=np.float64)).reshape(-1)
        sums = MC.plane_sums(phys, mp, lp, x, y)
        bx, by = MC.target_beta(sums, x, y, T)
        if flags:
            # `flagged` runs through the planes in order: once set it stays set, which is the inheritance of the later planes
            flagged = torch.zeros_like(x, dtype=torch.bool)
            for j, (xj, yj) in enumerate(plane_positions(mp, sums, x, y)):
                if T[j] == 0.0:  # a plane at or behind the source is not part of its ray
                    continue
                for l, lens in enumerate(phys.lenses):
                    if int(mp.plane_of_lens[l]) == j and type(lens).__name__ in C.SINGULAR:
                        flagged |= (xj == lp[l]["center_x"]) & (yj == lp[l]["center_y"])
            nan = torch.full_like(x, float("nan"))
            bx, by = torch.where(flagged, nan, bx), torch.where(flagged, nan, by)
        return bx.numpy().reshape(shape), by.numpy().reshape(shape)
    return beta


def scan(phys, mp, lens_params, b, target, window, n, sx, sy, flags=True):
    with np.errstate(all="ignore"):
        return IC.scan64(plane_beta(phys, mp, lens_params, b, target, flags), window, n, float(sx), float(sy))


def _model(lenses, z_lenses, couplings=None):
    """``(phys, phys_mp, mp)``; ``couplings`` {(i, j): C_ij} replaces ``mp.lens_scales``."""
    from gigalens_amd.model import PhysicalModel
    mp = MC._mp(z_lenses)
    if couplings is not None:
        Cm = np.zeros((mp.K, mp.K))
        for (i, j), v in couplings.items():
            Cm[i, j] = v
        assert all(Cm[i, j] > 0 for i in range(mp.K) for j in range(i + 1, mp.K))
        mp.lens_scales = Cm
    return PhysicalModel(lenses, [], []), PhysicalModel(lenses, [], [], multiplane=mp), mp


# ---- exact linear maps ------------------------------------------------------------------------------------------------------------
_K3_SHEARS = [(0.0, 0.5), (0.25, 0.0), (-0.5, 0.25)]
_K3_C = {(0, 1): 0.5, (0, 2): 0.75, (1, 2): 0.5}
# name -> (shears per plane (g1, g2), couplings above the diagonal, target row)
LINEAR = {
    "rot": ([(0.0, 0.5), (0.25, 0.0)], {(0, 1): 0.5}, (1.0, 1.0)),
    "neg": ([(1.5, 0.0), (0.0, 0.5)], {(0, 1): 0.5}, (1.0, 1.0)),
    "front": ([(0.0, 0.5), (0.25, 0.0)], {(0, 1): 0.5}, (0.5, 0.0)),
    "k3": (_K3_SHEARS, _K3_C, (1.0, 1.0, 0.5)),
    "k4": (_K3_SHEARS + [(0.25, 0.25)], {**_K3_C, (0, 3): 0.875, (1, 3): 0.75, (2, 3): 0.5}, (1.0, 1.0, 1.0, 1.0)),
}
# det A_t and A_xy - A_yx of the maps (the issue's table; tests/test_mp_images_edges_host.py holds linear_jacobian to it)
LINEAR_TABLE = {"rot": (0.6914, 0.125), "neg": (-1.359, -0.75), "front": (0.9375, 0.0), "k3": (0.6528, -0.094), "k4": (0.3840, -0.002)}


def linear_jacobian(shears, couplings, target):
    """``A_t`` [2, 2] of Shear planes: ``D_j = I - sum_{i<j} C_ij G_i D_i``, ``A_t = I - sum_i T_i G_i D_i``."""
    G = [MC.shear_matrix(g1, g2) for g1, g2 in shears]
    D = []
    for j in range(len(G)):
        Dj = np.eye(2)
        for i in range(j):
            Dj = Dj - couplings[i, j] * G[i] @ D[i]
        D.append(Dj)
    A = np.eye(2)
    for i, t in enumerate(target):
        if t != 0.0:
            A = A - t * G[i] @ D[i]
    return A


def front_row(K):
    """The coupling row of a source between planes 0 and 1."""
    return (0.5,) + (0.0,) * (K - 1)


def shear_params(shear_rows):
    """``shear_rows`` [B][K] of (g1, g2) -> list of K dicts of [B] float32 arrays."""
    rows = np.asarray(shear_rows, dtype=np.float32)
    return [{"gamma1": rows[:, k, 0].copy(), "gamma2": rows[:, k, 1].copy()} for k in range(rows.shape[1])]


@functools.lru_cache(maxsize=None)
def linear_model(K):
    """Shear | ... | Shear on K planes with the dyadic couplings of ``k4`` (its leading K x K block: those of rot / neg / k3)."""
    from gigalens_amd.profiles.mass.shear import Shear
    couplings = {ij: v for ij, v in LINEAR["k4"][1].items() if ij[1] < K}
    return _model([Shear() for _ in range(K)], Z_PLANES[:K], couplings) + (couplings,)


def linear_case(name):
    """``dict(phys, phys_mp, mp, shears, couplings, target, A)`` of a map of ``LINEAR``."""
    shears, couplings, target = LINEAR[name]
    phys, phys_mp, mp, model_c = linear_model(len(shears))
    assert model_c == couplings
    return dict(phys=phys, phys_mp=phys_mp, mp=mp, shears=shears, couplings=couplings, target=target,
                A=linear_jacobian(shears, couplings, target))


def jac_tuple(A):
    return ((float(A[0, 0]), float(A[0, 1])), (float(A[1, 0]), float(A[1, 1])))


# the tie-rule cases: a lens set, and the two coupling rows its sources alternate between (even: behind every plane of the table's
# row; odd: between planes 0 and 1)
TIE_MAPS = ("rot", "neg", "k3")


def tie_rows(name):
    """``(case, [row of even sources, row of odd sources], [A_t of each])``; for ``rot`` the odd row is the map ``front``."""
    c = linear_case(name)
    rows = [c["target"], front_row(len(c["shears"]))]
    return c, rows, [linear_jacobian(c["shears"], c["couplings"], r) for r in rows]


TIE_S = 363  # sources per sample of a tie-rule call: (4 n + 1)^2 = 289 lattice points in one sample, or 1089 = 3 x 363


def tie_sources(name, window, n):
    """The quarter-cell lattice in the order of a call [B, S] (S = min(P, TIE_S)): lattice point k is source s = k % S of sample
    k // S and sits on row s % 2 (the coupling rows belong to the sources, shared by the samples).  theta x, y [P], boundary [P],
    source x, y [P] (float64), the row index [P]."""
    _, _, As = tie_rows(name)
    X, Y, boundary = IC.quarter_lattice(window, n)
    row = (np.arange(len(X)) % min(len(X), TIE_S)) % 2
    SX, SY = np.empty_like(X), np.empty_like(Y)
    for r, A in enumerate(As):
        sx, sy = IC.apply_jac(jac_tuple(A), X, Y)
        SX[row == r], SY[row == r] = sx[row == r], sy[row == r]
    return X, Y, boundary, SX, SY, row


# the wave-range cases: K -> the shears of the three samples (B = 3, a different dyadic map in each) and the coupling row
WAVE_CELLS = {2: (1, 2, 5, 8, 12, 16), 3: (5, 8), 4: (1, 5, 16)}  # (K = 3, n = 5: V = 36, an odd vertex count against the stride 3)
WAVE_SHEARS = {
    2: [LINEAR["rot"][0], LINEAR["neg"][0], [(0.25, 0.25), (-0.5, 0.0)]],
    3: [_K3_SHEARS, [(0.25, 0.0), (-0.5, 0.25), (0.0, 0.5)], [(-0.5, 0.25), (0.0, -0.5), (0.25, 0.25)]],
    4: [LINEAR["k4"][0], [(0.25, 0.25), (0.0, 0.5), (0.25, 0.0), (-0.5, 0.25)], [(-0.5, 0.25), (0.25, 0.25), (0.0, -0.5), (0.25, 0.0)]],
}
WAVE_ROW = {2: (1.0, 1.0), 3: (1.0, 1.0, 0.5), 4: (1.0, 1.0, 1.0, 1.0)}


def wave_case(K):
    """``(phys, phys_mp, mp, lens_params [B = 3], target row, [A_t of each sample])``."""
    phys, phys_mp, mp, couplings = linear_model(K)
    return (phys, phys_mp, mp, shear_params(WAVE_SHEARS[K]), WAVE_ROW[K],
            [linear_jacobian(s, couplings, WAVE_ROW[K]) for s in WAVE_SHEARS[K]])


# ---- flag rules per plane -----------------------------------------------------------------------------------------------------------
FLAG_WINDOW, FLAG_CELLS = SQUARE, 8  # cells of 0.5: the vertices are multiples of 0.5
FAR = 40.0  # a singular centre moved far outside the window: (centre + FAR) on both axes


def _shear_plane(g1, g2):
    return {"gamma1": MC._f32(g1), "gamma2": MC._f32(g2)}


def _sis_plane(theta_E, cx, cy):
    return {"theta_E": MC._f32(theta_E), "center_x": MC._f32(cx), "center_y": MC._f32(cy)}


@functools.lru_cache(maxsize=None)
def flag_case(name):
    """``dict(phys, phys_mp, mp, lens_params [B = 1], far (the same with the SIS moved FAR away), vertex (theta_v of the flagged
    vertex), rows [S, K], flagged [S] (does source s lose the six triangles?), sx, sy [S] float32)``.  The sources were picked on the
    CPU so that every live triangle's decision holds by ``images_cases.RING_MARGIN`` (tests/test_mp_images_edges_host.py asserts it).

    front:  SIS (plane 0, centre ON the vertex (0, 0)) | Shear: every source is behind plane 0 and loses the six triangles.
    second: Shear | SIS with its centre at ``theta_1(v) = (I - C_01 G_0) theta_v``, v = (0.5, -0.5): the source behind both loses them,
            the source between the planes (row (t0, 0)) does not.
    third:  Shear | Shear | SIS with its centre at ``theta_2(v)``: a source between planes 1 and 2 (row (1, 0.5, 0)) and one behind all.
    A source in front of the singular plane has its image in one of the six triangles of v: flagged by mistake, it loses its hit."""
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    if name == "front":
        lenses, K, v = [SIS(), Shear()], 2, (0.0, 0.0)
        lp = lambda cx, cy: [_sis_plane(0.75, cx, cy), _shear_plane(0.25, 0.0)]
        centre = v
        rows, flagged = [(1.0, 1.0), (0.5, 0.0), (1.0, 0.5)], [True, True, True]
        sx, sy = [0.05, 0.3, -0.2], [0.02, -0.1, 0.4]
    elif name == "second":
        lenses, K, v = [Shear(), SIS()], 2, (0.5, -0.5)
        lp = lambda cx, cy: [_shear_plane(0.0, 0.5), _sis_plane(0.75, cx, cy)]
        centre = (0.5 - 0.5 * (0.5 * -0.5), -0.5 - 0.5 * (0.5 * 0.5))  # theta_v - C_01 (g2 y, g2 x)
        rows, flagged = [(1.0, 1.0), (0.5, 0.0), (1.0, 0.5)], [True, False, True]
        sx, sy = [0.3, 0.7125, -0.2], [-0.25, -0.6, 0.1]  # (the second: A theta at theta = v + (0.1, 0.05), row (0.5, 0))
    elif name == "third":
        lenses, K, v = [Shear(), Shear(), SIS()], 3, (0.5, -0.5)
        lp = lambda cx, cy: [_shear_plane(0.0, 0.5), _shear_plane(0.25, 0.0), _sis_plane(0.75, cx, cy)]
        a0 = (0.5 * -0.5, 0.5 * 0.5)                       # G_0 theta_v
        t1 = (0.5 - 0.5 * a0[0], -0.5 - 0.5 * a0[1])       # theta_1 = theta_v - C_01 a_0
        a1 = (0.25 * t1[0], -0.25 * t1[1])                 # G_1 theta_1
        centre = (0.5 - 0.75 * a0[0] - 0.5 * a1[0], -0.5 - 0.75 * a0[1] - 0.5 * a1[1])
        rows, flagged = [(1.0, 0.5, 0.0), (1.0, 1.0, 0.5)], [False, True]
        sx, sy = [0.7359375, 0.3], [-0.825, -0.2]  # (the first: A theta at theta = v + (0.1, 0.05), row (1, 0.5, 0))
    else:
        raise KeyError(name)
    couplings = {ij: c for ij, c in LINEAR["k4"][1].items() if ij[1] < K}
    phys, phys_mp, mp = _model(lenses, Z_PLANES[:K], couplings)
    return dict(phys=phys, phys_mp=phys_mp, mp=mp, lens_params=lp(*centre), far=lp(centre[0] + FAR, centre[1] + FAR), vertex=v,
                centre=centre, rows=np.asarray(rows, dtype=np.float32), flagged=flagged, sx=np.asarray(sx, dtype=np.float32),
                sy=np.asarray(sy, dtype=np.float32))


FLAG_CASES = ("front", "second", "third")


def vertex_triangles(v, window, n):
    """The six triangles (ids in the order of ``images_cases.scan64``) that hold the vertex at ``v``, an interior vertex."""
    xs, ys = IC.grid_vertices(window, n)
    i, j = int(np.argmin(np.abs(xs - v[0]))), int(np.argmin(np.abs(ys - v[1])))
    assert xs[i] == v[0] and ys[j] == v[1] and 0 < i < n and 0 < j < n
    V1, out = n + 1, []
    for cj, ci in ((j - 1, i - 1), (j - 1, i), (j, i - 1), (j, i)):
        v00 = cj * V1 + ci
        for k, tri in enumerate(((v00, v00 + 1, v00 + V1 + 1), (v00, v00 + V1 + 1, v00 + V1))):
            if j * V1 + i in tri:
                out.append(2 * (cj * n + ci) + k)
    assert len(out) == 6
    return sorted(out)


@functools.lru_cache(maxsize=None)
def flag_scans(name, far=False):
    """``images_cases.scan64`` with the restated flag for every source of a flag case (computed once and shared)."""
    c = flag_case(name)
    lp = c["far"] if far else c["lens_params"]
    return [scan(c["phys"], c["mp"], lp, 0, c["rows"][s], FLAG_WINDOW, FLAG_CELLS, c["sx"][s], c["sy"][s]) for s in range(len(c["sx"]))]


# ---- the candidate list: the Einstein ring of images_cases.RING_CASES through two planes ----------------------------------------------
RING_ROW = (1.0, 1.0)
RING_PLACEMENTS = (0, 1)  # the plane that holds the SIS; a zero Shear holds the other


@functools.lru_cache(maxsize=None)
def ring_case(n, sis_plane):
    """``(phys, phys_mp, mp, lens_params [B = 1], cx, cy)``: SIS (theta_E = 1, the centre of RING_CASES[n]) on plane ``sis_plane``, a
    Shear of zero on the other, C_01 = 0.5.  With the row (1, 1) the vertex values are the float32 numbers of the single-plane case:
    SIS in front, ``(x - 1 a_0) - 1 * 0``; SIS behind, ``theta_1 = theta - 0.5 * 0 = theta`` exactly and ``(x - 1 * 0) - 1 a_1``."""
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    (cx, cy), _, _ = IC.RING_CASES[n]
    cx, cy = float(np.float32(cx)), float(np.float32(cy))
    planes = [_sis_plane(1.0, cx, cy), _shear_plane(0.0, 0.0)]
    lenses = [SIS(), Shear()]
    if sis_plane == 1:
        planes, lenses = planes[::-1], lenses[::-1]
    return _model(lenses, Z_PLANES[:2], {(0, 1): 0.5}) + (planes, cx, cy)


@functools.lru_cache(maxsize=None)
def ring_scan(n, sis_plane):
    phys, _, mp, lp, cx, cy = ring_case(n, sis_plane)
    return scan(phys, mp, lp, 0, RING_ROW, IC.RING_WINDOW, n, cx, cy)


# ---- max_images: the four-plane case of mp_images_cases, one multiply imaged source ------------------------------------------------
MAX_IMAGES_SOURCE = (0.05, 0.03)
MAX_IMAGES_Z = 2.0


@functools.lru_cache(maxsize=None)
def max_images_reference():
    phys, _, mp, lp = C.four_plane_case()
    return C.solve64(phys, mp, lp, 0, mp.target_scales(MAX_IMAGES_Z), *MAX_IMAGES_SOURCE, C.GENERAL_WINDOW, 2 * C.GENERAL_CELLS)


# ---- every lens set and other windows against the float64 solver -------------------------------------------------------------------
# (the three lens sets of multilens_cases.MAP_CASES that mp_images_cases.GENERAL did not hold are added THERE, with sources of their
# own: tests/test_gpu_mp_images.py and tests/test_mp_images_host.py run over GENERAL.)  The other windows of the two first sets:
# 24 cells of 0.25 x 1/6 off-centre, and 40 cells of 0.15 x 0.1 -- vertices at multiples of 0.05 or thirds of 0.5, never on a lens centre
WINDOWS = [(24, (-2.5, 3.5, -2.0, 2.0)), (40, (-3.0, 3.0, -2.0, 2.0))]
# (lens set, cells) -> source_x, source_y [B = 3, S = 2] at the redshifts of mp_images_cases.GENERAL[set]; picked on the CPU for each
# window (the fold rule and the distance to a singular centre are counted in cells of the window in use), and so that the solver's
# procedure run in float64 (``procedure64`` below) yields every compared image: on the 24-cell window a first choice for
# ``epl_shear|sie`` held an image (mu = -8.3, 1.4 cells from the EPL centre) whose seed lies 0.19 from it, from where the clamped
# Newton steps end on the other image -- in float64 as on the GPU
WINDOW_SOURCES = {
    ("epl_shear|sie", 24): ([[-0.12, -0.14], [-0.06, 0.07], [0.0, 0.11]], [[-0.08, -0.06], [-0.07, 0.14], [0.13, -0.05]]),
    ("epl_shear|sie", 40): ([[0.04, 0.12], [0.08, -0.08], [-0.06, 0.11]], [[-0.15, 0.1], [0.09, -0.01], [-0.06, -0.07]]),
    ("nfw|dpie|sis", 24): ([[0.03, 0.04], [0.05, -0.1], [-0.02, -0.08]], [[-0.03, -0.12], [0.14, -0.09], [0.05, -0.06]]),
    ("nfw|dpie|sis", 40): ([[-0.04, -0.15], [0.1, -0.1], [-0.07, 0.11]], [[0.0, 0.1], [0.04, 0.07], [-0.12, 0.01]]),
}
WINDOW_SETS = ("epl_shear|sie", "nfw|dpie|sis")


def window_sources(name, n_cells):
    sx, sy = WINDOW_SOURCES[name, n_cells]
    return C.GENERAL[name][0], np.asarray(sx, dtype=np.float32), np.asarray(sy, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def window_reference(name, n_cells, window):
    """``{(b, s): [K, 3]}`` of the float64 solver at ``2 n_cells`` on the sources of the window."""
    c = MC.map_case(name)
    z, sx, sy = window_sources(name, n_cells)
    return {(b, s): C.solve64(c["phys"], c["mp"], c["lens_params"], b, c["mp"].target_scales(z[s]), sx[b, s], sy[b, s], window,
                              2 * n_cells) for b in range(3) for s in range(2)}


def window_vertices(n_cells, window):
    """The vertices of a window as float32 values, x [V], y [V]."""
    xs, ys = IC.grid_vertices(window, n_cells)
    X, Y = np.meshgrid(xs.astype(np.float32), ys.astype(np.float32))
    return X.ravel(), Y.ravel()


# a map whose Jacobian is far from symmetric AND not constant: two strong Shear planes (those of ``neg``, on the couplings of their
# redshifts) with an SIS beside the second.  Newton on the transpose of A_t contracts by ``transposed_newton_rate`` a step -- too slowly
# for max_iter = 30 -- so an evaluation that mixes up f_xy and f_yx loses these images, where the general sets (rotation of order
# 1e-2) would hide it behind a few more iterations.
ROTATED_WINDOW, ROTATED_CELLS = (-2.4, 2.4, -2.4, 2.4), 32
ROTATED_Z = (0.7, 2.0, 2.0)
ROTATED_SOURCES = ([[0.3, 0.12, 0.5]], [[-0.2, 0.25, 0.4]])  # source_x, source_y [B = 1, S = 3]
ROTATED_RATE = 0.8  # 0.8^30 = 1e-3: from a seed a fraction of a cell off, 30 steps do not reach tol ~ 1e-6


@functools.lru_cache(maxsize=None)
def rotated_case():
    """``(phys, phys_mp, mp, lens_params [B = 1])``: Shear (1.5, 0) at z = 0.4 | Shear (0, 0.5) + SIS at z = 1.0."""
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    lp = [_shear_plane(1.5, 0.0), _shear_plane(0.0, 0.5), _sis_plane(0.6, 2 * MC.PIX + MC.OFF, -MC.PIX + MC.OFF)]
    return _model([Shear(), Shear(), SIS()], [0.4, 1.0, 1.0]) + (lp,)


def transposed_newton_rate(A):
    """Spectral radius of ``I - (A')^-1 A`` with ``A'`` = A with its off-diagonal entries swapped: the factor by which a Newton step on
    the transposed Jacobian shrinks the error near a root of a map with Jacobian A."""
    At = np.array([[A[0, 0], A[1, 0]], [A[0, 1], A[1, 1]]])
    return float(np.abs(np.linalg.eigvals(np.eye(2) - np.linalg.solve(At, A))).max())


@functools.lru_cache(maxsize=None)
def rotated_reference():
    """``{s: [K, 3]}`` of the float64 solver at ``2 ROTATED_CELLS``, and the transposed-Newton rate at each image ``{s: [K]}``."""
    phys, _, mp, lp = rotated_case()
    ref, rate = {}, {}
    for s, z in enumerate(ROTATED_Z):
        T = mp.target_scales(z)
        ref[s] = C.solve64(phys, mp, lp, 0, T, np.float32(ROTATED_SOURCES[0][0][s]), np.float32(ROTATED_SOURCES[1][0][s]),
                           ROTATED_WINDOW, 2 * ROTATED_CELLS)
        m = MC.maps(phys, mp, lp, ref[s][:, 0], ref[s][:, 1], T)[:, :, 0]
        rate[s] = [transposed_newton_rate(np.array([[m[2, i], m[3, i]], [m[4, i], m[5, i]]])) for i in range(len(ref[s]))]
    return ref, rate


# ---- what the tie-rule test expects, and the exactness of its inputs ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_want(name, window, n):
    """``n_cand`` of every lattice point of ``tie_sources`` from ``images_cases.scan64`` on the recursion: 1 inside (every product of the
    scan is exact, and an interior point of a non-singular linear map lies in one triangle under the tie rule), the scan's own count on
    the boundary.  [P] int64 (left unchanged)."""
    c, rows, _ = tie_rows(name)
    lp = shear_params([c["shears"]])
    X, Y, boundary, SX, SY, row = tie_sources(name, window, n)
    want = np.ones(len(X), dtype=np.int64)
    for k in np.flatnonzero(boundary):
        want[k] = len(scan(c["phys"], c["mp"], lp, 0, rows[row[k]], window, n, SX[k], SY[k])["hits"])
    want.setflags(write=False)
    return want


def grid_edges(n):
    """(lo, hi) vertex indices, lo < hi, of every edge of the triangulation of ``images_cases.scan64``: horizontal, vertical, diagonal."""
    V1 = n + 1
    v = np.arange(V1 * V1).reshape(V1, V1)
    pairs = [(v[:, :-1], v[:, 1:]), (v[:-1, :], v[1:, :]), (v[:-1, :-1], v[1:, 1:])]
    return np.concatenate([p[0].ravel() for p in pairs]), np.concatenate([p[1].ravel() for p in pairs])


def edge_functions(bx, by, n, sx, sy, dtype):
    """The edge function of ``scan64`` / ``img_edge`` of every grid edge [E] at every source [P], evaluated in ``dtype`` operation by
    operation: ``(q.x - p.x) (s.y - p.y) - (q.y - p.y) (s.x - p.x)``.  [E, P] float64."""
    lo, hi = grid_edges(n)
    bx, by, sx, sy = (np.asarray(a, dtype=dtype) for a in (bx, by, sx, sy))
    ex, ey = (bx[hi] - bx[lo])[:, None], (by[hi] - by[lo])[:, None]
    ry, rx = sy[None, :] - by[lo][:, None], sx[None, :] - bx[lo][:, None]
    a, b = (ex * ry).astype(dtype), (ey * rx).astype(dtype)
    return (a - b).astype(dtype).astype(np.float64)


def procedure64(phys, mp, lens_params, b, target, sx, sy, window, n, max_iter=30, tol=1e-9):
    """The solver's own procedure in float64: the seeds of ``images_cases.scan64`` on the recursion, each taken through Newton with
    the kernel's rule (a step is at most one cell diagonal, ``max_iter`` steps).  Returns the points reached [K, 2] (those outside
    the window and those that did not converge to ``tol`` left out).  On a coarse grid a seed beside the centre of an EPL / SIE / SIS
    can lie so far from its image that the clamped iteration ends in the basin of another one -- in exact arithmetic too: which
    images a grid yields is a property of the procedure, and the window cases pick sources whose images it all yields."""
    deriv = C.deriv64(phys, mp, lens_params, b, target)
    seeds = scan(phys, mp, lens_params, b, target, window, n, sx, sy, flags=False)["seeds"]
    if not len(seeds):
        return np.zeros((0, 2))
    x, y = (torch.as_tensor(seeds[:, k].copy()) for k in (0, 1))
    step_max = float(np.hypot((window[1] - window[0]) / n, (window[3] - window[2]) / n))
    for _ in range(max_iter):
        bx, by, fxx, fxy, fyx, fyy = IC._beta_jac(deriv, x, y)
        rx, ry = float(sx) - bx, float(sy) - by
        a00, a01, a10, a11 = 1 - fxx, -fxy, -fyx, 1 - fyy
        det = a00 * a11 - a01 * a10
        dx, dy = (a11 * rx - a01 * ry) / det, (a00 * ry - a10 * rx) / det
        scale = torch.clamp(step_max / torch.hypot(dx, dy).clamp(min=1e-300), max=1.0)
        x, y = x + dx * scale, y + dy * scale
    res = IC._residual64(deriv, x.numpy(), y.numpy(), float(sx), float(sy))
    ok = (res <= tol) & (x.numpy() >= window[0]) & (x.numpy() <= window[1]) & (y.numpy() >= window[2]) & (y.numpy() <= window[3])
    return np.stack([x.numpy()[ok], y.numpy()[ok]], axis=1)


def yields_every_image(phys, mp, lens_params, b, target, sx, sy, window, n, ref):
    """Does ``procedure64`` reach every image of ``ref`` [K, 3] above the |mu| gate?"""
    got = procedure64(phys, mp, lens_params, b, target, sx, sy, window, n)
    return all(len(got) and np.hypot(got[:, 0] - r[0], got[:, 1] - r[1]).min() <= 1e-6 for r in ref if abs(r[2]) >= C.MU_MIN)
