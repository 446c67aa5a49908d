"""The launch-edge matrix of the point-likelihood kernels (csrc/gl_positions.hip.h, gl_multiplane_pos.hip.h, gl_fluxes.hip.h,
gl_tdelays.hip.h) and its float64 reference: tests/test_points_host.py pins the matrix and its input conditions without a GPU,
tests/test_gpu_points.py runs the kernels against it.

No new restatement: every value comes from ``mp_positions_cases.stats / leaf``, ``flux_cases.stats`` and ``tdelay_cases.stats /
loglike_grad`` called with ``fams=[fam]`` -- one family at a time, so that every (sample, family) element of the kernels' ``w_fam`` has
a float64 value of its own -- and summed in family order.  Only the data recipes are extended: ``with_fluxes`` / ``with_delays`` are
those of the two modules with ``PATTERN`` / ``ERRORS`` cycled for families of more than five images (bit for bit the old recipes
when the sizes match; asserted in the host test).

Lens sets.  ``plain``: EPL + Shear + SIE of ``multilens_cases.map_case("epl_shear|sie")`` on one plane with one Sersic source behind
(P = 18 > L = 13); ``scaled``: the same with two distinct ``centroids_scales`` (``fam_scale`` non-null); ``planes``: those lenses on
the two planes of ``mp_positions_cases.case("k2")``, families between and behind them (P = L = 13); ``zoo1``: dPIS + dPIEP + TNFW +
NFW_ELLIPSE + a 3-member ``DPIESubhalo`` catalogue on one plane (P = L = 26).  Samples beyond the three rows of a set follow
``tdelay_cases.case("b65")``: row ``b % 3``, each value moved by up to 2 % with a phase of its own.

Shapes (B, family sizes) and the thread counts of the four grids of ``run_positions`` -- every kernel runs 64-thread workgroups:

    name   B   sizes                          F   J   B F  B J   B J L (plain 13)  B (P+1) (plain 19 / planes 14)
    one    1   (1)                            1   1     1    1      13                19
    j4     4   (1)                            1   1     4    4      52                76 / 56
    j5     5   (1)                            1   1     5    5      65                95
    bf63   9   (1,2,3,4,2,3,5)                7  20    63  180    2340               171 / 126
    bf64   8   (2,3,1,4,2,5,3,2)              8  22    64  176    2288               152 / 112
    bf65  13   (3,1,6,2,4)                    5  16    65  208    2704               247 / 182
    bj63   7   (2,3,4)                        3   9    21   63     819               133 /  98
    bj64   8   (3,1,4)                        3   8    24   64     832               152 / 112
    bj65   5   (4,3,6)                        3  13    15   65     845 (zoo1 1690)    95 /  70 (zoo1 135)
    long   3   (12,2)                         2  14     6   42     546                57
    many   2   65 families of 1 or 2 images  65 108   130  216    2808                38
    big   33   (1,2,3,4,5,6,2,3,4,1,5,2,3)   13  41   429 1353   17589               627 / 462
    b1     1   sizes of bf64                  8  22     8   22     286                19

B F and B J have a case at 63, 64 and 65.  64 is no multiple of L = 13 / 26 nor of P + 1 = 19 / 14 / 27, so B J L and B (P + 1) cannot
equal 64; they have the nearest count on either side of it, each within L resp. P + 1 of 64: B J L = 52 (``j4``) and 65 (``j5``),
B (P + 1) = 57 (``long``) and 76 (``j4``) on one plane, 56 (``j4``) and 70 (``bj65``) on planes (``edge_counts``; asserted in the host
test).

Measurements (``modes``; the fluxes and the arrival times follow one table): a one-image family has none (the setters refuse a
single measurement); of the others every fourth (f % 4 == 3) has none, every odd one of three or more images misses one image, the
rest are fully measured; the shapes of up to five families name theirs, so that each holds a fully measured family, one with an
unmeasured image and one without a measurement (``long``, two families: the first two kinds).  A delay scale is profiled where f
is even and three or more times are measured, else given: every shape with delays but ``many`` (no family of three) has both.
``big`` holds each of the three kinds at thread indices >= 64, ``many`` the fully measured and the measurement-less; the one thread of
``bf65`` beyond 63 owns a family of four with one unmeasured image.

Every image is a lattice point (``PC.lattice``) on a ring of radius 2.6 - 3.95 arcsec around lenses whose Einstein radii add up to
about 1.5: ``PC.conditions`` >= (MIN_DET, MIN_PIX) and det A of one sign over the samples for every image of every case (asserted in
the host test)."""
import functools

import numpy as np
import torch

from tests import flux_cases as FC
from tests import multilens_cases as MC
from tests import mp_positions_cases as PC
from tests import tdelay_cases as TC

F64, F32 = MC.F64, MC.F32
f = MC._f32

_MANY = tuple(1 + (k * 7 % 3 != 0) for k in range(65))  # 65 families of 1 or 2 images
SHAPES = {
    "one": (1, (1,)),
    "j4": (4, (1,)),
    "j5": (5, (1,)),
    "bf63": (9, (1, 2, 3, 4, 2, 3, 5)),
    "bf64": (8, (2, 3, 1, 4, 2, 5, 3, 2)),
    "bf65": (13, (3, 1, 6, 2, 4)),
    "bj63": (7, (2, 3, 4)),
    "bj64": (8, (3, 1, 4)),
    "bj65": (5, (4, 3, 6)),
    "long": (3, (12, 2)),
    "many": (2, _MANY),
    "big": (33, (1, 2, 3, 4, 5, 6, 2, 3, 4, 1, 5, 2, 3)),
    "b1": (1, (2, 3, 1, 4, 2, 5, 3, 2)),
}
SETS = ("plain", "scaled", "planes", "zoo1")
_ON = {
    "one": ("plain",), "j4": ("plain", "planes"), "j5": ("plain",),
    "bf63": ("plain", "scaled", "planes"), "bf64": ("plain", "scaled", "planes"), "bf65": ("plain", "scaled", "planes"),
    "bj63": ("plain", "planes"), "bj64": ("plain", "planes"), "bj65": ("plain", "planes", "zoo1"),
    "long": ("plain",), "many": ("plain",), "big": ("plain", "planes"), "b1": ("plain",),
}
CASES = tuple((shape, s) for shape in SHAPES for s in _ON[shape])
IDS = tuple(f"{shape}-{s}" for shape, s in CASES)
TERMS = ("positions", "fluxes", "delays")
Z_FAMILIES = (0.8, 2.0)  # the redshifts the families of `scaled` and `planes` alternate between


def has_pairs(shape):
    """Some family of the shape holds two or more images: the flux and delay setters take it."""
    return max(SHAPES[shape][1]) >= 2


def held(shape, lens_set):
    """The terms a case holds data for: delays on one unscaled plane only (they are refused on planes and on scaled families),
    fluxes and delays only where a family can be measured."""
    t = ["positions"]
    if has_pairs(shape):
        t.append("fluxes")
        if lens_set in ("plain", "zoo1"):
            t.append("delays")
    return tuple(t)


def terms_of(shape, lens_set):
    """The terms that run ALONE on a case: those it holds, but for the delays of ``many``.  Every measured family of ``many`` has two
    images, both with times.  For such a family the difference of the two Fermat potentials does not depend on an external shear
    at all: psi is quadratic, and with the source at the barycentre of the two beta, d (phi_1 - phi_2) / d gamma =
    (theta_1 - theta_2) . (theta_1 + theta_2)-terms that cancel identically.  The Shear columns of the delay gradient are then
    exactly 0 in exact arithmetic (1e-10 in float64; asserted in the host test) while every image contributes addends of 1e4 - 1e5
    to them: a float32 sum cannot meet the absolute floor of ``PC.grad_gate`` (1e-6) on such a column (an MI355X left 2^-5 = 3e-7 of
    the addends), and nothing in the kernels is at fault.  The delays of ``many`` run inside the fused sums, where the position term
    gives those columns their scale and the accumulating delay kernel meets its families at thread indices >= 64; the delay term
    alone is taken beyond thread 64 by ``bf65`` and ``big``."""
    return tuple(t for t in held(shape, lens_set) if not (shape == "many" and t == "delays"))


# ---------------------------------------------------------------------------------------------------------------------
# thread counts
# ---------------------------------------------------------------------------------------------------------------------
def thread_counts(c):
    """``dict(p1 = B J, p2 = B F, p3 = B J L, p4 = B (P + 1))``: the threads of the four grids of ``run_positions``."""
    B, J, F = c["B"], sum(fm["x"].size for fm in c["fams"]), len(c["fams"])
    return dict(p1=B * J, p2=B * F, p3=B * J * c["lens_cols"], p4=B * (c["P"] + 1))


def edge_counts():
    """``{count name: sorted thread counts over the cases}``, with the stride (1, 1, L, P + 1) of every entry beside it."""
    out = {k: [] for k in ("p1", "p2", "p3", "p4")}
    for shape, s in CASES:
        c = case(shape, s)
        n = thread_counts(c)
        for k, stride in (("p1", 1), ("p2", 1), ("p3", c["lens_cols"]), ("p4", c["P"] + 1)):
            out[k].append((n[k], stride, f"{shape}-{s}"))
    return {k: sorted(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the data recipes of flux_cases / tdelay_cases, their patterns cycled for families of more than five images
# ---------------------------------------------------------------------------------------------------------------------
def with_fluxes(c, fams, rule=None):
    """``flux_cases.with_fluxes`` with ``PATTERN`` cycled: ``F_j = (3 + f) |mu_j of sample 0 in float64| PATTERN[j % 5]``,
    ``s_j = 0.05 F_j`` as float32; ``rule(f, j)``: False for an image without a measurement (NaN)."""
    _, lp = PC.leaf(c)
    out = []
    for k, fam in enumerate(fams):
        mu0 = 1.0 / FC.dets(c["phys"], c["mp"], lp, fam, c["B"])[:, 0].detach().abs().numpy()
        F = ((3 + k) * mu0 * np.resize(np.asarray(FC.PATTERN), mu0.size)).astype(np.float32)
        s = (np.float32(FC.REL_ERR) * F).astype(np.float32)
        if rule is not None:
            keep = np.asarray([bool(rule(k, j)) for j in range(F.size)])
            F, s = np.where(keep, F, np.float32(np.nan)), np.where(keep, s, np.float32(np.nan))
        out.append(dict(fam, flux=None if np.isnan(F).all() else F, flux_err=None if np.isnan(F).all() else s))
    return out


def with_delays(c, fams, rule=None, given=()):
    """``tdelay_cases.with_delays`` with ``PATTERN`` / ``ERRORS`` cycled; ``rule(f, j)``: False for an image without a measurement,
    None for a family without delays; ``given``: the families whose scale is given (``LAMBDA0 (1 + 0.05 f)``) instead of profiled."""
    p, lp = PC.leaf(c)
    rows = p.detach().numpy()
    out = []
    for k, fam in enumerate(fams):
        n = fam["x"].size
        keep = [True] * n if rule is None else [rule(k, j) for j in range(n)]
        if keep[0] is None:
            out.append(dict(fam, delay=None, delay_err=None, scale=np.nan))
            continue
        psi = TC.host_psi_model(c, rows, fam["x"], fam["y"]) if c.get("catalogue") is not None else None
        phi0 = TC.fermat(c, p, lp, fam, F64, psi)[:, 0].detach().numpy()
        t = (TC.LAMBDA0 * phi0 * np.resize(np.asarray(TC.PATTERN), n)).astype(np.float32)
        s = np.resize(np.asarray(TC.ERRORS, dtype=np.float32), n)
        t = np.where(keep, t, np.float32(np.nan))
        out.append(dict(fam, delay=t, delay_err=s, scale=float(np.float32(TC.LAMBDA0 * (1 + 0.05 * k))) if k in given else np.nan))
    return out


_MODES = {"bj63": ("full", "none", "one_nan"), "bj64": ("one_nan", "none", "full"), "bj65": ("one_nan", "full", "none"),
          "long": ("one_nan", "full"), "bf65": ("full", "none", "one_nan", "full", "one_nan")}


def modes(shape):
    """``"none"``, ``"one_nan"`` or ``"full"`` for every family of the shape -- the fluxes and the arrival times follow the same
    table.  A one-image family has none; the shapes of up to five families name theirs (``_MODES``), so that each holds the
    kinds its families allow; in the others every fourth family (f % 4 == 3) has none, every odd one of three or more images misses
    one image and the rest are fully measured."""
    sizes = SHAPES[shape][1]
    if shape in _MODES:
        assert all(m == "none" or n >= (3 if m == "one_nan" else 2) for m, n in zip(_MODES[shape], sizes))
        return _MODES[shape]
    return tuple("none" if (n == 1 or k % 4 == 3) else "one_nan" if (k % 2 == 1 and n >= 3) else "full" for k, n in enumerate(sizes))


def _missing(k, n):
    return k % n  # the unmeasured image of a family that misses one


def flux_rule(shape):
    m, sizes = modes(shape), SHAPES[shape][1]
    return lambda k, j: {"none": False, "full": True, "one_nan": j != _missing(k, sizes[k])}[m[k]]


def delay_rule(shape):
    m, sizes = modes(shape), SHAPES[shape][1]
    return lambda k, j: {"none": None, "full": True, "one_nan": j != _missing(k, sizes[k])}[m[k]]


def n_measured(shape):
    return tuple({"none": 0, "full": n, "one_nan": n - 1}[m] for m, n in zip(modes(shape), SHAPES[shape][1]))


def delay_given(shape):
    """The families with a given delay scale: every measured family that is odd or has fewer than three measured times (a profiled
    scale takes three or more); the others with measurements are profiled."""
    return tuple(k for k, n in enumerate(n_measured(shape)) if n and (k % 2 == 1 or n < 3))


# ---------------------------------------------------------------------------------------------------------------------
# lens sets
# ---------------------------------------------------------------------------------------------------------------------
def _rows(lp, B):
    """``B`` samples of the three rows of ``lp``: the first three as they are, sample b >= 3 is row b % 3 with every value moved
    by up to 2 % with a phase of its own (the recipe of ``tdelay_cases.case("b65")``)."""
    b = np.arange(B)
    move = lambda i: np.where(b < 3, 0.0, 0.02 * np.sin(0.9 * b + i))
    return [{k: (np.asarray(v, np.float64)[b % 3] * (1 + move(i))).astype(np.float32) for i, (k, v) in enumerate(d.items())} for d in lp]


_SERSIC = {"R_sersic": f(0.3, 0.35, 0.25), "n_sersic": f(2.0, 1.5, 2.5), "center_x": f(0.02, -0.03, 0.01), "center_y": f(-0.01, 0.02, 0.03),
           "Ie": f(10.0, 12.0, 8.0)}
_CATALOGUE = dict(lum=f(1.0, 0.6, 1.5), center_x=f(0.83, -0.67, 0.23), center_y=f(-0.57, 0.73, 1.03), e1=f(0.1, -0.05, 0.0),
                  e2=f(0.0, 0.1, -0.1))


def _zoo1():
    """dPIS + dPIEP + TNFW + NFW_ELLIPSE + a dPIE catalogue of 3 members: Einstein radii that add up to about 1.5; the rings at
    2.6 - 3.95 arcsec stay clear of r = Rs of either NFW halo (1.0 - 1.4 and 5.5 - 6.5), where its float32 evaluation cancels."""
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    from gigalens_amd.profiles.mass.nfw import NFW_ELLIPSE
    from gigalens_amd.profiles.mass.piemd import DPIS
    from gigalens_amd.profiles.mass.piep import DPIEP
    from gigalens_amd.profiles.mass.tnfw import TNFW
    P, O = MC.PIX, MC.OFF
    lenses = [DPIS(), DPIEP(), TNFW(), NFW_ELLIPSE(), DPIESubhalo(lum_star=1.0, galaxy_catalogue=_CATALOGUE)]
    lp = [dict(theta_E=f(0.55, 0.5, 0.6), r_core=f(0.1, 0.15, 0.08), r_cut=f(2.0, 1.5, 2.5), center_x=f(O, P + O, -P + O),
               center_y=f(-P + O, O, O)),
          dict(theta_E=f(0.4, 0.45, 0.35), Ra=f(0.08, 0.1, 0.05), Rs=f(1.5, 2.0, 1.2), center_x=f(2 * P + O, -P + O, O),
               center_y=f(-2 * P + O, O, P + O), e1=f(0.1, -0.1, 0.05), e2=f(0.0, 0.08, -0.1)),
          dict(Rs=f(1.2, 1.0, 1.4), alpha_Rs=f(0.3, 0.25, 0.35), r_trunc=f(6.0, 5.0, 7.0), center_x=f(-2 * P + O, P + O, 2 * P + O),
               center_y=f(P + O, -2 * P + O, O)),
          dict(Rs=f(6.0, 5.5, 6.5), alpha_Rs=f(0.5, 0.45, 0.6), e1=f(0.08, -0.1, 0.05), e2=f(-0.05, 0.05, 0.1),
               center_x=f(P + O, -2 * P + O, -P + O), center_y=f(2 * P + O, P + O, -2 * P + O)),
          dict(theta_E=f(0.1, 0.12, 0.08), r_core=f(0.05, 0.04, 0.06), r_cut=f(1.5, 2.0, 1.2))]
    return lenses, lp


# The rings of `long` are turned by 1.4 rad.  With three samples and two families a value yardstick is the largest of three to six
# float32 deviations, and as first drawn several landed far below the unit roundoff u = 2^-24 of the format (the position log_like
# within 0.2 - 0.3 u of float64, the flux chi2 at a fifth of what every other flux case shows): four times such a draw is no gate -- an
# MI355X, 1.4 u off on log_like and an ordinary 6.6e-7 off on the flux chi2 of twelve residuals, missed them by 1.7.  The figure moves
# with the CPU that computes it (0.2 u on one x86-64 host, 1.0 u on another, for the same turn), so turns of 0.0 to 1.5 rad in steps
# of 0.1 were scanned on two hosts for the one property that no value yardstick of any term or fused sum falls below 1 u on either:
# 0.2, 0.3, 0.6 and 1.4 have it; 1.4 has the largest smallest yardstick (1.67 u on both).  Nothing a kernel returned entered the choice.
_TURN = {"long": 1.4}


def _ring(k, n, turn=0.0):
    """Lattice indices ``(kx, ky)`` of the ``n`` images of family ``k``: a ring of radius 2.6 - 3.95 arcsec, its images spread over
    the circle with radii and angles of their own, snapped to the 0.1 arcsec lattice."""
    j = np.arange(n)
    r0 = 2.6 + 1.35 * ((0.618034 * (k + 1)) % 1.0)
    r = np.clip(r0 * (1 + 0.07 * np.sin(2.1 * j + k)), 2.6, 3.95)
    th = turn + 2.399963 * k + 2 * np.pi * j / n + 0.23 * np.sin(1.7 * j + 0.5 * k)
    return tuple(int(v) for v in np.rint(r * np.cos(th) / MC.PIX)), tuple(int(v) for v in np.rint(r * np.sin(th) / MC.PIX))


@functools.lru_cache(maxsize=None)
def case(shape, lens_set):
    """``dict(phys, phys_mp, mp, params, B, fams, sizes, pix, scales, catalogue, lens_cols, P)``: the keys of the cases of
    ``mp_positions_cases`` / ``flux_cases`` / ``tdelay_cases`` at once; every family carries ``flux`` / ``flux_err`` and, on ``plain``
    and ``zoo1``, ``delay`` / ``delay_err`` / ``scale`` (None / NaN where the shape or the set takes no measurement)."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    B, sizes = SHAPES[shape]
    catalogue, src, src_p = None, [], []
    if lens_set == "zoo1":
        lenses, lp = _zoo1()
        catalogue = _CATALOGUE
    else:
        m = MC.map_case("epl_shear|sie")
        lenses, lp = list(m["phys"].lenses), m["lens_params"]
        if lens_set in ("plain", "scaled"):
            src, src_p = [Sersic()], [_SERSIC]
    params = {"lens_mass": _rows(lp, B), "lens_light": [], "source_light": _rows(src_p, B)}
    phys = PhysicalModel(lenses, [], src)
    mp = MC._mp([0.5, 0.5, 1.0]) if lens_set == "planes" else MC._mp([0.5] * len(lenses))
    assert mp.K == (2 if lens_set == "planes" else 1)
    phys_mp = PhysicalModel(lenses, [], [], multiplane=mp) if lens_set == "planes" else None
    fams = []
    for k, n in enumerate(sizes):
        kx, ky = _ring(k, n, _TURN.get(shape, 0.0))
        fm = PC.family(mp, Z_FAMILIES[k % 2], kx, ky, 0.01 * (1 + 0.5 * (k % 3)))
        fams.append(dict(fm, T=np.ones(1)) if lens_set in ("plain", "zoo1") else fm)
    scales = [float(np.float32(fm["T"][0])) for fm in fams] if lens_set == "scaled" else None
    lens_cols = sum(len(l._native_params()) for l in lenses)
    P = lens_cols + sum(len(s.params) for s in src)
    c = dict(phys=phys, phys_mp=phys_mp, mp=mp, params=params, B=B, fams=fams, sizes=sizes, pix=MC.PIX, scales=scales, catalogue=catalogue,
             lens_cols=lens_cols, P=P)
    if "fluxes" in held(shape, lens_set):
        c["fams"] = with_fluxes(c, c["fams"], flux_rule(shape))
    else:
        c["fams"] = [dict(fm, flux=None, flux_err=None) for fm in c["fams"]]
    if "delays" in held(shape, lens_set):
        c["fams"] = with_delays(c, c["fams"], delay_rule(shape), delay_given(shape))
    return c


def centroids(c, fluxes=True, delays=True):
    """The keyword arguments of ``ForwardProbModel`` that carry the families of case ``c`` with the measurements asked for."""
    from gigalens_amd.simulator import LensSimulator
    fams = c["fams"]
    kw = dict(centroids_x=[fm["x"] for fm in fams], centroids_y=[fm["y"] for fm in fams], centroids_errors_x=[fm["ex"] for fm in fams],
              centroids_errors_y=[fm["ey"] for fm in fams])
    if c["phys_mp"] is not None:
        kw["centroids_redshifts"] = [fm["z"] for fm in fams]
    elif c["scales"] is not None:
        kw["centroids_scales"] = c["scales"]
    if fluxes and FC.n_flux(c):
        kw.update(centroids_fluxes=[fm["flux"] for fm in fams], centroids_fluxes_errors=[fm["flux_err"] for fm in fams])
    if delays and "delay" in fams[0] and TC.n_delay(c):
        dist = [None if np.isnan(fm["scale"]) else fm["scale"] / LensSimulator.DAYS_PER_MPC_ARCSEC2 for fm in fams]
        kw.update(centroids_time_delays=[fm["delay"] for fm in fams], centroids_time_delays_errors=[fm["delay_err"] for fm in fams],
                  time_delay_distances=dist)
    return kw


# ---------------------------------------------------------------------------------------------------------------------
# the reference: one family at a time through the restatements of the three modules
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().double().numpy()


def evaluate(c, term, dtype=F64):
    """``dict(log_like [B], chi2 [B], fam [B, F, 2], grad [B, P] or None, ...)`` of one term of case ``c`` as float64 numpy arrays
    holding ``dtype`` arithmetic: every family through ``stats`` of its module with ``fams=[fam]``, summed in family order; the
    gradient by ``torch.autograd`` on that sum.  ``fluxes``: + ``S`` [B, F] and ``model`` [B, J]; ``delays``: + ``scale``, ``offset``
    [B, F] and ``model`` [B, J] -- in float64 through the line integral of the deflection (a catalogue: the host psi and central
    differences, ``TC.loglike_grad``), in float32 with psi of the float32 host build and no gradient (``TC.yardstick_values``)."""
    p, lp = PC.leaf(c, dtype)
    B = c["B"]
    host = term == "delays" and (dtype == F32 or c["catalogue"] is not None)
    per, extra = [], []
    for fam in c["fams"]:
        if term == "positions":
            ll, red, _ = PC.stats(c["phys"], c["mp"], lp, [fam], B, dtype)
            chi2 = red * (2.0 * fam["x"].size)
        elif term == "fluxes":
            ll, chi2, S, model, _ = FC.stats(c["phys"], c["mp"], lp, [fam], B, dtype)
            extra.append((S, model))
        else:
            ll, chi2, lam, T, model = TC.stats(c, p, lp, dtype, host=host, fams=[fam])
            extra.append((lam, T, model))
        per.append((ll, chi2))
    ll, chi2 = sum(v[0] for v in per), sum(v[1] for v in per)
    if host:
        g = TC.loglike_grad(c)[2] if dtype == F64 else None
    else:
        g = _np(torch.autograd.grad(ll.sum(), p)[0]) if ll.requires_grad else np.zeros(tuple(p.shape))
    out = dict(log_like=_np(ll), chi2=_np(chi2), grad=g,
               fam=np.stack([np.stack([_np(a), _np(b)], axis=-1) for a, b in per], axis=1))
    if term == "fluxes":
        out.update(S=_np(torch.cat([e[0] for e in extra], dim=1)), model=_np(torch.cat([e[1] for e in extra], dim=1)))
    elif term == "delays":
        out.update(scale=_np(torch.cat([e[0] for e in extra], dim=1)), offset=_np(torch.cat([e[1] for e in extra], dim=1)),
                   model=_np(torch.cat([e[2] for e in extra], dim=1)))
    return out


def nan_err(got, ref):
    """``MC.rel_err`` over the finite entries of ``ref``; the NaN patterns must agree."""
    return TC.nan_err(got, ref)


VALUE_KEYS = {"positions": ("log_like", "chi2", "fam_ll", "fam_chi2"), "fluxes": ("log_like", "chi2", "fam_ll", "fam_chi2", "S", "model"),
              "delays": ("log_like", "chi2", "fam_ll", "fam_chi2", "scale", "offset", "model")}


def deviations(got, ref, term):
    """The deviation of ``got`` from ``ref`` (dicts of ``evaluate``) for every value key of ``term``, relative to the largest value of
    the reference array (``MC.rel_err``; NaN patterns must agree): the figure the gates of the per-term GPU tests are written in."""
    out = dict(log_like=MC.rel_err(got["log_like"], ref["log_like"]), chi2=_rel0(got["chi2"], ref["chi2"]),
               fam_ll=MC.rel_err(got["fam"][..., 0], ref["fam"][..., 0]), fam_chi2=_rel0(got["fam"][..., 1], ref["fam"][..., 1]))
    for k in VALUE_KEYS[term][4:]:
        out[k] = nan_err(got[k], ref[k])
    return out


def _rel0(got, ref):
    """``MC.rel_err``; a reference that is exactly 0 everywhere (one-image families: chi2 = 0) must be met exactly."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.abs(ref).max():
        return float(np.abs(got).max())
    return MC.rel_err(got, ref)


@functools.lru_cache(maxsize=None)
def _both(shape, lens_set, term):
    c = case(shape, lens_set)
    return evaluate(c, term, F64), evaluate(c, term, F32)


@functools.lru_cache(maxsize=None)
def data(shape, lens_set, term):
    """``(case, ref, yard)`` -- computed once and shared (left unchanged).  ``ref``: ``evaluate`` in float64; ``yard``: the deviations
    of the float32 restatement from it (``deviations``) and ``grad`` in units of the gate (``PC.grad_gate``; None for the delays,
    whose float32 restatement carries no gradient)."""
    c = case(shape, lens_set)
    ref, r32 = _both(shape, lens_set, term)
    yard = deviations(r32, ref, term)
    yard["grad"] = None if r32["grad"] is None else PC.grad_gate(r32["grad"][:, :c["lens_cols"]], ref["grad"][:, :c["lens_cols"]])
    return c, ref, yard


# ---------------------------------------------------------------------------------------------------------------------
# the fused sums: prior + positions (+ fluxes) (+ delays) of the fused log-prob path
# ---------------------------------------------------------------------------------------------------------------------
COMBOS = (("positions", "fluxes"), ("positions", "delays"), ("positions", "fluxes", "delays"))
PRIOR_REL = 0.3


def combos_of(shape, lens_set):
    return tuple(cb for cb in COMBOS if set(cb) <= set(held(shape, lens_set)))


def packed_rows(c):
    """``[B, P]`` float64 array of the float32 packed rows of case ``c`` (the library's column order)."""
    from tests import multilens_grad_cases as GC
    return GC.pack_np(c["phys"], c["params"]).numpy()


def prior_normal(v0):
    """``(loc, scale)`` of the prior of a column whose first sample is ``v0``: a Normal, hence an Identity bijector -- the rows the
    fused path hands its kernels are the float32 rows of the case bit for bit, and the float64 sum of the restated terms at those
    rows is its reference; the gradient comes back in z-space = x-space, carried there by the float64 Identity / Normal column of
    tests/zspace_cases.py.  (The Exp and Sigmoid front end has its own matrix in tests/test_gpu_zspace.py.)"""
    v0 = float(v0)
    return v0, PRIOR_REL * max(abs(v0), 0.3)


@functools.lru_cache(maxsize=None)
def fused(shape, lens_set, combo):
    """``(case, ref, yard)`` of the fused log-prob of ``combo`` under the prior of ``prior_normal`` -- ``ref``: ``log_prob``,
    ``red_chi2`` [B], ``fam`` [B, F, 2] and ``grad`` [B, P] with respect to the packed columns (= the z columns, in the packed order)
    as the FLOAT64 prior (``zspace_cases.evaluate / log_prior / grad_z``) plus the float64 sum of the restated terms; ``yard``: the
    deviation of the same sum of the float32 restatements (``grad`` None with the delays, which have no float32 gradient)."""
    from tests import zspace_cases as Z
    c = case(shape, lens_set)
    rows = packed_rows(c)
    specs = [Z.Spec(Z.ID, Z.NORMAL, *prior_normal(v0)) for v0 in rows[0]]
    n = 2.0 * sum(c["sizes"]) + (FC.n_flux(c) if "fluxes" in combo else 0) + (TC.n_delay(c) if "delays" in combo else 0)
    out = []
    for dt, slot in ((np.float64, 0), (np.float32, 1)):
        parts = [_both(shape, lens_set, t)[slot] for t in combo]
        ev = Z.evaluate(specs, rows.astype(np.float32), dt)
        lprior = Z.log_prior(ev)[0].astype(np.float64)
        G = None if any(p["grad"] is None for p in parts) else sum(p["grad"] for p in parts)
        out.append(dict(log_prob=lprior + sum(p["log_like"] for p in parts), red_chi2=sum(p["chi2"] for p in parts) / n,
                        fam=sum(p["fam"] for p in parts),
                        grad=None if G is None else Z.grad_z(ev, G, range(rows.shape[1]))[0].astype(np.float64)))
    ref, r32 = out
    yard = dict(log_prob=MC.rel_err(r32["log_prob"], ref["log_prob"]), red_chi2=_rel0(r32["red_chi2"], ref["red_chi2"]),
                fam_ll=MC.rel_err(r32["fam"][..., 0], ref["fam"][..., 0]), fam_chi2=_rel0(r32["fam"][..., 1], ref["fam"][..., 1]),
                grad=None if r32["grad"] is None else PC.grad_gate(r32["grad"], ref["grad"]))
    return c, ref, yard


def det_signs(c):
    """``det A [J, B]`` of every image of case ``c`` in float64."""
    _, lp = PC.leaf(c)
    with torch.enable_grad():
        return np.concatenate([_np(FC.dets(c["phys"], c["mp"], lp, fam, c["B"])) for fam in c["fams"]], axis=0)


def min_centre(c):
    """``tdelay_cases.min_centre``: the smallest distance of a segment of the line integral's paths to a profile centre."""
    return TC.min_centre(c)
