"""Float64 restatement of the time-delay likelihood on lens planes (csrc/gl_multiplane_tdelays.hip.h) and the cases of its tests:
tests/test_mp_tdelay_like_host.py pins the restatement without a GPU, tests/test_gpu_mp_tdelay_like.py runs the kernels against it.

The restatement is composed of pieces other tests pin:

* ``beta_j`` of every observed image of a family, and the ray's position ``theta_j,i`` on every plane in front of it, from
  ``mp_positions_cases.trace`` (the float32 couplings the library holds, float64 arithmetic); the source is ``mean beta``;
* ``phi_j = T(theta_j; mean beta)`` from ``mp_tdelay_cases.reference_T`` with ``sx, sy = mean beta`` (``composed_T`` below writes the
  same sum on the same parts -- the rays above and ``potential_cases.host_psi`` -- with float64 parameter rows, which ``reference_T``
  rounds to float32: the central differences of the gradient need them; tests/test_mp_tdelay_like_host.py asserts that the two agree
  at the rows of every case);
* the statistic from ``tdelay_cases.family_term``: ``lambda_f`` given (days per arcsec^2 c / H0) or profiled, ``chi2``, ``log_like``,
  ``T_f`` and the model delays.

The gradient reference: central differences in float64 over the packed lens columns, step ``1e-5 max(1, max |column|)`` (the rule of
``tdelay_cases.loglike_grad``'s catalogue branch); the host test asserts that ``h`` and ``h / 2`` agree to 1e-3 of the gradient gate.
(The TNFW's psi there: ``SMOOTH_KINDS``.  Two columns of ``zoo_b`` whose gradient vanishes by cancellation: ``CANCELLED``.)

The value yardstick (CPU): the same restatement with ``mp_tdelay_cases.host_T`` -- tests/hostmath/multiplane_fermat_host.cpp, the
kernel's own double arithmetic compiled with g++ -- in the place of ``reference_T``.  ``host_T`` takes the source as float32; the
last geometric summand is the only one that sees it, so the value at ``mean beta`` itself is ``host_T`` at the rounded source plus
``g_last (s - mean beta) . (theta_last - (s + mean beta) / 2)``, exactly.  ``YARD_CEILING``: twice the largest figure per quantity
measured when the cases were fixed; every case stays below ``2^-24`` of the quantity's scale (asserted in the host test).

Deterministic data, as ``tdelay_cases``: ``t_j = LAMBDA0 T_j(sample 0, float64) PATTERN[j]`` in days as float32, ``s_j = ERRORS[j]``."""
import functools

import numpy as np
import torch

from tests import helpers
from tests import multilens_cases as MC
from tests import multilens_grad_cases as GC
from tests import mp_positions_cases as PC
from tests import mp_tdelay_cases as MT
from tests import potential_cases as POT
from tests import tdelay_cases as TC

F64 = MC.F64
H0_TRUE = 70.0
PATTERN, ERRORS = TC.PATTERN, TC.ERRORS
EPS32 = 2.0 ** -24
QUANTITIES = ("log_like", "chi2", "scale", "offset", "model")
# twice the largest |host - composed| / scale over the cases, measured on the CPU (x86-64, g++ -O2, torch CPU float64) when the cases
# were fixed: log_like 2.1e-14, chi2 2.2e-14, lambda 2.9e-14, T 1.9e-14 and the model delays 4.0e-15 (all k2_b65; k3: 1.9e-14 in
# log_like and chi2) -- double rounding times the cancellation of phi~, six orders below the float32 rounding of the results; and
# no less than mp_tdelay_cases.ROUNDING_FLOOR, whose reasons hold here
YARD_CEILING = {k: max(2 * v, MT.ROUNDING_FLOOR) for k, v in
                dict(log_like=2.1e-14, chi2=2.2e-14, scale=2.9e-14, offset=1.9e-14, model=4.0e-15).items()}


def lambda_of(h0):
    """``c / H0`` in days per arcsec^2: the scale of a family with a given H0 (km/s/Mpc); NaN stays NaN (profiled)."""
    from gigalens_amd.cosmology import C_KM_S
    from gigalens_amd.simulator import LensSimulator
    return C_KM_S / h0 * LensSimulator.DAYS_PER_MPC_ARCSEC2


LAMBDA0 = lambda_of(H0_TRUE)


def h0_of(lam):
    """H0 in km/s/Mpc of a scale ``lambda_f`` in days per arcsec^2 c / H0 (the inverse of ``lambda_of``)."""
    return lambda_of(1.0) / lam


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def family_weights(c):
    """``(geom [F, K], pot [K])`` float64: ``MultiPlane.delay_weights`` of every family; ``pot`` from the farthest family with delays."""
    w = [c["mp"].delay_weights(fm["z"]) for fm in c["fams"]]
    has = [fm.get("delay") is not None and bool(np.any(~np.isnan(fm["delay"]))) for fm in c["fams"]]
    z = [fm["z"] if h else -np.inf for fm, h in zip(c["fams"], has)]
    far = int(np.argmax(z)) if any(has) else int(np.argmax([fm["z"] for fm in c["fams"]]))
    return np.stack([g for g, _ in w], axis=0), w[far][1]


def rays(c, rows, fam):
    """``(beta_x, beta_y [J_f, B], [(plane, theta_x, theta_y [J_f, B])])`` float64 numpy of the images of ``fam`` at the packed rows
    ``rows`` ``[B, P]`` (float64): ``mp_positions_cases.trace``."""
    p = torch.as_tensor(np.asarray(rows, dtype=np.float64))
    lp = helpers.struct_from_packed(c["phys"], p)["lens_mass"]
    B = p.shape[0]
    cx, cy = PC._points(fam["x"], F64, B), PC._points(fam["y"], F64, B)
    with torch.enable_grad():
        bx, by, _, r = PC.trace(c["phys"], c["mp"], lp, cx, cy, fam["T"])
    return bx.detach().numpy(), by.detach().numpy(), [(j, x.detach().numpy(), y.detach().numpy()) for j, x, y in r]


def _lens_columns(phys):
    n = [len(lens._native_params()) for lens in phys.lenses]
    return np.concatenate([[0], np.cumsum(n)]).astype(int)


# The TNFW's potential template is a quadrature whose value jumps by 1e-11 of psi as its arguments move (measured: the central
# differences of every column that moves a ray on a TNFW's plane, or its Rs, scatter by up to 6.5e-2 of the gate between h and h / 2,
# every other column by 1e-5).  For the GRADIENT reference the psi of these kinds is therefore the line integral of the oracle's
# deflection from the fixed anchor of ``tdelay_cases.path`` (composite Gauss-Legendre on fixed nodes: smooth in the end point and in
# the parameters; equal to the host potential differences to 1e-9, tests/test_tdelays_host.py) plus the host psi at the anchor, which
# is common to the images of a family and drops out of everything but T_f.  The values keep ``host_psi``.
SMOOTH_KINDS = ("TNFW",)


def line_integral_psi(c, l, row, x, y):
    """``psi(anchor) + int alpha . dl`` ``[n]`` of lens l with the float64 parameter row ``row`` at the points ``x, y`` ``[n]``."""
    from oracle import ref_torch as ref
    lens = c["phys"].lenses[l]
    names = [n for n in lens._native_params() if n in lens.params]
    lp = {n: torch.as_tensor(float(v), dtype=F64) for n, v in zip(names, row)}
    consts = MC._consts(c["phys"], F64)[l]
    px, py, Wx, Wy = TC._nodes(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    with torch.no_grad():
        fx, fy = ref.mass_deriv(lens, torch.as_tensor(px), torch.as_tensor(py), **lp, **consts)
    kind, iparam, _ = lens._component()
    anchor = POT.host_psi(kind, row, [TC.R_ANCHOR], [0.0], iparam=iparam)[0]
    return anchor + Wx @ fx.numpy() + Wy @ fy.numpy()


def smooth_min_centre(c):
    """The smallest distance of a path of ``line_integral_psi`` to the centre of its lens, over the rays of case ``c``."""
    rows = GC.pack_np(c["phys"], c["params"]).numpy()
    off, best = _lens_columns(c["phys"]), np.inf
    for fam in c["fams"]:
        for plane, tx, ty in rays(c, rows, fam)[2]:
            for l, lens in enumerate(c["phys"].lenses):
                if int(c["mp"].plane_of_lens[l]) != plane or type(lens).__name__ not in SMOOTH_KINDS:
                    continue
                names = [n for n in lens._native_params()]
                for b in range(rows.shape[0]):
                    cx, cy = rows[b, off[l] + names.index("center_x")], rows[b, off[l] + names.index("center_y")]
                    for x, y in zip(tx[:, b], ty[:, b]):
                        for xa, ya, xb, yb, _ in TC.path(x, y):
                            d, L2 = np.array([xb - xa, yb - ya]), (xb - xa) ** 2 + (yb - ya) ** 2
                            t = np.clip(((cx - xa) * d[0] + (cy - ya) * d[1]) / L2, 0.0, 1.0)
                            best = min(best, float(np.hypot(xa + t * d[0] - cx, ya + t * d[1] - cy)))
    return best


def composed_T(c, rows, fam, geom, pot, bx, by, r, smooth=False):
    """``T(theta_j; mean beta)`` ``[J_f, B]``: the sum of ``mp_tdelay_cases.reference_T`` on the rays ``r`` and
    ``potential_cases.host_psi`` at the float64 rows.  ``smooth``: the ``SMOOTH_KINDS`` through ``line_integral_psi``."""
    rows = np.asarray(rows, dtype=np.float64)
    B, off = rows.shape[0], _lens_columns(c["phys"])
    ks = int(np.count_nonzero(geom))
    assert ks == len(r) and np.all(geom[:ks] > 0) and np.all(geom[ks:] == 0)
    mbx, mby = bx.mean(axis=0, keepdims=True), by.mean(axis=0, keepdims=True)
    T = np.zeros_like(bx)
    for i, (plane, tx, ty) in enumerate(r):
        assert plane == i
        nx, ny = (r[i + 1][1], r[i + 1][2]) if i + 1 < ks else (mbx, mby)
        psi = np.zeros_like(tx)
        for l, lens in enumerate(c["phys"].lenses):
            if int(c["mp"].plane_of_lens[l]) == i:
                kind, iparam, _ = lens._component()
                for b in range(B):
                    if smooth and type(lens).__name__ in SMOOTH_KINDS:
                        psi[:, b] += line_integral_psi(c, l, rows[b, off[l]:off[l + 1]], tx[:, b], ty[:, b])
                    else:
                        psi[:, b] += POT.host_psi(kind, rows[b, off[l]:off[l + 1]], tx[:, b], ty[:, b], iparam=iparam)
        T += geom[i] * 0.5 * ((tx - nx) ** 2 + (ty - ny) ** 2) - pot[i] * psi
    return T


def _lens_dicts(c, rows):
    """The lens parameter dicts ``mp_tdelay_cases`` takes, from packed rows that hold float32 values."""
    lp = helpers.struct_from_packed(c["phys"], torch.as_tensor(np.asarray(rows, dtype=np.float64)))["lens_mass"]
    return [{k: v.numpy().astype(np.float32) for k, v in d.items()} for d in lp]


def reference_T(c, rows, fam, geom, pot, bx, by, r, host=False):
    """``T(theta_j; mean beta)`` ``[J_f, B]`` from ``mp_tdelay_cases.reference_T`` (``host``: ``host_T``, completed for the float32
    rounding of its source -- module docstring) at rows that hold float32 values."""
    B = np.shape(rows)[0]
    x = np.ascontiguousarray(np.broadcast_to(np.asarray(fam["x"], np.float32)[None, None, :], (B, 1, fam["x"].size)))
    y = np.ascontiguousarray(np.broadcast_to(np.asarray(fam["y"], np.float32)[None, None, :], (B, 1, fam["y"].size)))
    mbx, mby = bx.mean(axis=0), by.mean(axis=0)  # [B]
    lp = _lens_dicts(c, rows)
    if not host:
        return MT.reference_T(c["phys"], c["mp"], lp, x, y, mbx[:, None], mby[:, None], geom[None, :], pot)[0][:, 0].T
    sx, sy = mbx.astype(np.float32), mby.astype(np.float32)
    T = MT.host_T(c["phys"], c["mp"], lp, x, y, sx[:, None], sy[:, None], geom[None, :], pot)[0][:, 0].T  # [J_f, B]
    glast, (_, lx, ly) = geom[np.count_nonzero(geom) - 1], r[-1]
    dx, dy = sx.astype(np.float64) - mbx, sy.astype(np.float64) - mby
    return T + glast * (dx[None, :] * (lx - 0.5 * (sx + mbx)[None, :]) + dy[None, :] * (ly - 0.5 * (sy + mby)[None, :]))


def values(c, rows=None, how="composed", fams=None, smooth=False, source_rows=None):
    """``(log_like [B], chi2 [B], lambda [B, F], T_f [B, F], model delay [B, J])`` float64 numpy over the families of case ``c`` at the
    packed rows (default: the case's).  ``how``: ``composed`` (float64 rows), ``reference`` (``mp_tdelay_cases.reference_T``) or
    ``host`` (``host_T``: the yardstick).  ``smooth``: ``composed_T``'s.  ``source_rows``: mean beta is that of these rows, held fixed
    (the direct part of the gradient)."""
    rows = GC.pack_np(c["phys"], c["params"]).numpy() if rows is None else np.asarray(rows, dtype=np.float64)
    geom, pot = family_weights(c)
    ll = chi2 = 0.0
    lams, offs, models = [], [], []
    for f, fam in enumerate(c["fams"] if fams is None else fams):
        bx, by, r = rays(c, rows, fam)
        if source_rows is not None:
            bx, by, _ = rays(c, source_rows, fam)
        if how == "composed":
            T = composed_T(c, rows, fam, geom[f], pot, bx, by, r, smooth)
        else:
            T = reference_T(c, rows, fam, geom[f], pot, bx, by, r, host=how == "host")
        lam = np.nan if np.isnan(fam.get("h0", np.nan)) else lambda_of(fam["h0"])
        ll_f, chi2_f, lam_f, T_f, model = TC.family_term(torch.as_tensor(T), fam.get("delay"), fam.get("delay_err"), lam)
        ll, chi2 = ll + ll_f.numpy(), chi2 + chi2_f.numpy()
        lams.append(lam_f.numpy())
        offs.append(T_f.numpy())
        models.append(model.numpy())
    return ll, chi2, np.stack(lams, axis=1), np.stack(offs, axis=1), np.concatenate(models, axis=0).T


def gradient(c, halve=1.0, fams=None, cols=None, direct=False):
    """``d log_like / d packed`` ``[B, P]``: central differences of ``values`` (composed) over the lens columns (``cols``: these
    alone, the others 0), every sample at once; step ``1e-5 max(1, max |column|) / halve``.  ``direct``: at fixed mean beta -- the part
    the grad kernel adds; the rest passes through the beta adjoints of the position likelihood."""
    base = GC.pack_np(c["phys"], c["params"]).numpy()
    g = np.zeros_like(base)
    for k in (range(base.shape[1]) if cols is None else cols):
        h = 1e-5 * max(1.0, float(np.abs(base[:, k]).max())) / halve
        out = []
        for sgn in (1.0, -1.0):
            q = base.copy()
            q[:, k] += sgn * h
            out.append(values(c, q, fams=fams, smooth=True, source_rows=base if direct else None)[0])
        g[:, k] = (out[0] - out[1]) / (2 * h)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
BASE = ("k2", "k3", "k4", "front", "zoo_a", "zoo_b")
VARIANTS = ("k2_given", "k2_nan", "k2_two", "k2_one", "k2_mixed", "k2_b65")
CASES = BASE + VARIANTS
# ``zoo_b`` carries the kinds ``zoo_a`` does not (TNFW, NFW_ELLIPSE, dPIEP, SIE behind the first plane).  In the two columns of its
# Shear, on the last plane, the direct part of the gradient and the part through the source are +-2.7e4 and cancel to 3e-4 (asserted
# in the host test: the sum is below 1e-6 of the direct part, element by element).  The kernels form the second part in float32 (P3 of the position
# likelihood), so what is left there is rounding of numbers the size of the row's other elements, and a gate whose scale is the
# column's own 1e-4 cannot hold; nor can the central differences reach 1e-3 of it (|log_like| is 1e4, their rounding 1e-6).  These
# columns, by name, take the project's gate with the scale of their row: ``5e-4 max_k |g64[b, k]| + 1e-6`` -- the scale
# tests/test_gpu_positions.py uses for every element.  Every other column of every case takes ``mp_positions_cases.grad_gate``.
CANCELLED = {"zoo_b": "Shear"}


def cancelled_columns(name, c):
    """``[P]`` bool: the columns of case ``name`` whose gradient vanishes by cancellation (``CANCELLED``), gated at the row's scale."""
    out = np.zeros(int(_lens_columns(c["phys"])[-1]), dtype=bool)
    off = _lens_columns(c["phys"])
    for l, lens in enumerate(c["phys"].lenses):
        if type(lens).__name__ == CANCELLED.get(name):
            out[off[l]:off[l + 1]] = True
    return out


def gate_units(name, c, g, g64):
    """``(worst element of the gated columns in units of grad_gate's gate, worst element of the cancelled columns in units of the
    gate at the row's scale)`` -- the scales are those of the whole matrix ``g64``; 0.0 where a case has no cancelled column."""
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    row = np.abs(g64).max(axis=1, keepdims=True)
    scale = np.minimum(np.abs(g64).max(axis=0, keepdims=True), row)
    ex = cancelled_columns(name, c)
    u = np.abs(g - g64) / (PC.GRAD_RTOL * scale + PC.GRAD_ATOL)
    u_row = np.abs(g - g64) / (PC.GRAD_RTOL * row + PC.GRAD_ATOL)
    return float(u[:, ~ex].max()), float(u_row[:, ex].max()) if ex.any() else 0.0


def with_delays(c, rule=None, h0=None):
    """The families of ``c`` with the deterministic arrival times of this module.  ``rule(f, j)``: False for an image without a
    measurement, None for a family without delays; ``h0(f, n)``: the family's given H0 or NaN (default: profiled with three or more
    measured times, ``H0_TRUE`` with two)."""
    rows = GC.pack_np(c["phys"], c["params"]).numpy()
    first = dict(c, fams=[dict(fm, delay=np.zeros(fm["x"].size, np.float32)) for fm in c["fams"]])  # (the weights of every family)
    geom, pot = family_weights(first)
    out = []
    for f, fam in enumerate(c["fams"]):
        keep = [True] * fam["x"].size if rule is None else [rule(f, j) for j in range(fam["x"].size)]
        if keep[0] is None:
            out.append(dict(fam, delay=None, delay_err=None, h0=np.nan))
            continue
        bx, by, r = rays(c, rows, fam)
        T0 = composed_T(c, rows, fam, geom[f], pot, bx, by, r)[:, 0]
        t = (LAMBDA0 * T0 * np.asarray(PATTERN[:T0.size])).astype(np.float32)
        t = np.where(keep, t, np.float32(np.nan))
        n = int(np.count_nonzero(keep))
        out.append(dict(fam, delay=t, delay_err=np.asarray(ERRORS[:T0.size], dtype=np.float32),
                        h0=(np.nan if n >= 3 else H0_TRUE) if h0 is None else h0(f, n)))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """``dict(phys, phys_mp, mp, params, B, fams, lens_cols)`` on the lens sets, families and redshifts of ``mp_positions_cases``; every
    family has ``delay`` / ``delay_err`` / ``h0`` (NaN: profiled).  ``k2`` / ``k3`` / ``k4`` / ``front`` (every family in front of the last
    plane) / ``zoo_a`` and ``zoo_b`` (between them every kind with a potential on a plane behind the first: EPL, Shear, NFW, dPIS, dPIE, SIS
    and TNFW, NFW_ELLIPSE, dPIEP, SIE): every family with delays, H0 profiled where the family has
    three images or more and given (70) where it has two.  Variants of ``k2``: ``k2_given`` a given H0; ``k2_nan`` one unmeasured image;
    ``k2_two`` the second family without delays and ``k2_one`` the first family alone; ``k2_mixed`` one profiled and one given (67);
    ``k2_b65`` 65 samples (the three rows in turn, moved by up to 0.2 %), across the 64-thread block edge of the family kernel."""
    assert name in CASES, name
    base = name.split("_")[0] if name in VARIANTS else name
    c = dict(PC.case(base))
    rule = h0 = None
    if name == "k2_given":
        h0 = lambda f, n: H0_TRUE * (1 + 0.05 * f)
    elif name == "k2_nan":
        rule = lambda f, j: not (f == 1 and j == 2)
    elif name == "k2_two":
        rule = lambda f, j: True if f == 0 else None
    elif name == "k2_one":
        c["fams"] = c["fams"][:1]
    elif name == "k2_mixed":
        h0 = lambda f, n: np.nan if f == 0 else 67.0
    elif name == "k2_b65":
        # the three rows in turn, each value moved by up to 0.2 % with a phase of its own (tdelay_cases b65 moves them by 2 %: here
        # some of 65 rows then land close to a best fit, where the gradient is small against the h^2 term of the central
        # differences at the fixed step, and h and h / 2 no longer agree to 1e-3 of the gate; measured 4.0e-3, with 0.2 % 9.8e-4)
        b = np.arange(65)
        lp = [{k: (np.asarray(v, np.float64)[b % 3] * (1 + 0.002 * np.sin(0.9 * b + i))).astype(np.float32)
               for i, (k, v) in enumerate(d.items())} for d in c["params"]["lens_mass"]]
        c["params"], c["B"] = dict(c["params"], lens_mass=lp), 65
    c["lens_cols"] = int(_lens_columns(c["phys"])[-1])
    return dict(c, fams=with_delays(c, rule, h0))


def centroids(c):
    """The keyword arguments of ``ForwardProbModel`` that carry the families of case ``c`` with their delays and H0."""
    return dict(PC.centroids(c), centroids_time_delays=[fm["delay"] for fm in c["fams"]],
                centroids_time_delays_errors=[fm["delay_err"] for fm in c["fams"]],
                time_delay_h0=[None if np.isnan(fm["h0"]) else fm["h0"] for fm in c["fams"]])


def behind_columns(c):
    """``[P]`` bool: the packed columns of lenses on a plane at or behind every family with delays -- no ray of the term meets them."""
    reach = max(int(np.count_nonzero(fm["T"])) for fm in c["fams"] if fm["delay"] is not None and np.any(~np.isnan(fm["delay"])))
    off = _lens_columns(c["phys"])
    out = np.zeros(off[-1], dtype=bool)
    for l in range(len(c["phys"].lenses)):
        out[off[l]:off[l + 1]] = int(c["mp"].plane_of_lens[l]) >= reach
    return out


def n_delay(c):
    return int(sum(0 if fm["delay"] is None else np.count_nonzero(~np.isnan(fm["delay"])) for fm in c["fams"]))


def errors(got, ref):
    """``{quantity: max |got - ref| / max |ref|}`` of two ``values`` tuples (``tdelay_cases.nan_err``: the NaN patterns must agree)."""
    return {k: TC.nan_err(g, r) for k, g, r in zip(QUANTITIES, got, ref)}


@functools.lru_cache(maxsize=None)
def data(name):
    """``(case, ref, yard)`` -- computed once and shared (left unchanged).  ``ref``: the ``QUANTITIES`` in float64 (composed);
    ``yard``: the deviation of the host build from them, relative to their largest value."""
    c = case(name)
    ref = values(c)
    return c, dict(zip(QUANTITIES, ref)), errors(values(c, how="host"), ref)


@functools.lru_cache(maxsize=None)
def grad(name):
    """The float64 gradient reference of case ``name`` (central differences), computed once and shared."""
    return gradient(case(name))


def value_gate(yard):
    """The gate of a GPU value against float64: 4 x the case's CPU yardstick, and no less than 8 x 2^-24 of the quantity's scale (the
    results are float32 roundings of double arithmetic)."""
    return max(4 * yard, 8 * EPS32)
