"""Float64 restatement of the unconstrained-space front end and back end (gl_prep_kernel / gl_prep_wave_kernel of
csrc/gl_frontend.hip.h, gl_finalize_kernel of csrc/gl_finalize.hip.h) and the case matrix of their tests
(tests/test_zspace_host.py pins the restatement without a GPU, tests/test_gpu_zspace.py runs the kernels against it).

Everything is numpy, written from the definitions and independent of gigalens_amd/prior.py: the bijectors Identity / Exp /
Sigmoid(lo, hi) with value, dx/dz, log|dx/dz| and its derivative in forms that do not cancel, the log-densities Normal / LogNormal /
Uniform / TruncatedNormal with d log p / dx (the truncation normaliser from ``math.erf``), and the EPL coefficient table from its
definition.  Every function takes ``dt``: ``numpy.float64`` is the reference; the same formulas in ``numpy.float32`` are the
yardstick of the gates (``gate``): four times the worst deviation of the float32 restatement from float64 over the case, never
below a floor derived from the number format.  No gate is taken from what the kernels return."""
import math
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

ID, EXP, SIG = 0, 1, 2
NORMAL, LOGNORMAL, UNIFORM, TRUNC = 0, 1, 2, 3
BIJECTORS = ("Identity", "Exp", "Sigmoid")
PRIORS = ("Normal", "LogNormal", "Uniform", "TruncatedNormal")
F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of float32
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
EPL_TOL32 = 1e-9  # the series tolerance of the float32 kernels (gl_profiles.h epl_series_tol)
EPL_K, EPL_KI, EPL_TAB = 8, 10, 12  # slots of an EPL derived block (gl_profiles.h)


def f32(v):
    return float(np.float32(v))


@dataclass(frozen=True)
class Spec:
    """One column of z: bijector, prior and its constants (taken as the float32 values the library receives); ``zr``: the range of
    prior-typical z; ``edge``: z values the first rows of a case visit instead (Identity / Exp columns)."""
    bij: int
    prior: int
    a: float = 0.0
    b: float = 1.0
    lo: float = 0.0
    hi: float = 1.0
    zr: Tuple[float, float] = (-1.0, 1.0)
    edge: Tuple[float, ...] = ()

    def __post_init__(self):
        for n in ("a", "b", "lo", "hi"):
            object.__setattr__(self, n, f32(getattr(self, n)))

    @property
    def pair(self):
        return (BIJECTORS[self.bij], PRIORS[self.prior])


def log_norm(s):
    """log(Phi(beta) - Phi(alpha)) of a TruncatedNormal, float64 (0 for the other priors)."""
    if s.prior != TRUNC:
        return 0.0
    al, be = (s.lo - s.a) / s.b, (s.hi - s.a) / s.b
    return math.log(0.5 * (math.erf(be / math.sqrt(2)) - math.erf(al / math.sqrt(2))))


# ---------------------------------------------------------------------------------------------------------------------
# bijectors and priors of one column
# ---------------------------------------------------------------------------------------------------------------------
def eval_column(s, z, dt=F64):
    """``z`` [B] (float32 values) -> dict of [B] arrays in ``dt``: ``x``, ``xs`` (the scale of x: the sum of the |addends| that form
    it), ``dxdz``, ``fldj``, ``dfldj``, ``logp``, ``dlogp`` (d log p / dx) and ``t = logp + fldj``.

    Sigmoid: with e = exp(-|z|) and r = 1 / (1 + e), the smaller of (sg, 1 - sg) is e r, so
    x = hi - w e r (z >= 0) or lo + w e r (z < 0), dx/dz = w e r^2, fldj = log w - |z| - 2 log1p(e), dfldj/dz = -tanh(z / 2): no
    difference of nearly equal numbers anywhere.  In float32 x is the plain ``lo + w sg`` kept inside [lo, hi]."""
    z = np.asarray(z, dtype=F32).astype(dt)
    a, b, lo, hi = dt(s.a), dt(s.b), dt(s.lo), dt(s.hi)
    one, zero = np.ones_like(z), np.zeros_like(z)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        lnx = None
        if s.bij == ID:
            x, dxdz, fldj, dfldj = z.copy(), one, zero, zero
            xs = np.abs(x)
        elif s.bij == EXP:
            x = np.exp(z)
            dxdz, fldj, dfldj, lnx, xs = x, z, one, z, np.abs(x)
        else:
            w = hi - lo
            az = np.abs(z)
            e = np.exp(-az)
            r = dt(1) / (dt(1) + e)
            small = e * r
            sg = np.where(z >= 0, r, small)
            if dt is F64:
                x = np.where(z >= 0, hi - w * small, lo + w * small)
            else:
                x = lo + w * sg
            x = np.minimum(np.maximum(x, lo), hi)
            xs = np.abs(lo) + np.abs(w * sg)
            dxdz = w * e * (r * r)
            fldj = np.log(w) - az - dt(2) * np.log1p(e)
            dfldj = -np.tanh(dt(0.5) * z)
        if s.prior in (NORMAL, TRUNC):
            u = (x - a) / b
            logp = dt(-0.5) * u * u - np.log(b) - dt(HALF_LOG_2PI)
            dlogp = -u / b
            if s.prior == TRUNC:
                logp = logp - dt(log_norm(s))
                inside = (x >= lo) & (x <= hi)
                logp = np.where(inside, logp, dt(-np.inf))
                dlogp = np.where(inside, dlogp, dt(0))
        elif s.prior == LOGNORMAL:
            if lnx is None:
                lnx = np.log(x)
            u = (lnx - a) / b
            logp = dt(-0.5) * u * u - np.log(b) - dt(HALF_LOG_2PI) - lnx
            dlogp = (-u / b - dt(1)) / x
        else:
            inside = (x >= lo) & (x <= hi)
            logp = np.where(inside, -np.log(hi - lo) * one, dt(-np.inf))
            dlogp = zero
    out = dict(x=x, xs=xs, dxdz=dxdz, fldj=fldj, dfldj=dfldj, logp=logp, dlogp=dlogp, t=logp + fldj)
    assert all(v.dtype == dt for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


def evaluate(specs, z, dt=F64):
    """Every column of ``z`` [B, d]: the dict of ``eval_column`` with [B, d] arrays."""
    z = np.asarray(z, dtype=F32)
    cols = [eval_column(s, z[:, k], dt) for k, s in enumerate(specs)]
    return {key: np.stack([c[key] for c in cols], axis=1) for key in cols[0]}


def log_prior(ev):
    """sum_k (logp_k + fldj_k), summed in column order in the dtype of ``ev`` (the order of the finalize kernel), and the scale
    sum_k |t_k| of that sum."""
    t = ev["t"]
    acc = np.zeros(t.shape[0], dtype=t.dtype)
    for k in range(t.shape[1]):
        acc = acc + t[:, k]
    return acc, np.abs(t.astype(F64)).sum(axis=1)


def grad_z(ev, G, param_cols):
    """``(G[:, param_col] + dlogp/dx) dx/dz + dfldj/dz`` in the dtype of ``ev``, and the scale of every element: the sum of the
    |addends|.  ``G`` [B, P]: the gradient of the log-likelihood w.r.t. the constrained rows (float32 values)."""
    dt = ev["x"].dtype.type
    g = np.asarray(G, dtype=F32)[:, list(param_cols)].astype(dt)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        val = (g + ev["dlogp"]) * ev["dxdz"] + ev["dfldj"]
        g64, e64 = g.astype(F64), {k: v.astype(F64) for k, v in ev.items()}
        scale = np.abs(g64 * e64["dxdz"]) + np.abs(e64["dlogp"] * e64["dxdz"]) + np.abs(e64["dfldj"])
    return val, scale


def gate(yardstick, floor):
    """4 x the float32 yardstick (the factor of pixsrc_cases.py / multilens_cases.py), never below the derived floor."""
    return np.maximum(4.0 * yardstick, floor)


def worst(dev, scale):
    """Largest ``|dev| / scale`` over the elements with a scale (an element of scale 0 must be met exactly: its gate is 0)."""
    dev, scale = np.abs(np.asarray(dev, dtype=F64)), np.asarray(scale, dtype=F64)
    ok = scale > 0
    return float((dev[ok] / scale[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# EPL coefficient table
# ---------------------------------------------------------------------------------------------------------------------
def epl_head(e1, e2, gamma, cap, dt=F64):
    """``(f, 2 - t, niter, K)`` of one sample in ``dt``: f = (1 - q) / (1 + q) with q = (1 - c) / (1 + c), c = min(|e|, 1);
    t = gamma - 1; niter = log(tol) / log(f) + 2 and K = min(ceil(niter) - 1, cap) terms (0 unless niter > 1)."""
    e1, e2, gamma = dt(F32(e1)), dt(F32(e2)), dt(F32(gamma))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = min(np.sqrt(e1 * e1 + e2 * e2), dt(1))
        q = (dt(1) - c) / (dt(1) + c)
        f = (dt(1) - q) / (dt(1) + q)
        niter = np.log(dt(EPL_TOL32)) / np.log(f) + dt(2)
    K = int(min(math.ceil(niter) - 1, cap)) if niter > 1 else 0
    return f, dt(2) - (gamma - dt(1)), float(niter), K


def epl_table_ref(f, s, K):
    """Rows 0 .. K + 3 of the table, float64, from the definition: c_n = prod_{k<=n} p_k with p_k = -f (2k - s) / (2k + s),
    s = 2 - t; columns (c_n, (2n + 1) c_n, dc_n/df = n c_n / f, dc_n/dt = c_n sum_k (dp_k/dt) / p_k); rows K + 1 .. K + 3 zero.
    Where a factor vanishes (f = 0, gamma = 1) the two derivatives are the same sums written without the division:
    n f^(n-1) prod r_k and sum_k dp_k/dt prod_{j != k} p_j."""
    f, s = float(f), float(s)
    tab = np.zeros((K + 4, 4), dtype=F64)
    tab[0] = (1.0, 1.0, 0.0, 0.0)
    if K == 0:
        return tab
    k = np.arange(1, K + 1, dtype=F64)
    r = -(2 * k - s) / (2 * k + s)
    p = f * r
    dpdt = -f * 4 * k / (2 * k + s) ** 2
    c = np.cumprod(p)
    tab[1:K + 1, 0] = c
    tab[1:K + 1, 1] = (2 * k + 1) * c
    if np.all(p != 0):
        tab[1:K + 1, 2] = k * c / f
        tab[1:K + 1, 3] = c * np.cumsum(dpdt / p)
    else:
        tab[1:K + 1, 2] = k * f ** (k - 1) * np.cumprod(r)
        for n in range(1, K + 1):
            tab[n, 3] = sum(dpdt[j] * np.prod(np.delete(p[:n], j)) for j in range(n))
    return tab


def epl_table_f32(f, s, K):
    """The same table by the float32 recurrence (c, cf, ct) <- (c p, cf p + c r, ct p + c dp/dt), one row after the other."""
    f, s = F32(f), F32(s)
    tab = np.zeros((K + 4, 4), dtype=F32)
    tab[0] = (1.0, 1.0, 0.0, 0.0)
    c, cf, ct = F32(1), F32(0), F32(0)
    for n in range(1, K + 1):
        iden = F32(1) / (F32(2 * n) + s)
        r = -(F32(2 * n) - s) * iden
        pn = f * r
        dpdt = -f * F32(4 * n) * (iden * iden)
        cf = cf * pn + c * r
        ct = ct * pn + c * dpdt
        c = c * pn
        tab[n] = (c, F32(2 * n + 1) * c, cf, ct)
    return tab


def table_row_errors(got, ref):
    """Per row the largest error of its four entries relative to the entry's own value; an entry that is exactly zero in the
    reference must be exactly zero (its error is 0 or inf)."""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.where(got == 0, 0.0, np.inf))
    return rel.max(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# models and the case matrix
# ---------------------------------------------------------------------------------------------------------------------
NUM_PIX, DELTA_PIX = 8, 0.25
MODELS = ("epl", "sie", "nfw", "wide", "epl65")
# front-end variants: the environment of the model's creation, and the model they run on
VARIANTS = {
    "wave_lds": ({}, "epl"),                                   # gl_prep_wave_kernel, rows in LDS
    "wave_global": ({"GIGALENS_HIP_PREP_LDS": "0"}, "epl"),    # gl_prep_wave_kernel, the row read back behind __threadfence_block
    "thread": ({"GIGALENS_HIP_WAVE_PREP": "0"}, "epl"),        # gl_prep_kernel on an EPL model: the sequential table
    "sie": ({}, "sie"),                                        # gl_prep_kernel, no EPL
    "epl65": ({}, "epl65"),                                    # an EPL model of more than 64 components: gl_prep_kernel
}


def physical_model(model, niter=50):
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    if model == "epl":
        return PhysicalModel([EPL(niter=niter), Shear()], [], [Sersic()])
    if model == "sie":
        return PhysicalModel([SIE(), Shear()], [], [Sersic()])
    if model == "nfw":  # an NFW lens: gl_finalize_kernel<false>
        return PhysicalModel([EPL(niter=niter), NFW()], [], [Sersic()])
    if model == "wide":  # P = 8 + 18 x 7 = 134 packed columns
        return PhysicalModel([EPL(niter=niter), Shear()], [], [SersicEllipse() for _ in range(18)])
    if model == "epl65":  # 65 components, P = 6 + 64 x 5 = 326
        return PhysicalModel([EPL(niter=niter)], [], [Sersic() for _ in range(64)])
    raise KeyError(model)


def sim_config(num_pix=NUM_PIX):
    from gigalens_amd.simulator import SimulatorConfig
    return SimulatorConfig(delta_pix=DELTA_PIX, num_pix=num_pix)


def slots(phys):
    """``[(group, index, name)]`` of the packed columns."""
    return [(g, i, n) for g, i, n, _ in phys._packing().slots]


SIG_A, SIG_B = (-0.7, 0.1), (1.5, 2.5)  # the two Sigmoid ranges of the matrix
# Sigmoid columns: every row of a case takes the next value (all Sigmoid columns of a row share it)
SIG_GRID = (0.0, 17.0, -17.0, 1e-3, -1e-3, 1.0, -1.0, 4.0, -4.0, 8.0, -8.0, 12.0, -12.0, 15.0, -15.0, 20.0, -20.0, 40.0, -40.0,
            80.0, -80.0)
SATURATED = 17.0  # |z| from which a Sigmoid column counts as saturated

# prior-typical columns by parameter name (models and columns a case does not set otherwise); physically valid at every z of the grid
DEFAULTS = {
    "theta_E": Spec(EXP, LOGNORMAL, math.log(0.6), 0.3, zr=(-0.9, -0.2)),
    "gamma": Spec(SIG, TRUNC, 2.12, 0.25, *SIG_B),
    "e1": Spec(SIG, TRUNC, -0.2, 0.2, *SIG_A),
    "e2": Spec(SIG, UNIFORM, 0.0, 1.0, *SIG_A),
    "center_x": Spec(ID, NORMAL, 0.0, 0.05, zr=(-0.08, 0.08)),
    "center_y": Spec(ID, NORMAL, 0.0, 0.05, zr=(-0.08, 0.08)),
    "gamma1": Spec(ID, NORMAL, 0.0, 0.05, zr=(-0.05, 0.05)),
    "gamma2": Spec(ID, NORMAL, 0.0, 0.05, zr=(-0.05, 0.05)),
    "R_sersic": Spec(EXP, LOGNORMAL, math.log(0.3), 0.15, zr=(-1.5, -0.9)),
    "n_sersic": Spec(SIG, UNIFORM, 0.0, 1.0, *SIG_B),
    "Ie": Spec(EXP, LOGNORMAL, math.log(20.0), 0.5, zr=(2.0, 4.0)),
    "Rs": Spec(EXP, LOGNORMAL, math.log(0.5), 0.3, zr=(-1.0, -0.3)),
    "alpha_Rs": Spec(EXP, LOGNORMAL, math.log(0.3), 0.3, zr=(-1.5, -0.8)),
}
CONSTANTS = {"theta_E": 0.6, "gamma": 2.0, "e1": 0.05, "e2": -0.03, "center_x": 0.01, "center_y": -0.02, "gamma1": 0.01,
             "gamma2": -0.01, "R_sersic": 0.3, "n_sersic": 2.0, "Ie": 10.0, "Rs": 0.5, "alpha_Rs": 0.3}

# The twelve (bijector, prior) pairs gl_model_set_prior accepts, on the columns of the "epl" model (the "nfw" model: its NFW takes the
# Shear's two).  Tight Normal / TruncatedNormal scales under the Sigmoid columns: d log p / dx is large there, so the chain-rule
# factor dx/dz carries weight in the gradient at |z| = 8 .. 15.  Supports of Uniform / TruncatedNormal hold every x the rows visit.
# No location sits where a row puts x (the midpoint of a Sigmoid range at z = 0, the image of an Exp range): x - a would cancel and
# d log p / dx be rounding noise of x on the scale |dlogp/dx dx/dz| -- a property of the input, in float32 of any form.
PAIRS = {
    ("lens_mass", 0, "theta_E"): Spec(EXP, LOGNORMAL, math.log(0.6), 0.3, zr=(-0.9, -0.2)),
    ("lens_mass", 0, "gamma"): Spec(SIG, LOGNORMAL, 1.0, 0.2, *SIG_B),
    ("lens_mass", 0, "e1"): Spec(SIG, UNIFORM, 0.0, 1.0, *SIG_A),
    ("lens_mass", 0, "e2"): Spec(SIG, TRUNC, -0.2, 0.02, *SIG_A),
    ("lens_mass", 0, "center_x"): Spec(ID, NORMAL, 0.0, 0.05, zr=(-0.08, 0.08), edge=(500.0, -500.0)),
    ("lens_mass", 0, "center_y"): Spec(ID, UNIFORM, 0.0, 1.0, -1000.0, 1000.0, zr=(-0.08, 0.08)),
    ("lens_mass", 1, "gamma1"): Spec(ID, TRUNC, 0.0, 0.1, -0.5, 0.5, zr=(-0.3, 0.3)),
    ("lens_mass", 1, "gamma2"): Spec(SIG, NORMAL, -0.2, 0.02, *SIG_A),
    ("lens_mass", 1, "Rs"): Spec(EXP, TRUNC, 1.0, 0.3, 0.01, 10.0, zr=(-1.0, -0.3)),
    ("lens_mass", 1, "alpha_Rs"): Spec(SIG, NORMAL, 2.12, 0.02, *SIG_B),
    ("lens_mass", 1, "center_x"): Spec(ID, TRUNC, 0.0, 0.1, -0.5, 0.5, zr=(-0.3, 0.3)),
    ("lens_mass", 1, "center_y"): Spec(SIG, NORMAL, -0.2, 0.02, *SIG_A),
    ("source_light", 0, "R_sersic"): Spec(EXP, UNIFORM, 0.0, 1.0, 0.01, 10.0, zr=(-1.5, 0.5)),
    ("source_light", 0, "n_sersic"): Spec(EXP, TRUNC, 4.0, 1.5, 0.3, 8.0, zr=(0.0, 1.2)),
    ("source_light", 0, "center_x"): Spec(ID, LOGNORMAL, -1.0, 1.5, zr=(0.02, 0.4), edge=(0.05, 2.0, 500.0)),
    ("source_light", 0, "center_y"): Spec(SIG, TRUNC, 2.12, 0.02, *SIG_B),
    ("source_light", 0, "Ie"): Spec(EXP, NORMAL, 0.0, 1e8, zr=(1.0, 4.0), edge=(20.0, -20.0, 20.0, -20.0)),
}


@dataclass(frozen=True)
class Case:
    """``kind``: which test of tests/test_gpu_zspace.py runs it.  ``d_z``: how many packed columns z drives (None: all); ``perm``:
    z lists the driven columns in a shuffled order; ``consts``: slots held constant; ``typical``: Sigmoid columns draw from (-2, 2)
    instead of walking SIG_GRID; ``rows``: per-row overrides {row: {slot: z}}; ``extra``: case-specific settings."""
    id: str
    kind: str
    variant: str = "wave_lds"
    model: str = ""
    niter: int = 50
    B: int = len(SIG_GRID)
    pairs: bool = True
    d_z: int = None
    perm: bool = False
    consts: Tuple = ()
    typical: bool = False
    seed: int = 0
    env: Tuple = ()
    extra: Dict = field(default_factory=dict, hash=False, compare=False)

    @property
    def model_name(self):
        return self.model or VARIANTS[self.variant][1]

    @property
    def environment(self):
        return {**VARIANTS[self.variant][0], **dict(self.env)}


@dataclass
class Built:
    case: Case
    phys: object
    slots: list
    specs: list         # per column of z
    param_cols: list    # per column of z
    const_row: np.ndarray
    z: np.ndarray       # [B, d_z] float32

    @property
    def columns(self):
        """The raw tuples of ``Model.set_prior``."""
        return [(pc, s.bij, s.prior, s.a, s.b, s.lo, s.hi, f32(log_norm(s))) for pc, s in zip(self.param_cols, self.specs)]

    def rows(self, x):
        """Packed rows [B, P] from the constrained columns ``x`` [B, d_z] (float32) and the constants."""
        out = np.broadcast_to(self.const_row, (x.shape[0], self.const_row.size)).astype(F32).copy()
        out[:, self.param_cols] = np.asarray(x, dtype=F32)
        return out


def _table_rows(cap):
    """(e1, e2, gamma) of the EPL table cases: |e| = f chosen so that niter = K + 0.5, for K on both sides of the wavefront's
    64 rows per round (K + 3 >= 64 from K = 61), of 128, and beyond every cap; e = 0 (K = 1, p_1 = -0 f); gamma = 1 (p_1 = 0)."""
    rows = []
    for i, K in enumerate((12, 49, 60, 61, 64, 65, 127, 128, 129, 400)):
        f = math.exp(math.log(EPL_TOL32) / (K + 0.5 - 2))
        phi = 0.4 + 0.55 * i
        rows.append((f * math.cos(phi), f * math.sin(phi), (2.0, 1.7, 2.3)[i % 3]))
    rows.append((0.0, 0.0, 2.0))
    rows.append((0.3, -0.4, 1.0))
    rows.append((-0.62, 0.5, 1.0))
    return np.asarray(rows, dtype=F32)


def build(case):
    phys = physical_model(case.model_name, case.niter)
    sl = slots(phys)
    rng = np.random.default_rng(2024 + case.seed)
    driven = [p for p, s in enumerate(sl) if s not in case.consts]
    if case.d_z is not None:  # the first d_z of a fixed shuffle of the columns, back in packed order unless `perm`
        driven = sorted(rng.permutation(driven)[:case.d_z].tolist())
    if case.perm:
        driven = rng.permutation(driven).tolist()
    over = case.extra.get("specs", {})
    specs = [over.get(sl[p]) or (PAIRS.get(sl[p]) if case.pairs else None) or DEFAULTS[sl[p][2]] for p in driven]
    const_row = np.asarray([case.extra.get("const_values", {}).get(s, CONSTANTS[s[2]]) for s in sl], dtype=F32)
    B = case.B
    z = np.empty((B, len(driven)), dtype=F32)
    for k, s in enumerate(specs):
        col = rng.uniform(s.zr[0], s.zr[1], size=B)
        if s.bij == SIG:
            col = rng.uniform(-2.0, 2.0, size=B) if case.typical else np.asarray([SIG_GRID[b % len(SIG_GRID)] for b in range(B)])
        elif not case.typical:
            col[:min(B, len(s.edge))] = s.edge[:B]
        z[:, k] = col
    for b, d in case.extra.get("rows", {}).items():
        for slot, v in d.items():
            z[b, driven.index(sl.index(slot))] = v
    if "table_rows" in case.extra:  # Identity columns: z is the physical value
        t = case.extra["table_rows"]
        for j, name in enumerate(("e1", "e2", "gamma")):
            z[:, driven.index(sl.index(("lens_mass", 0, name)))] = t[:, j]
    return Built(case, phys, sl, specs, driven, const_row, z)


_ID_N = lambda s, lo, hi: Spec(ID, NORMAL, 0.0, s, zr=(lo, hi))
# e1, e2, gamma (and what else is listed) under an Identity: z IS the packed value, so the EPL table cases place |e| exactly
_TABLE_SPECS = {
    ("lens_mass", 0, "theta_E"): _ID_N(1.0, 0.4, 0.7), ("lens_mass", 0, "gamma"): _ID_N(3.0, 1.7, 2.3),
    ("lens_mass", 0, "e1"): _ID_N(1.0, -0.3, 0.3), ("lens_mass", 0, "e2"): _ID_N(1.0, -0.3, 0.3),
    ("source_light", 0, "R_sersic"): _ID_N(1.0, 0.2, 0.4), ("source_light", 0, "n_sersic"): _ID_N(3.0, 1.5, 3.0),
    ("source_light", 0, "Ie"): _ID_N(50.0, 5.0, 30.0),
}
_CHAIN_SPECS = {  # prior-typical pairs; the amplitude under an Identity so that a row can make it negative
    ("lens_mass", 0, "gamma"): Spec(SIG, TRUNC, 2.12, 0.25, *SIG_B),
    ("lens_mass", 0, "e1"): Spec(SIG, UNIFORM, 0.0, 1.0, *SIG_A),
    ("lens_mass", 0, "e2"): Spec(SIG, TRUNC, -0.2, 0.2, *SIG_A),
    ("source_light", 0, "n_sersic"): Spec(SIG, UNIFORM, 0.0, 1.0, *SIG_B),
    ("source_light", 0, "Ie"): Spec(ID, NORMAL, 50.0, 20.0, zr=(20.0, 60.0)),
}
_CHAIN_SIG = (0.3, -0.5, 8.0, -12.0, 15.0, -4.0, 12.0, -8.0)  # Sigmoid z of the rows of the chain case
_SIG_SLOTS = [k for k, s in _CHAIN_SPECS.items() if s.bij == SIG]
NAN_ROW = 1
_ORDER_SPECS = {("lens_mass", 0, "e1"): Spec(SIG, TRUNC, -0.3, 0.2, *SIG_A), ("lens_mass", 0, "e2"): Spec(SIG, TRUNC, -0.3, 0.2, *SIG_A)}


def _cases():
    out = []
    for v in VARIANTS:
        out.append(Case(f"forward-{v}", "forward", variant=v, B=5 if v == "epl65" else len(SIG_GRID), pairs=v != "epl65"))
    out.append(Case("isolated-basic", "isolated", model="epl"))   # gl_finalize_kernel<true>
    out.append(Case("isolated-full", "isolated", model="nfw"))    # gl_finalize_kernel<false>
    out.append(Case("chain-epl", "chain", model="epl", B=len(_CHAIN_SIG), perm=True, typical=True, pairs=False, seed=3,
                    consts=(("lens_mass", 0, "center_x"), ("source_light", 0, "center_x")),
                    extra=dict(specs=_CHAIN_SPECS,
                               rows={b: {**{s: v for s in _SIG_SLOTS},
                                         **({("source_light", 0, "Ie"): -50.0} if b == NAN_ROW else {})}
                                     for b, v in enumerate(_CHAIN_SIG)})))
    for B in (1, 3, 5, 45):  # 5: a partly empty four-sample workgroup; 45 x 3 components cross gl_prep_kernel's 128 threads
        for v in ("wave_lds", "thread"):
            out.append(Case(f"shape-B{B}-{v}", "shape", variant=v, B=B, seed=B))
    for d in (1, 13, 63, 64, 65, 130):  # both kernels stride the columns of z by 64; P = 134 > 64 with constants
        out.append(Case(f"shape-d{d}", "shape", model="wide", B=3, d_z=d, perm=True, pairs=False, seed=d))
    for niter in (50, 61, 64, 65, 130, 300):
        for v, name in (("wave_lds", "scan"), ("thread", "sequential")):
            rows = _table_rows(niter)
            out.append(Case(f"table-n{niter}-{name}", "table", variant=v, niter=niter, B=len(rows), typical=True, seed=7,
                            extra=dict(specs=_TABLE_SPECS, table_rows=rows)))
    for fused in ("1", "0"):
        env = (("GIGALENS_HIP_ORDER_FUSED", fused),)
        out.append(Case(f"order-truncnormal-fused{fused}", "order", model="epl", B=257, typical=True, pairs=False, seed=11, env=env,
                        extra=dict(specs=_ORDER_SPECS)))
        out.append(Case(f"order-constant-e1-fused{fused}", "order", model="epl", B=257, typical=True, pairs=False, seed=12, env=env,
                        consts=(("lens_mass", 0, "e1"),), extra=dict(specs=_ORDER_SPECS, const_values={("lens_mass", 0, "e1"): 0.3})))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
LONG_NITER, LONG_PIX, LONG_B = 140, 16, 3  # the long series end to end: EPL(niter=140), |e| ~ 0.8 (test_gpu_zspace.py)


def of_kind(*kinds):
    return [c for c in CASES if c.kind in kinds]


_REF = {}


def reference(case_id):
    """``(built, float64 evaluation, float32 evaluation)`` of a case, computed once and left unchanged."""
    if case_id not in _REF:
        b = build(BY_ID[case_id])
        _REF[case_id] = (b, evaluate(b.specs, b.z, F64), evaluate(b.specs, b.z, F32))
    return _REF[case_id]


def long_workload():
    """EPL(niter=140) + Shear | Sersic at |e| ~ 0.8 on 16 x 16, three samples: the series runs ~95 (float32) / ~126 (float64 oracle)
    terms, beyond the 50 rows of every other pixel-likelihood case and the 64 rows of one scan round."""
    from gigalens_amd import prior as tfd
    from gigalens_amd.workloads import Workload
    J, S, N = tfd.JointDistributionNamed, tfd.JointDistributionSequential, tfd.Normal
    prior = J(dict(lens_mass=S([J(dict(theta_E=tfd.LogNormal(math.log(0.7), 0.05), gamma=tfd.TruncatedNormal(2.0, 0.1, 1.5, 2.5),
                                       e1=N(0.62, 0.01), e2=N(0.5, 0.01), center_x=N(0.01, 0.01), center_y=N(-0.02, 0.01))),
                                J(dict(gamma1=N(0, 0.02), gamma2=N(0, 0.02)))]),
                   source_light=S([J(dict(R_sersic=tfd.LogNormal(math.log(0.3), 0.1), n_sersic=tfd.Uniform(1.0, 3.0),
                                          center_x=N(0.05, 0.03), center_y=N(-0.03, 0.03), Ie=tfd.LogNormal(math.log(50.0), 0.2)))])))
    return Workload("LONG", physical_model("epl", LONG_NITER), prior, sim_config(LONG_PIX), LONG_B)
