"""The post-processing matrix: every PSF / pooling kernel of csrc/gl_post.hip.h against a float64 convolution written from the
definition (tests/test_post_host.py checks the matrix and the reference without a GPU, tests/test_gpu_post.py runs it).

The reference.  LensSimulator.simulate's post-processing of a supersampled stack S [B, Hs, Ws] with a PSF [kh, kw] is
    flip the PSF; cross-correlate with TF 'SAME' padding ((k - 1) // 2 zeros before, k // 2 after); ss x ss mean pool; x scale
`post_fwd_f64` is those four steps in numpy float64 and `post_bwd_f64` their explicit adjoint, step by step in reverse.  Neither
forms the effective kernel flip(psf) (*) box / ss^2 or the residue classes the HIP kernels work with.

The bound.  A float32 sum of n products, each formed by a fused multiply-add, in ANY order differs from the exact sum by at most
gamma_n * sum |s_i| |k_i| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1; partial sums added across wavefronts count as further additions).  Per output element
    n = (kernel rows) x (padded row width)      the multiply-adds the kernel executes for it, zero padding taps included
      + (KS - 1)                                the additions of the other row groups' partial sums
      + 2                                       the rounding of the effective kernel to float32, and the final x scale
and the element's own sum of absolute products comes from the reference applied to |S| and |psf|.  Nothing in the bound is
measured on the kernels."""
import zlib
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

ENV_KNOBS = ("GIGALENS_HIP_CORR_PAIR", "GIGALENS_HIP_CORR_WIDE", "GIGALENS_HIP_CORR_MAXPAIRS")
U = 2.0 ** -24
MAX_SIDE = 96  # supersampled pixels a side, at most

TAP_F, TAP_B = "gl_psf_pool_fwd_kernel", "gl_psf_pool_bwd_kernel"


def P(kwp, st, ks, ncj, ox):
    """gl_corr_pair_kernel<KWP, ST, KS, NCJ, OX> as the demangler spells it"""
    return f"gl_corr_pair_kernel<{kwp}, {st}, {ks}, {ncj}, {ox}>"


def S1(kwp):   # stride 1, one column class: forward and transpose at supersample 1
    return P(kwp, 1, 2, 1, 8)


def WIDE(kwp):  # forward at supersample 2, 16 outputs per thread, 8 row groups (KWP <= 28 and KH <= 28)
    return P(kwp, 2, 8, 1, 16)


def S2(kwp):   # forward at supersample 2, 8 outputs per thread, 4 row groups
    return P(kwp, 2, 4, 1, 8)


def T2(kwp):   # transpose at supersample 2: two column classes per thread
    return P(kwp, 1, 2, 2, 8)


def short_name(demangled: str) -> str:
    """'void glk::gl_corr_pair_kernel<4, 1, 2, 1, 8>(float const*, float*, glk::CorrArgs)' -> 'gl_corr_pair_kernel<4, 1, 2, 1, 8>';
    'glk::gl_psf_pool_fwd_kernel(float const*, float*, glk::PostArgs)' -> 'gl_psf_pool_fwd_kernel'"""
    s = demangled.strip()
    if s.startswith("void "):
        s = s[5:]
    if s.startswith("glk::"):
        s = s[5:]
    depth = 0
    for i, ch in enumerate(s):  # cut the parameter list: the first '(' outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def pair_args(name: str) -> Optional[Tuple[int, ...]]:
    """(KWP, ST, KS, NCJ, OX) of a pair-kernel name, None for the tap kernels"""
    if not name.startswith("gl_corr_pair_kernel<"):
        return None
    return tuple(int(v) for v in name[len("gl_corr_pair_kernel<"):-1].split(","))


@dataclass(frozen=True)
class Case:
    id: str
    psf: Optional[Tuple[int, int]]  # (rows, columns) on the supersampled grid, None = pooling only
    ss: int
    n: int                          # pooled image side; the supersampled stack is (n ss) x (n ss)
    batch: int
    fwd: str                        # kernel expected to serve the forward launch ...
    bwd: str                        # ... and the transposed one
    env: Dict[str, str] = field(default_factory=dict)
    offset: int = 0                 # the input stack starts this many floats after a 16-byte boundary
    scale: float = 0.0064           # 0.08^2, the det(T) of the suites' cameras

    @property
    def hs(self):
        return self.n * self.ss

    @property
    def kh(self):
        return self.psf[0] if self.psf else 1

    @property
    def kw(self):
        return self.psf[1] if self.psf else 1

    @property
    def KH(self):  # the effective kernel's sides
        return self.kh + self.ss - 1

    @property
    def KW(self):
        return self.kw + self.ss - 1


def _env(pair=None, wide=None, maxpairs=None):
    return {k: str(v) for k, v in zip(ENV_KNOBS, (pair, wide, maxpairs)) if v is not None}


C = Case
CASES = [
    # ---- supersample 1: <KWP, 1, 2, 1, 8> in both directions, every KWP; square / rectangular, even / odd sides; widths 0..3 mod 4
    C("s1_1x1", (1, 1), 1, 20, 1, S1(4), S1(4)),
    C("s1_3x2", (3, 2), 1, 33, 2, S1(4), S1(4)),
    C("s1_5x7", (5, 7), 1, 22, 3, S1(8), S1(8)),
    C("s1_12x9", (12, 9), 1, 35, 2, S1(12), S1(12)),
    C("s1_13x16_on_grid", (13, 16), 1, 32, 3, S1(16), S1(16)),          # 32 x 32: whole 16 x 32 tiles, float4 path
    C("s1_17x17", (17, 17), 1, 48, 2, S1(20), S1(20)),
    C("s1_9x24", (9, 24), 1, 21, 3, S1(24), S1(24)),
    C("s1_27x25", (27, 25), 1, 40, 2, S1(28), S1(28)),
    C("s1_31x32_kw32", (31, 32), 1, 64, 2, S1(32), S1(32)),             # KW = 32: the widest the pair kernel serves
    C("s1_7x33_kw33", (7, 33), 1, 36, 2, TAP_F, TAP_B),                 # KW = 33: the tap kernels
    C("s1_64x5_kh64", (64, 5), 1, 24, 2, S1(8), S1(8)),                 # KH = 64: the tallest
    C("s1_65x5_kh65", (65, 5), 1, 24, 2, TAP_F, TAP_B),                 # KH = 65: the tap kernels
    C("s1_small_tile", (5, 5), 1, 9, 3, S1(8), S1(8)),                  # smaller than one tile
    C("s1_offset_scalar_path", (7, 7), 1, 32, 3, S1(8), S1(8), offset=1),  # widths multiples of four, input one float off: vec = 0
    C("s1_b16", (4, 6), 1, 36, 16, S1(8), S1(8)),                       # 8 pairs: the whole launch in the XCD remap's first branch
    C("s1_b17", (6, 3), 1, 34, 17, S1(4), S1(4)),                       # 9 pairs: full = 8, rest = 1, odd last pair
    C("s1_b7_maxpairs3", (5, 5), 1, 36, 7, S1(8), S1(8), env=_env(maxpairs=3)),  # slices of 6 and 1 samples
    C("s1_pair_off", (9, 9), 1, 24, 3, TAP_F, TAP_B, env=_env(pair=0)),
    # ---- supersample 2, forward wide <KWP, 2, 8, 1, 16> (every KWP), transpose <KWP, 1, 2, 2, 8> (every KWP)
    C("s2_pool_only", None, 2, 22, 3, WIDE(4), T2(4)),                  # no PSF: KW = 2
    C("s2_1x1", (1, 1), 2, 19, 2, WIDE(4), T2(4)),
    C("s2_6x5", (6, 5), 2, 21, 3, WIDE(8), T2(4)),
    C("s2_9x8", (9, 8), 2, 32, 2, WIDE(12), T2(8)),                     # 64 x 64 -> 32 x 32, on the 16 x 32 grid of the transpose
    C("s2_13x13_demo", (13, 13), 2, 30, 5, WIDE(16), T2(8), scale=-1.25),  # the reference's demo PSF; a negative scale
    C("s2_15x17", (15, 17), 2, 23, 2, WIDE(20), T2(12)),
    C("s2_8x21", (8, 21), 2, 26, 3, WIDE(24), T2(12)),
    C("s2_27x27_wide_edge", (27, 27), 2, 36, 2, WIDE(28), T2(16)),      # KWP = 28 and KH = 28: the last wide
    C("s2_27x28_kwp32", (27, 28), 2, 36, 2, S2(32), T2(16)),            # KWP = 32: not wide
    C("s2_28x27_kh29", (28, 27), 2, 36, 2, S2(28), T2(16)),             # KH = 29: not wide
    C("s2_small_tile", (3, 3), 2, 7, 3, WIDE(4), T2(4)),
    C("s2_on_grid_48", (5, 6), 2, 48, 2, WIDE(8), T2(4)),               # 96 x 96 -> 48 x 48
    C("s2_b15", (5, 5), 2, 40, 15, WIDE(8), T2(4)),                     # 8 pairs, odd last pair
    C("s2_b17", (3, 5), 2, 34, 17, WIDE(8), T2(4)),                     # 9 pairs: rest = 1 with two row classes in the transpose
    C("s2_b33_narrow", (4, 4), 2, 33, 33, S2(8), T2(4), env=_env(wide=0)),  # 17 pairs: full = 16, rest = 1
    C("s2_b5_maxpairs1", (7, 7), 2, 24, 5, WIDE(8), T2(8), env=_env(maxpairs=1)),  # slices of 2, 2 and 1 samples
    C("s2_basis_stack", (9, 9), 2, 20, 12, WIDE(12), T2(8), scale=1.0),  # lstsq's basis stack: B x D = 3 x 4 images, no det(T)
    C("s2_offset_scalar_path", (5, 5), 2, 24, 3, WIDE(8), T2(4), offset=1),
    # ---- supersample 2, forward <KWP, 2, 4, 1, 8>: every KWP with GIGALENS_HIP_CORR_WIDE=0, and without the knob beyond the wide rule
    C("s2_narrow_kwp4", (3, 2), 2, 25, 3, S2(4), T2(4), env=_env(wide=0)),
    C("s2_narrow_kwp12", (5, 11), 2, 22, 2, S2(12), T2(8), env=_env(wide=0)),
    C("s2_narrow_kwp16", (13, 13), 2, 30, 3, S2(16), T2(8), env=_env(wide=0)),
    C("s2_narrow_kwp20", (11, 18), 2, 27, 2, S2(20), T2(12), env=_env(wide=0)),
    C("s2_narrow_kwp24", (29, 22), 2, 28, 2, S2(24), T2(12)),           # KH = 30 > 28: not wide, no knob
    C("s2_narrow_kwp28", (9, 25), 2, 20, 3, S2(28), T2(16), env=_env(wide=0)),
    C("s2_31x31_kw32", (31, 31), 2, 32, 2, S2(32), T2(20)),             # KW = 32: the only transpose plan 17 taps wide
    C("s2_3x32_kw33", (3, 32), 2, 24, 2, TAP_F, TAP_B),                 # KW = 33
    C("s2_63x3_kh64", (63, 3), 2, 20, 2, S2(4), T2(4)),                 # KH = 64
    C("s2_64x3_kh65", (64, 3), 2, 20, 2, TAP_F, TAP_B),                 # KH = 65
    # the LDS limit of the non-wide stride-2 forward kernel at KWP = 32: (30 + KH) x 101 float2 <= 64 KB up to KH = 51
    C("s2_50x30_lds_fits", (50, 30), 2, 20, 2, S2(32), T2(16)),
    C("s2_51x30_lds_falls_back", (51, 30), 2, 20, 2, TAP_F, T2(16)),    # forward: the tap kernel; the transpose plan still fits
    # ---- supersample 3: the tap kernels
    C("s3_5x5", (5, 5), 3, 17, 3, TAP_F, TAP_B),
    C("s3_pool_only", None, 3, 32, 2, TAP_F, TAP_B),
    C("s3_4x7_b16", (4, 7), 3, 12, 16, TAP_F, TAP_B),
]
del C


def declared_names():
    return {k for c in CASES for k in (c.fwd, c.bwd)}


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _rng(case, salt):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{salt}".encode()))


def make_psf(case):
    """asymmetric, every tap significant: uniform(0.1, 1), normalised (float32, as LensSimulator receives it)"""
    if case.psf is None:
        return None
    k = _rng(case, "psf").uniform(0.1, 1.0, size=case.psf)
    return (k / k.sum()).astype(np.float32)


def in_shape(case, transpose):
    side = case.n if transpose else case.hs
    return (case.batch, side, side)


def out_shape(case, transpose):
    return in_shape(case, not transpose)


def random_input(case, transpose):
    """N(0, 1) with a different amplitude per sample"""
    r = _rng(case, f"random{int(transpose)}")
    shape = in_shape(case, transpose)
    amp = 10.0 ** r.uniform(-2, 2, size=(shape[0], 1, 1))
    return (amp * r.normal(size=shape)).astype(np.float32)


def impulse_input(case, transpose):
    """One impulse per sample: position and amplitude differ per sample.  Positions walk the image corners, the last row and
    column, and both sides of the kernels' tile edges (16 output rows, 32 or 64 output columns; in input pixels of either
    direction), clipped to the image."""
    shape = in_shape(case, transpose)
    B, n, _ = shape
    st = 1 if transpose else case.ss
    cand = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, n - 1), (n - 1, n // 3),
            (16 * st - 1, 32 * st - 1), (16 * st, 32 * st), (16 * st - 1, 32 * st), (16 * st, 64 * st - 1), (15, 31), (16, 32),
            (8, 16), (32 * st - 1, 16 * st), (n // 2 + 1, n // 2)]
    x = np.zeros(shape, dtype=np.float32)
    for b in range(B):
        i, j = cand[b % len(cand)]
        i, j = min(i, n - 1), min(j, n - 1)
        x[b, i, j] = np.float32((-1.0) ** b * (1.5 + 0.37 * b))
    return x


# ---- the float64 reference, from the definition -----------------------------------------------------------------------------
def _pads(k):
    return (k - 1) // 2, k // 2  # TF 'SAME': the extra zero goes to the end


def post_fwd_f64(S, psf, ss, scale):
    """[B, Hs, Ws] -> [B, Hs / ss, Ws / ss]"""
    S = np.asarray(S, dtype=np.float64)
    B, Hs, Ws = S.shape
    if psf is not None:
        k = np.asarray(psf, dtype=np.float64)[::-1, ::-1]  # flip ...
        kh, kw = k.shape
        (pt, pb), (pl, pr) = _pads(kh), _pads(kw)
        Sp = np.pad(S, ((0, 0), (pt, pb), (pl, pr)))
        conv = np.zeros_like(S)
        for u in range(kh):  # ... and cross-correlate: conv[i, j] = sum_uv Sp[i + u, j + v] k[u, v]
            for v in range(kw):
                conv += k[u, v] * Sp[:, u:u + Hs, v:v + Ws]
    else:
        conv = S
    pooled = conv.reshape(B, Hs // ss, ss, Ws // ss, ss).sum(axis=(2, 4)) / float(ss * ss)
    return pooled * float(scale)


def post_bwd_f64(G, psf, ss, scale, Hs, Ws):
    """The adjoint of post_fwd_f64, step by step in reverse: [B, Hs / ss, Ws / ss] -> [B, Hs, Ws]"""
    G = np.asarray(G, dtype=np.float64) * float(scale)
    B = G.shape[0]
    assert G.shape == (B, Hs // ss, Ws // ss)
    up = np.repeat(np.repeat(G, ss, axis=1), ss, axis=2) / float(ss * ss)  # adjoint of the mean pool
    if psf is None:
        return up
    k = np.asarray(psf, dtype=np.float64)[::-1, ::-1]
    kh, kw = k.shape
    (pt, pb), (pl, pr) = _pads(kh), _pads(kw)
    gSp = np.zeros((B, Hs + pt + pb, Ws + pl + pr))
    for u in range(kh):  # adjoint of the cross-correlation: every tap scatters the cotangent back to where it read
        for v in range(kw):
            gSp[:, u:u + Hs, v:v + Ws] += k[u, v] * up
    return gSp[:, pt:pt + Hs, pl:pl + Ws]  # adjoint of the zero padding


def post_f64(case, x, transpose, psf, scale=None):
    """The reference of the case's direction; `scale` (default: the case's) as the float32 the library receives"""
    scale = float(np.float32(case.scale if scale is None else scale))
    if transpose:
        return post_bwd_f64(x, psf, case.ss, scale, case.hs, case.hs)
    return post_fwd_f64(x, psf, case.ss, scale)


# ---- the derived bound ------------------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1.0 - n * U)


def fma_count(case, transpose, kernel=None):
    """n of the module docstring for the kernel that serves `case` in this direction (default: the declared one)"""
    name = kernel or (case.bwd if transpose else case.fwd)
    rows = -(-case.KH // case.ss) if transpose else case.KH
    args = pair_args(name)
    if args is None:  # the tap kernels: one multiply-add per tap of the element, one wavefront
        width, ks = (-(-case.KW // case.ss) if transpose else case.KW), 1
    else:
        width, ks = args[0], args[2]
    return rows * width + (ks - 1) + 2


def error_bound(case, x, transpose, psf, kernel=None):
    """Per output element: gamma_n |scale| sum |x_i| |k_i| over that element's own taps"""
    apsf = None if psf is None else np.abs(psf)
    return gamma(fma_count(case, transpose, kernel)) * post_f64(case, np.abs(np.asarray(x, dtype=np.float64)), transpose, apsf,
                                                                scale=abs(case.scale))


def impulse_error_in_u(case, xi, y, transpose, psf):
    """The impulse check: per element, |y - float32(Keff) amplitude scale| in units of u |that product| (two roundings: at most
    2 + u), and the number of nonzero outputs where the reference puts no tap.  Keff comes from the reference's response to unit
    impulses.  The reference knows it to float64 rounding only, and with ss = 3 (taps / 9) it often lies on a float32 rounding
    tie, where the last float64 bit decides: both float32 neighbours of such a value are float32(Keff), the nearer result counts."""
    k64 = post_f64(case, (xi != 0).astype(np.float64), transpose, psf, scale=1.0)
    amp = xi.astype(np.float64).sum(axis=(1, 2), keepdims=True)  # the one nonzero of each sample
    hit = k64 != 0
    worst = np.full(k64.shape, np.inf)
    for eps in (-2.0 ** -50, 2.0 ** -50):
        want = (k64 * (1.0 + eps)).astype(np.float32).astype(np.float64) * amp * float(np.float32(case.scale))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = np.minimum(worst, np.where(hit, np.abs(y - want) / np.abs(want) / U, 0.0))
    return float(worst.max()), int(np.count_nonzero(np.asarray(y)[~hit]))
