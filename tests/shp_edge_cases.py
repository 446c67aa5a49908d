"""The shapelet kernels (csrc/gl_shp.hip.h: `gl_shp_kernel`, `gl_shp_normal_kernel`) at every compaction, cull and block edge:
the case list and the float64 geometry that says which edge each case sits on.

Every case fixes every parameter -- nothing is drawn from a prior (`FixedPrior` hands the rows out where a suite asks a
workload's prior for samples).  The model is EPL + Shear, an optional SersicEllipse lens light and one Shapelets source, on a
`Workload` with bg = 1 as tests/dispatch_cases.py builds it for shapelets.

`geometry(case)` ray-shoots the case with oracle/ref_torch.py in float64 and restates, per sample and per wave-tile,
  * the live counts (c0, c1) of the two 64-pixel slots: the pixels with |u|, |v| <= 5, (u, v) = (beta - c) / beta_s;
  * whether every pixel of the wave-tile passes the test of `ShpCull::tile_outside`:
        |x - c|^2 > T^2,  T = 1.001 (5 sqrt2 beta_s + sum of the lenses' bounds),   and   |x - c_lens|^2 >= rb2,
    EPL bound (b/q) grow with grow = max(D/b, 1)^(2 - gamma) for gamma < 2 (D = r_max + |c_lens|), else 1, and
    rb2 = 1.002 (b/q)^2 for gamma > 2, else 0;  shear bound |gamma| r_max  (r_max: the largest |(x, y)| of the grid);
  * how far the pixels stay from the table boundary (| |u| - 5 |, | |v| - 5 |) and from the two cull thresholds.
The pixel -> (wave-tile, slot) map of both orders is restated from `pixel_of`:
  linear   slot w of wave `wave` in the step at `base` = pixels base + 256 w + 64 wave + lane;
  blocked  the image's 8-row x 16-column block 4 (base / 512) + wave in row-major block order, slot w = rows 4 w .. 4 w + 3.
A slot past the end of the pixel list re-reads the list's last pixel (the kernels clamp the index and mask the result), so a
live last pixel counts once per such slot: the restatement keeps that.

A plain module (no GPU, no torch at import)."""
import math
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

from tests import dispatch_cases as DC

MARGIN = 1e-3        # clearance from the table boundary, in (u, v): ~20 float32 ulps of a 2" coordinate / the smallest beta_s
BETA_MIN = 20 * float(np.spacing(np.float32(2.0))) / MARGIN  # the smallest beta_s that margin serves (4.8e-3)
# relative clearance of |x - c|^2 from T^2 and of |x - c_lens|^2 from rb2.  In float32 T = 1.001 (7.07 / (1 / beta_s) + A) carries
# at most ~5 roundings (3e-7), T^2 twice that, a squared distance ~3 more (2e-7): under 1e-6 together, a tenth of this margin
CULL_MARGIN = 1e-5
# clearance of a live pixel's table position fi = (u + 5) 599.9 from the nearest NODE, in node spacings.  The interpolant's slope
# jumps at a node (by ~h S''/S' ~ 1e-3 of itself), and float32 places fi to about 1e-3: (u + 5) rounds to ulp(10) / 2 x 600 =
# 2.9e-4, the product to ulp(6000) / 2 = 2.4e-4, and u = (beta - c) / beta_s itself carries ~1.5 ulp(5) x 600 = 4.3e-4.  Inside
# that distance a float32 evaluation may take the neighbouring interval's slope, and a position gradient that cancels across the
# pixels shows it (the count-pinning cases, whose cancelling sums have few terms, stay outside)
NODE_MARGIN = 1e-3


@dataclass(frozen=True)
class Sample:
    src: Tuple[float, float, float]                      # beta_s, center_x, center_y of the shapelet source
    lens: Tuple[float, ...] = (1e-3, 2.0, 0.02, -0.01, 0.0, 0.0)   # theta_E, gamma, e1, e2, center_x, center_y
    shear: Tuple[float, float] = (0.0, 0.0)


@dataclass(frozen=True)
class Case:
    id: str
    num_pix: int
    delta_pix: float
    n_max: int
    samples: Tuple[Sample, ...]
    roles: Tuple[str, ...] = ()      # "count": pins wave-tile counts; "cull": a realistic lens whose cull fires; "chunk"; "order"
    interpolate: bool = True
    err: bool = True
    lens_light: bool = False
    pix_region: bool = False
    env: Dict[str, str] = field(default_factory=dict)
    lstsq: bool = False              # use_lstsq=True, no amplitudes: the fused linear solve (gl_shp_normal_kernel)
    pins: Tuple[Tuple[int, int], ...] = ()   # (c0, c1) pairs the case is there for (checked on the host)

    @property
    def batch(self):
        return len(self.samples)

    @property
    def n_pixels(self):
        return int(region(self).sum()) if self.pix_region else self.num_pix ** 2

    @property
    def ragged(self):
        return self.pix_region or self.n_pixels % 512 != 0

    @property
    def kernels(self):
        """gl_shp_kernel<MODE, 2, EPL+Shear, lens light, 6, table, ragged> per mode (dispatch_cases.shp)"""
        return DC.shp(DC.SERE if self.lens_light else DC.NONE, self.interpolate, self.ragged)


def region(case):
    """The circular pixel region of dispatch_cases.workload."""
    n = case.num_pix
    yy, xx = np.mgrid[:n, :n]
    c = (n - 1) / 2
    return (((xx - c) ** 2 + (yy - c) ** 2) < (0.42 * n) ** 2).astype(np.float32)


def blocked(case, fused=False):
    """Whether the launch uses 8 x 16 blocks: table mode on a whole image with width % 16 == 0 and height % 8 == 0, unless
    GIGALENS_HIP_SHP_BLOCKED=0; gl_shp_kernel also needs whole 512-pixel tiles, gl_shp_normal_kernel (`fused`) does not."""
    n = case.num_pix
    ok = case.interpolate and not case.pix_region and n % 16 == 0 and case.env.get("GIGALENS_HIP_SHP_BLOCKED", "1") != "0"
    return ok and (fused or not case.ragged)


def slot_map(n_pix_list, width, blocked_):
    """[wave-tile, slot, lane] -> index into the pixel list (clamped to the last pixel), and the mask of real slots."""
    steps = (n_pix_list + 511) // 512
    s, wave, w, lane = np.meshgrid(np.arange(steps), np.arange(4), np.arange(2), np.arange(64), indexing="ij")
    if blocked_:
        nbx = width // 16
        t = 4 * s + wave
        by, bx = t // nbx, t % nbx
        j = (by * 8 + 4 * w + lane // 16) * width + bx * 16 + lane % 16
    else:
        j = 512 * s + 256 * w + 64 * wave + lane
    j = j.reshape(steps * 4, 2, 64)
    valid = j < n_pix_list
    return np.where(valid, j, n_pix_list - 1), valid


# ---- the models -----------------------------------------------------------------------------------------------------------
class FixedPrior:
    """A 'prior' whose samples are the case's rows: `sample(n)` returns the first n of them, whatever the seed."""

    def __init__(self, struct):
        self.struct = struct

    def sample(self, sample_shape=(), seed=None, **_):
        n = int(np.prod(sample_shape)) if not isinstance(sample_shape, int) else sample_shape
        assert 1 <= n <= len(next(iter(self.struct["lens_mass"][0].values()))), n
        return {g: [{k: v[:n].clone() for k, v in d.items()} for d in lst] for g, lst in self.struct.items()}


def amplitudes(k, n_layers):
    """Sample k's amplitudes: a fixed oscillating sequence of the size of dispatch_cases' prior, N(0, 500 / sqrt(i + 1))."""
    i = np.arange(n_layers)
    return (300.0 * np.cos(0.7 * i + 1.1 * k + 0.3) / np.sqrt(i + 1.0)).astype(np.float32)


def params(case):
    """The case's parameters as the nested struct of float32 tensors (B,) the simulators take."""
    import torch
    from gigalens_amd.profiles.light.shapelets import Shapelets
    col = lambda vals: torch.tensor(np.asarray(vals, dtype=np.float32))
    S = case.samples
    epl = {n: col([s.lens[i] for s in S]) for i, n in enumerate(("theta_E", "gamma", "e1", "e2", "center_x", "center_y"))}
    shear = {n: col([s.shear[i] for s in S]) for i, n in enumerate(("gamma1", "gamma2"))}
    src = {n: col([s.src[i] for s in S]) for i, n in enumerate(("beta", "center_x", "center_y"))}
    if not case.lstsq:
        names = Shapelets(case.n_max)._amp_names
        amps = np.stack([amplitudes(k, len(names)) for k in range(len(S))])
        src.update({nm: col(amps[:, i]) for i, nm in enumerate(names)})
    out = {"lens_mass": [epl, shear], "source_light": [src]}
    if case.lens_light:
        B = len(S)
        out["lens_light"] = [dict(R_sersic=col([0.6] * B), n_sersic=col([2.5] * B), e1=col([0.05] * B), e2=col([-0.04] * B),
                                  center_x=col([0.01] * B), center_y=col([-0.02] * B), Ie=col([20.0 + 3 * k for k in range(B)]))]
    return out


def workload(case):
    """The case's Workload: bg = 1 as dispatch_cases.workload gives the shapelet models, the prior a FixedPrior."""
    from gigalens_amd import workloads as W
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.light.shapelets import Shapelets
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    phys = PhysicalModel([EPL(), Shear()], [SersicEllipse()] if case.lens_light else [],
                         [Shapelets(case.n_max, use_lstsq=case.lstsq, interpolate=case.interpolate)])
    cfg = SimulatorConfig(delta_pix=case.delta_pix, num_pix=case.num_pix, pix_region=region(case) if case.pix_region else None)
    return W.Workload(case.id, phys, FixedPrior(params(case)), cfg, case.batch, background_rms=1.0, use_error_map=case.err)


# ---- float64 geometry -----------------------------------------------------------------------------------------------------
@dataclass
class Geometry:
    c0: np.ndarray            # [B, wave-tiles] live pixels of slot 0 / slot 1
    c1: np.ndarray
    culled: np.ndarray        # [B, wave-tiles] every pixel passes the cull test (False everywhere where the test is off)
    live: np.ndarray          # [B, N] the pixel is inside the table
    clearance: np.ndarray     # [B] smallest | |u| - 5 | or | |v| - 5 | over the pixels
    near: np.ndarray          # [B] pixels whose classification the MARGIN does not settle
    cull_clearance: np.ndarray  # [B] smallest relative distance of |x - c|^2 from T^2 and of |x - c_lens|^2 from rb2
    node_clearance: np.ndarray  # [B] smallest distance of a live pixel's fi = (u + 5) 599.9 from a node, u and v alike
    rb2_decides: np.ndarray   # [B] wave-tiles far from the source that a pixel inside the lens's rb2 radius keeps un-culled
    blocked: bool

    @property
    def count(self):
        return self.c0 + self.c1

    @property
    def tiles(self):
        return self.c0.size

    def rounds(self, interpolate=True):
        """chain rounds of a launch: sum of ceil(count / 64) in table mode, 2 per wave-tile in direct mode"""
        return int(((self.count + 63) // 64).sum()) if interpolate else 2 * self.tiles


def geometry(case, fused=False, wl=None):
    import torch
    from oracle import ref_torch as ref
    wl = workload(case) if wl is None else wl
    B = case.batch
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, B, dtype=torch.float64)
    p = {g: [{k: v.double() for k, v in d.items()} for d in lst] for g, lst in params(case).items()}
    bx, by = rs.beta(rs.img_X, rs.img_Y, p["lens_mass"])
    s = p["source_light"][0]
    u = ((bx - s["center_x"]) / s["beta"]).numpy().T      # [B, N]
    v = ((by - s["center_y"]) / s["beta"]).numpy().T
    x, y = rs.img_X[:, 0].numpy(), rs.img_Y[:, 0].numpy()
    N = x.size
    assert N == case.n_pixels
    live = (np.abs(u) <= 5.0) & (np.abs(v) <= 5.0)
    du, dv = np.abs(np.abs(u) - 5.0), np.abs(np.abs(v) - 5.0)
    clearance = np.minimum(du, dv).min(axis=1)
    near = (np.abs(np.maximum(np.abs(u), np.abs(v)) - 5.0) < MARGIN).sum(axis=1)
    fu, fv = (u + 5.0) * 599.9, (v + 5.0) * 599.9
    to_node = np.minimum(np.abs(fu - np.round(fu)), np.abs(fv - np.round(fv)))
    node_clearance = np.where(live, to_node, np.inf).min(axis=1)
    is_blocked = blocked(case, fused)
    j, _ = slot_map(N, case.num_pix, is_blocked)
    lv = live[:, j]                                          # [B, tiles, 2, 64]
    c0, c1 = lv[:, :, 0].sum(-1), lv[:, :, 1].sum(-1)
    # the cull test (table mode, GIGALENS_HIP_SHP_CULL unset or 1)
    culled = np.zeros(c0.shape, dtype=bool)
    cull_clear = np.full(B, np.inf)
    rb2_decides = np.zeros(B, dtype=int)
    if case.interpolate and case.env.get("GIGALENS_HIP_SHP_CULL", "1") != "0":
        r_max = np.hypot(x, y).max()
        for b, smp in enumerate(case.samples):
            te, gam, e1, e2, lx, ly = (float(np.float32(t)) for t in smp.lens)
            g1, g2 = (float(np.float32(t)) for t in smp.shear)
            beta_s, cx, cy = (float(np.float32(t)) for t in smp.src)
            c = min(math.hypot(e1, e2), 1.0)
            q = (1 - c) / (1 + c)
            bb = te * math.sqrt(q)
            tm1 = float(np.float32(gam) - np.float32(1) - np.float32(1))
            D = r_max + math.hypot(lx, ly)
            grow = max(D / bb, 1.0) ** (-tm1) if tm1 < 0 else 1.0
            A = (bb / q) * grow + math.hypot(g1, g2) * r_max
            T2 = (1.001 * (5.0 * math.sqrt(2.0) * beta_s + A)) ** 2
            rb2 = 1.002 * (bb / q) ** 2 if tm1 > 0 else 0.0
            d2 = (x - cx) ** 2 + (y - cy) ** 2
            e2_ = (x - lx) ** 2 + (y - ly) ** 2
            far = (d2 > T2) & (e2_ >= rb2)
            culled[b] = far[j].all(axis=(1, 2))
            rb2_decides[b] = int(((d2 > T2)[j].all(axis=(1, 2)) & ~culled[b]).sum())
            cull_clear[b] = min(np.abs(d2 / T2 - 1).min(), np.abs(e2_ / rb2 - 1).min() if rb2 > 0 else np.inf)
    return Geometry(c0, c1, culled, live, clearance, near, cull_clear, node_clearance, rb2_decides, is_blocked)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def square(num_pix, delta_pix, k, row, col, nudge=(0.0, 0.0), **kw):
    """A source behind a near-zero lens (theta_E = 1e-3, no shear) whose live region is the k x k pixel square with first
    pixel (row, col), clipped by the image: centre on the square's centre, 5 beta_s = k / 2 pixels -- the table boundary
    runs half-way between pixel rows and columns, 5 / k in (u, v) from the nearest pixel.  `nudge` (arcsec, a few 1e-5) moves
    the centre off that position: it keeps every live pixel clear of the table's nodes (NODE_MARGIN)."""
    c = (num_pix - 1) / 2
    return Sample(src=(k * delta_pix / 10.0, (col + (k - 1) / 2 - c) * delta_pix + nudge[0],
                       (row + (k - 1) / 2 - c) * delta_pix + nudge[1]), **kw)


def _lens(theta_E, gamma, e1, e2, cx=0.0, cy=0.0):
    return (theta_E, gamma, e1, e2, cx, cy)


# q = (1 - |e|) / (1 + |e|): |e| = 0.25 gives q = 0.6, |e| = 0.01 gives q = 0.98
E06, E098 = (0.2, -0.15), (0.008, 0.006)

CASES = [
    # -- 32 x 32, blocked (nbx = 2): blocks of 8 rows x 16 columns, slot 0 = rows 0-3 of the block, slot 1 = rows 4-7
    Case("shp_cnt32_a", 32, 0.08, 6, roles=("count",), samples=(
        square(32, 0.08, 2, 7, 15),    # 2 x 2 on the corner of four blocks: count 1 four times, (0, 1) above and (1, 0) below
        square(32, 0.08, 9, 1, 2, nudge=(9e-6, 3e-6)),     # 9 x 9: rows 1-7 of block (0, 0) = 7 x 9 = 63 = (27, 36); rows 8-9 below = (18, 0)
        square(32, 0.08, 8, 8, 16, nudge=(3e-5, 1.8e-5)),    # 8 x 8 = all rows of block (1, 1): 64 = (32, 32)
    ), pins=((0, 1), (1, 0), (27, 36), (18, 0), (32, 32))),
    Case("shp_cnt32_b", 32, 0.08, 10, roles=("count",), err=False, lens_light=True, samples=(
        square(32, 0.08, 13, 3, 1, nudge=(9e-6, 3e-6)),    # 13 x 13: rows 3-7 of block (0, 0) = 5 x 13 = 65 = (13, 52); 8 x 13 = (52, 52) below
        square(32, 0.08, 16, 16, 0, nudge=(9e-6, 6e-6)),   # 16 x 16 = blocks (2, 0) and (3, 0) whole: 128 = (64, 64)
        square(32, 0.08, 16, -11, 16), # rows 0-4 of block (0, 1), 16 wide: (64, 16) -- round 2 starts at the slot boundary
    ), pins=((13, 52), (52, 52), (64, 64), (64, 16))),
    # -- ragged, linear: slot 0 = pixels 64 wave .. + 63 of the step, slot 1 = the same 256 further
    Case("shp_cnt30", 30, 0.08, 8, roles=("count",), err=False, samples=(
        square(30, 0.08, 15, -4, 1, nudge=(3e-5, 1.8e-5)),   # (33, 30) = 63 in the first wave-tile
        square(30, 0.08, 15, 3, 0, nudge=(1.5e-5, 1.8e-5)),    # (33, 32) = 65 in wave-tile 3, and live pixels in the partial tile
        square(30, 0.08, 30, -19, 0, nudge=(3e-6, -9e-6)),  # rows 0-10 whole: (64, 64) = 128, then (64, 10)
    ), pins=((33, 30), (33, 32), (64, 64), (64, 10))),
    Case("shp_cnt28", 28, 0.08, 5, roles=("count",), lens_light=True, samples=(
        square(28, 0.08, 1, 18, 8),    # one live pixel, in the partial tile: (1, 0)
        square(28, 0.08, 28, -18, 0, nudge=(6e-6, 2.7e-5)),  # rows 0-9 whole: (64, 24), then (64, 0) = 64
        square(28, 0.08, 12, 9, 4, nudge=(3e-5, 1.8e-5)),    # rows 9-20: wave-tiles with only slot 1 live
    ), pins=((1, 0), (64, 24), (64, 0))),
    # -- a pixel region (the pixel-list path: linear over the list) whose masked pixels are live: the square hangs over the edge
    Case("shp_pixregion32", 32, 0.08, 6, roles=("count",), lens_light=True, pix_region=True, samples=(
        square(32, 0.08, 6, 13, 0),
        square(32, 0.08, 9, 24, 18),
    )),
    # -- realistic lenses whose cull test fires inside the field: theta_E = 0.3, one sample per slope branch of shp_cull_setup
    Case("shp_cull64", 64, 0.08, 6, roles=("cull", "chunk"), samples=(
        Sample(src=(0.05, 0.93, 0.71), lens=_lens(0.3, 2.2, *E06, 0.03, -0.02), shear=(0.02, -0.01)),    # gamma > 2: rb2
        Sample(src=(0.06, -0.41, 0.52), lens=_lens(0.3, 2.0, *E098, -0.02, 0.01), shear=(-0.01, 0.02)),  # gamma = 2, q ~ 1
        Sample(src=(0.05, 0.12, -0.33), lens=_lens(0.3, 1.8, *E06, 0.01, 0.02), shear=(0.01, 0.01)),     # gamma < 2: grow
    )),
    Case("shp_cull32", 32, 0.1, 4, roles=("cull",), err=False, lens_light=True, samples=(
        Sample(src=(0.03, -0.62, -0.48), lens=_lens(0.25, 2.3, *E06, 0.02, 0.03), shear=(0.01, 0.0)),
        Sample(src=(0.03, 0.21, 0.17), lens=_lens(0.2, 1.7, *E06, -0.03, 0.01), shear=(0.0, -0.01)),
    )),
    # -- 96 x 96 (nbx = 6): eighteen whole tiles, a step's four blocks straddle block rows
    Case("shp_blk96", 96, 0.05, 8, roles=("cull", "chunk"), samples=(
        Sample(src=(0.05, 0.44, -0.37), lens=_lens(0.3, 2.1, *E06, 0.02, 0.01), shear=(0.01, -0.02)),
        square(96, 0.05, 20, 30, 70),  # near-zero lens: a 20 x 20 square over blocks (3..6, 4..5), steps 5-9
    )),
    # -- direct mode: every pixel is live, two rounds per wave-tile, no cull
    Case("shp_direct64", 64, 0.08, 6, roles=("chunk",), interpolate=False, err=False, samples=(
        Sample(src=(0.12, 0.21, -0.13), lens=_lens(0.9, 2.1, *E06, 0.02, 0.01), shear=(0.02, -0.01)),
        Sample(src=(0.15, -0.11, 0.08), lens=_lens(0.8, 1.9, 0.05, 0.1, -0.02, 0.03), shear=(-0.01, 0.02)),
    )),
    Case("shp_direct96", 96, 0.05, 4, roles=("chunk",), interpolate=False, lens_light=True, samples=(
        Sample(src=(0.12, 0.11, 0.07), lens=_lens(0.9, 2.05, *E06, 0.01, -0.02), shear=(0.01, 0.02)),
        Sample(src=(0.1, -0.05, 0.12), lens=_lens(1.0, 1.95, 0.1, -0.05, 0.02, 0.02), shear=(0.02, 0.0)),
    )),
]

# -- orders: n_max = 0 (the smallest the front end accepts: one amplitude), 1, 2, 3 -- 1, 3, 6, 10 amplitudes in the zero-padded
# 12 x 12 matrix -- and 10, table and direct, 32 x 32
_ORDER_SAMPLES = (
    Sample(src=(0.11, 0.13, -0.09), lens=_lens(0.8, 2.1, *E06, 0.02, 0.01), shear=(0.02, -0.01)),
    Sample(src=(0.09, -0.07, 0.11), lens=_lens(0.7, 1.9, 0.05, 0.1, -0.02, 0.03), shear=(-0.01, 0.02)),
)
ORDER_CASES = [Case(f"shp_order{n}_{'table' if interp else 'direct'}", 32, 0.08, n, roles=("order",), interpolate=interp,
                    err=(n % 2 == 0), samples=_ORDER_SAMPLES)
               for n in (0, 1, 2, 3, 10) for interp in (True, False)]

# -- the fused linear solve (gl_shp_normal_kernel, table mode): Dl = 3, 15, 21, 55 channels put the skipped pixels' sum of
# (obs w)^2 into lane o = Dl & 3 = 3, 3, 1, 3 of its quad (Dl = 15: the observation column is the last channel of a tile row);
# 16, 48 and 80 px are blocked with N % 512 != 0: blocks past the image are masked out
_LSQ_LENS = dict(lens=_lens(0.5, 2.1, *E06, 0.02, 0.01), shear=(0.02, -0.01))
LSTSQ_CASES = [
    Case("shp_lsq_n1_32", 32, 0.08, 1, roles=("lstsq",), lstsq=True, samples=(
        Sample(src=(0.12, 0.31, -0.17), **_LSQ_LENS), Sample(src=(0.1, -0.22, 0.14), lens=_lens(0.5, 1.9, 0.05, 0.1)))),
    Case("shp_lsq_n4_48", 48, 0.08, 4, roles=("lstsq",), lstsq=True, samples=(
        Sample(src=(0.12, 0.31, -0.17), **_LSQ_LENS), Sample(src=(0.1, -0.22, 0.14), lens=_lens(0.5, 1.9, 0.05, 0.1)))),
    Case("shp_lsq_n9_80", 80, 0.05, 9, roles=("lstsq",), lstsq=True, samples=(
        Sample(src=(0.12, 0.3167, -0.172), **_LSQ_LENS), Sample(src=(0.1, -0.223, 0.141), lens=_lens(0.5, 1.9, 0.05, 0.1)))),
    Case("shp_lsq_n5_16", 16, 0.12, 5, roles=("lstsq",), lstsq=True, samples=(
        Sample(src=(0.2, 0.11, -0.07), **_LSQ_LENS), Sample(src=(0.22, -0.12, 0.14), lens=_lens(0.5, 1.9, 0.05, 0.1)))),
    # a compact source: most wave-tiles hold no live pixel and add only their sum of (obs w)^2
    Case("shp_lsq_compact64", 64, 0.08, 4, roles=("lstsq",), lstsq=True, samples=(
        square(64, 0.08, 7, 20, 37, nudge=(-1.2e-5, -1.2e-5)), square(64, 0.08, 9, 41, 9))),
    # count pinned at 64 = (32, 32) and at 65 = (13, 52) in one wave-tile (the squares of shp_cnt32_a / _b)
    Case("shp_lsq_pinned32", 32, 0.08, 4, roles=("lstsq", "count"), lstsq=True, samples=(
        square(32, 0.08, 8, 8, 16, nudge=(3e-5, 1.8e-5)), square(32, 0.08, 13, 3, 1, nudge=(9e-6, 3e-6))), pins=((32, 32), (13, 52))),
]

ALL_CASES = CASES + ORDER_CASES + LSTSQ_CASES
BY_ID = {c.id: c for c in ALL_CASES}


def variant(case, suffix, **env):
    """The same case under other GIGALENS_HIP_* knobs."""
    from dataclasses import replace
    return replace(case, id=f"{case.id}_{suffix}", env={**case.env, **{k: str(v) for k, v in env.items()}})


# one workgroup per sample (GIGALENS_HIP_LSTSQ_WGS=1): every 512-pixel tile of the image in one trip loop, the waves swapping
# blocks from trip to trip, each wave-tile's list over the stale entries of the one before
LSTSQ_ONE_WG = [variant(BY_ID[cid], "onewg", GIGALENS_HIP_LSTSQ_WGS=1) for cid in ("shp_lsq_n4_48", "shp_lsq_n9_80", "shp_lsq_compact64")]
