"""Point images in the pixel likelihood (LensSimulator.point_images, fit_point_images, point_image_log_like_and_grad,
model.PointImageProbModel; csrc/gl_ptimg.hip.h) restated from the definition in torch, float64 by default, and the cases the tests
run.  No GPU; the product is imported only for its model classes (the profiles a RefSimulator is built from).

The unit point image D(x, y) [H, W] is written here in SPLAT form, step by step:
    (u, v) = supersample * wcs.angle2pix(x, y): the position in supersampled pixel coordinates, u along the columns
    splat      S[floor(v) - 1 + j, floor(u) - 1 + i] += wv[j] wu[i], i, j = 0..3, Keys' weights (a = -1/2) in the Horner form of
               glp::interp_weights at t = u - floor(u), v - floor(v); taps outside the frame are dropped
    convolve   flip the PSF, cross-correlate with SAME padding ((k - 1) // 2 before, k // 2 after), as post_cases.post_fwd_f64
    pool       ss x ss SUM pool, no det T
The kernels gather instead (a cubic interpolation of the zero-extended PSF per sub-pixel, factored weights) and never form S: the
two are coded independently.

The fit, per sample: m = E + sum_j a_j D_j, w = 1 / err^2 on the used pixels U; N = sum_U w D_j D_k, r = sum_U w D_j (obs - E),
a = N^-1 r, chi2 = sum_U w (obs - m)^2, log_like = -chi2 / 2 - sum_U log(2 pi err^2) / 2.  `profiled_log_like` keeps the solve
inside the autograd graph: its gradient is the total derivative, which the product's envelope-theorem gradient must equal."""
import math
import zlib

import numpy as np
import torch

from oracle import ref_torch as ref
from tests import post_cases as PO

F64, F32 = torch.float64, torch.float32
U32 = 2.0 ** -24
DELTA_PIX = 0.0625  # a power of two: pixel centres and half-pixel offsets are exact float32 numbers on the axis-aligned cameras


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def gauss_psf(shape, sigma, skew=0.0):
    """Gaussian-like, normalised, float32; ``skew`` makes it asymmetric under both flips (pins the flip of the convolution)"""
    kh, kw = shape
    yy, xx = np.meshgrid(np.arange(kh) - (kh - 1) / 2, np.arange(kw) - (kw - 1) / 2, indexing="ij")
    k = np.exp(-0.5 * (xx ** 2 + yy ** 2) / sigma ** 2) * (1.0 + skew * (0.5 * xx + 0.3 * yy) / max(kh, kw))
    return (k / k.sum()).astype(np.float32)


def _hole(n):
    r = np.ones(n if isinstance(n, tuple) else (n, n), dtype=np.float64)
    r[4:6, 5:7] = 0.0
    return r


# name -> (num_pix, supersample, PSF on the supersampled grid or None, transform_pix2angle or None, pix_region or None, mask or None)
def _cameras():
    rot = DELTA_PIX * np.array([[0.96, -0.31], [0.22, 1.04]])  # rotated and not symmetric: T against T^T
    mask = np.ones((12, 12), dtype=bool)
    mask[:6, :6] = False  # a block large enough to hold the whole footprint of an image
    return {
        "plain9": (9, 1, None, None, None, None),                                   # no PSF: the [[1]] kernel
        "ss2_psf5": ((10, 12), 2, gauss_psf((5, 5), 1.3, skew=0.8), None, None, None),  # not square; asymmetric PSF
        "ss3_psf7": (8, 3, gauss_psf((7, 7), 1.6), None, None, None),
        "rot_even": (11, 1, gauss_psf((4, 3), 1.0, skew=0.5), rot, _hole(11), None),   # even-sided kernel, hole in pix_region
        "ss2_psf3_mask": (12, 2, gauss_psf((3, 3), 0.9), None, None, mask),
        "plain12_mask": (12, 1, None, None, None, mask),
    }


def camera(name):
    """``dict(cfg, psf, mask, ss, H, W, x0, M)``: ``(u, v) = M (x - x0[0], y - x0[1])`` in float64"""
    from gigalens_amd.simulator import SimulatorConfig
    num_pix, ss, psf, T, region, mask = _cameras()[name]
    cfg = SimulatorConfig(delta_pix=DELTA_PIX, num_pix=num_pix, supersample=ss, transform_pix2angle=T, pix_region=region)
    wcs = ref.LensWCS(n=num_pix, supersample=ss, transform_pix2angle=T, pix_scale=DELTA_PIX)
    # pix2angle applies (T / ss)^T to (column, row) and adds radec_at_xy_0: its inverse
    M = np.linalg.inv(wcs.transform_pix2angle.T)
    return dict(name=name, cfg=cfg, psf=psf, mask=mask, ss=ss, H=wcs.n_x, W=wcs.n_y, x0=np.asarray(wcs.radec_at_xy_0, dtype=np.float64),
                M=M, region=region)


def uv_of(cam, x, y):
    """arcsec -> supersampled pixel coordinates, torch (keeps dtype and graph)"""
    dx, dy = x - float(cam["x0"][0]), y - float(cam["x0"][1])
    M = cam["M"]
    return float(M[0, 0]) * dx + float(M[0, 1]) * dy, float(M[1, 0]) * dx + float(M[1, 1]) * dy


def xy_of(cam, u, v):
    """supersampled pixel coordinates -> arcsec, float64 numpy"""
    Minv = np.linalg.inv(cam["M"])
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (0 x inf: a position that is not finite stays not finite)
        return Minv[0, 0] * u + Minv[0, 1] * v + cam["x0"][0], Minv[1, 0] * u + Minv[1, 1] * v + cam["x0"][1]


def used_pixels(cam):
    used = np.ones((cam["H"], cam["W"]), dtype=bool) if cam["region"] is None else np.asarray(cam["region"]) != 0
    return used & cam["mask"] if cam["mask"] is not None else used


# ---- the unit point image, splat form ---------------------------------------------------------------------------------------
def keys_weights(t, deriv=False):
    """the four weights of one axis, taps floor - 1 .. floor + 2 (glp::interp_weights, linear = false), or their derivatives"""
    if deriv:
        return [(-1.5 * t + 2.0) * t - 0.5, (4.5 * t - 5.0) * t, (-4.5 * t + 4.0) * t + 0.5, (1.5 * t - 1.0) * t]
    return [((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * t * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * t * t]


def unit_image_uv(cam, u, v, mode="value"):
    """D [H, W] of one position given in supersampled pixel coordinates (0-d tensors).  ``mode``: "value"; "abs" (every weight and
    PSF tap by its absolute value: the sum of |terms| of the error bound); "du" / "dv" (the derivative in u / v)."""
    ss, H, W = cam["ss"], cam["H"], cam["W"]
    Hs, Ws = H * ss, W * ss
    dtype = u.dtype
    psf = np.ones((1, 1), dtype=np.float32) if cam["psf"] is None else cam["psf"]
    u0, v0 = float(u.detach()), float(v.detach())
    if not (math.isfinite(u0) and math.isfinite(v0)) or abs(u0) > 1e6 or abs(v0) > 1e6:
        return torch.zeros((H, W), dtype=dtype) + 0.0 * torch.nan_to_num(u + v, nan=0.0, posinf=0.0, neginf=0.0)
    fu, fv = math.floor(u0), math.floor(v0)
    wu = keys_weights(u - fu, deriv=mode == "du")
    wv = keys_weights(v - fv, deriv=mode == "dv")
    S = torch.zeros((Hs, Ws), dtype=dtype)
    for j in range(4):
        for i in range(4):
            r, c = fv - 1 + j, fu - 1 + i
            if 0 <= r < Hs and 0 <= c < Ws:
                val = wv[j] * wu[i]
                S = S.index_put((torch.tensor(r), torch.tensor(c)), val.abs() if mode == "abs" else val, accumulate=True)
    k = torch.as_tensor(np.ascontiguousarray(psf[::-1, ::-1].astype(np.float64))).to(dtype)  # flip ...
    if mode == "abs":
        k = k.abs()
    kh, kw = k.shape
    Sp = torch.nn.functional.pad(S, ((kw - 1) // 2, kw // 2, (kh - 1) // 2, kh // 2))
    conv = torch.nn.functional.conv2d(Sp[None, None], k[None, None])[0, 0]  # ... and cross-correlate (conv2d is one)
    return conv.reshape(H, ss, W, ss).sum(dim=(1, 3))


def unit_images(cam, x, y, mode="value"):
    """[B, J] positions in arcsec (torch) -> D [B, J, H, W]"""
    u, v = uv_of(cam, x, y)
    B, J = x.shape
    return torch.stack([torch.stack([unit_image_uv(cam, u[b, j], v[b, j], mode) for j in range(J)]) for b in range(B)])


# ---- the fit ----------------------------------------------------------------------------------------------------------------
def _as_batch(a, B, dtype):
    t = torch.as_tensor(np.asarray(a)).to(dtype) if not torch.is_tensor(a) else a.to(dtype)
    return t.expand(B, *t.shape[-2:]) if t.dim() == 3 else t[None].expand(B, *t.shape)


def fit(cam, D, E, obs, err, order=None):
    """The linear fit per sample.  ``D`` [B, J, H, W], ``E`` [B, H, W]; ``obs``, ``err`` [H, W] or [B, H, W].  ``order``: a permutation
    of the used pixels -- the pixel sums are then accumulated one term after the other in that order (what the float32 runs vary).
    Returns a dict of tensors: amplitudes [B, J], model [B, H, W], chi2, log_like [B], ok [B] (bool), cond [B]."""
    dtype = D.dtype
    B, J = D.shape[:2]
    used = torch.as_tensor(used_pixels(cam)).reshape(-1)
    idx = torch.nonzero(used)[:, 0]
    if order is not None:
        idx = idx[torch.as_tensor(order)]
    Du = D.reshape(B, J, -1)[:, :, idx]
    obs_u, err_u = _as_batch(obs, B, dtype).reshape(B, -1)[:, idx], _as_batch(err, B, dtype).reshape(B, -1)[:, idx]
    y = obs_u - E.reshape(B, -1)[:, idx]
    w = 1.0 / (err_u * err_u)
    # (numpy's accumulate adds one term after the other in the array's own type; torch.cumsum accumulates float32 in float64)
    total = ((lambda t: torch.as_tensor(np.cumsum(t.detach().numpy(), axis=-1, dtype=t.detach().numpy().dtype)[..., -1]))
             if order is not None else (lambda t: t.sum(dim=-1)))
    N = total(w[:, None, None, :] * Du[:, :, None, :] * Du[:, None, :, :])
    r = total(w[:, None, :] * Du * y[:, None, :])
    amps, oks, conds = [], [], []
    for b in range(B):
        ev = torch.linalg.eigvalsh(N[b].detach().double())
        ok = bool(torch.isfinite(ev).all()) and float(ev[0]) > 1e-6 * float(ev[-1])
        oks.append(ok)
        conds.append(float(ev[-1] / ev[0]) if ok else float("inf"))
        amps.append(torch.linalg.solve(N[b], r[b]) if ok else torch.full((J,), float("nan"), dtype=dtype))
    a = torch.stack(amps)
    model = E + (a[:, :, None, None] * D).sum(dim=1)
    res = obs_u - model.reshape(B, -1)[:, idx]
    chi2 = total(w * res * res)
    noise = total(torch.log(2.0 * math.pi * err_u * err_u))
    return {"amplitudes": a, "model_image": model, "chi2": chi2, "log_like": -0.5 * chi2 - 0.5 * noise,
            "ok": torch.as_tensor(oks), "cond": torch.as_tensor(conds)}


def tie(beta_x, beta_y, sigma):
    """[B, J] source-plane positions -> -1/2 sum_j |beta_j - mean beta|^2 / sigma^2 - (J - 1) log(2 pi sigma^2), [B]"""
    J = beta_x.shape[1]
    dx, dy = beta_x - beta_x.mean(dim=1, keepdim=True), beta_y - beta_y.mean(dim=1, keepdim=True)
    return -0.5 * (dx * dx + dy * dy).sum(dim=1) / sigma ** 2 - (J - 1) * math.log(2.0 * math.pi * sigma ** 2)


# ---- extended model ---------------------------------------------------------------------------------------------------------
def phys_model():
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    return PhysicalModel([SIE(), Shear()], [], [Sersic()])


def lens_params(B, key):
    """SIE + Shear | Sersic source on a frame about 0.6 arcsec wide, [B] float32 arrays per parameter"""
    r = _rng("params", key)
    f = lambda lo, hi: r.uniform(lo, hi, size=B).astype(np.float32)
    return {"lens_mass": [{"theta_E": f(0.17, 0.2), "e1": f(-0.1, 0.1), "e2": f(-0.1, 0.1), "center_x": f(-0.01, 0.01),
                           "center_y": f(-0.01, 0.01)}, {"gamma1": f(-0.03, 0.03), "gamma2": f(-0.03, 0.03)}],
            "source_light": [{"R_sersic": f(0.05, 0.07), "n_sersic": f(1.0, 2.0), "center_x": f(-0.02, 0.02), "center_y": f(-0.02, 0.02),
                              "Ie": f(8.0, 12.0)}]}


GROUPS = ("lens_mass", "source_light")


def packed_of(params):
    """the nested dict as [B, P] float64 in the layout's order (lens_mass then source_light, each profile's `params` order)"""
    pm = phys_model()
    cols = []
    for g, profs in zip(GROUPS, (pm.lenses, pm.source_light)):
        for p, d in zip(profs, params[g]):
            cols += [np.asarray(d[n], dtype=np.float64) for n in p._native_params()]
    return torch.as_tensor(np.stack(cols, axis=1))


def struct_of(packed):
    pm = phys_model()
    k, out = 0, {}
    for g, profs in zip(GROUPS, (pm.lenses, pm.source_light)):
        out[g] = []
        for p in profs:
            names = p._native_params()
            out[g].append({n: packed[:, k + i] for i, n in enumerate(names)})
            k += len(names)
    return out


def extended(cam, packed):
    """E [B, H, W] of the packed rows, in their dtype (oracle.ref_torch.RefSimulator, as smoke() uses it)"""
    B = packed.shape[0]
    rs = ref.RefSimulator(phys_model(), cam["cfg"], B, dtype=packed.dtype, supersampled_kernel=cam["psf"])
    return rs.simulate(struct_of(packed)).reshape(B, cam["H"], cam["W"])


def profiled_log_like(cam, packed, x, y, obs, err):
    """log_like [B] with the solve inside the graph (float64 autograd: the total derivative)"""
    return fit(cam, unit_images(cam, x, y), extended(cam, packed), obs, err)["log_like"]


# ---- positions of the render test -------------------------------------------------------------------------------------------
def render_positions(cam):
    """(u, v) in supersampled pixel coordinates, one list per camera: integer nodes, generic fractions, t = 0 and t just below 1,
    both sides of every frame edge, far outside, not finite"""
    Hs, Ws = cam["H"] * cam["ss"], cam["W"] * cam["ss"]
    kh, kw = (1, 1) if cam["psf"] is None else cam["psf"].shape
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    return [
        (Ws // 2, Hs // 2), (3.0, 5.0),                                  # integer nodes
        (Ws / 2 + 0.37, Hs / 2 - 0.81), (4.25, 6.5), (7.6180339, 3.1415926),  # generic
        (5.0, 4.0 + below), (4.0 + below, 6.0), (6.0, 2.5),                 # t = 0 on one axis, t just below 1 on the other
        (0.3, Hs / 2 + 0.2), (1.9, 1.2), (Ws - 1.4, Hs - 2.8), (Ws / 2 - 0.4, Hs - 1.05),  # within 2 nodes of an edge, inside
        (-0.6, Hs / 2 + 0.3), (Ws - 0.3, 4.4), (5.7, -1.2), (3.3, Hs + 0.45), (-1.5, -0.7),   # just outside: part of the footprint
        (-(kw // 2) - 2.5, 3.0), (Ws + kw + 40.0, 2.0), (4.0, -(kh + 50.0)),  # beyond the footprint, far outside
        (float("nan"), 3.0), (2.0, float("inf")),                          # not finite
    ]


def render_case(cam_name, J, B, first=0):
    """``dict(cam, x, y, amp)`` with [B, J] float32 arrays: the positions of `render_positions` from number ``first`` on, cycled
    through the batch; on the axis-aligned cameras with supersample 1 and 2 they are exact in float32 (DELTA_PIX is a power of two)"""
    cam = camera(cam_name)
    pos = render_positions(cam)
    uv = np.array([pos[(first + k) % len(pos)] for k in range(B * J)], dtype=np.float64).reshape(B, J, 2)
    x, y = xy_of(cam, uv[..., 0], uv[..., 1])
    r = _rng("amp", cam_name, J, B)
    amp = (r.uniform(0.5, 2.0, size=(B, J)) * r.choice([-1.0, 1.0], size=(B, J), p=[0.2, 0.8])).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return dict(cam=cam, x=x.astype(np.float32), y=y.astype(np.float32), amp=amp, uv=uv)


N_RENDER_POSITIONS = 22
# camera, J, B, first position: every camera but one walks the whole list (B J >= 22, or from the frame edges on)
RENDER_CASES = [("plain9", 1, 65, 0), ("ss2_psf5", 8, 3, 0), ("ss3_psf7", 2, 1, 2), ("ss3_psf7", 4, 3, 10), ("rot_even", 4, 65, 0),
                ("ss2_psf3_mask", 2, 3, 8)]


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def render_bound(c):
    """Per pixel [B, H, W]: what a float32 evaluation of the definition may differ from float64 by, nothing measured on the kernels.
    Per image gamma_n sum |terms| with n = 16 ss^2 + 2 (the 16 ss^2 products of a pixel, any order, plus the rounding of the two
    weights; Higham section 3.1, as tests/post_cases.py) and the rounding of (u, v) to float32: 4 ulp of the larger of |u|, |v|
    times |dD/du| + |dD/dv|; then the J products and additions of the amplitudes."""
    cam, ss = c["cam"], c["cam"]["ss"]
    x, y = torch.as_tensor(c["x"]).double(), torch.as_tensor(c["y"]).double()
    a = np.abs(c["amp"].astype(np.float64))[:, :, None, None]
    J = c["x"].shape[1]
    D_abs = unit_images(cam, x, y, "abs").numpy()
    slope = np.abs(unit_images(cam, x, y, "du").numpy()) + np.abs(unit_images(cam, x, y, "dv").numpy())
    u, v = (t.numpy() for t in uv_of(cam, x, y))
    with np.errstate(invalid="ignore"):
        big = np.where(np.isfinite(u) & np.isfinite(v), np.maximum(np.abs(u), np.abs(v)), 0.0)
    ulp = np.spacing(big.astype(np.float32)).astype(np.float64)[:, :, None, None]
    per_image = gamma(16 * ss * ss + 2) * D_abs + 4.0 * ulp * slope
    return (a * per_image).sum(axis=1) + gamma(J + 1) * (a * D_abs).sum(axis=1)


# ---- cases of the fit -------------------------------------------------------------------------------------------------------
def _ring(cam, J, B, key, radius, jitter):
    """J images per sample on a ring around the frame centre, in supersampled pixel coordinates"""
    r = _rng("ring", key)
    Hs, Ws = cam["H"] * cam["ss"], cam["W"] * cam["ss"]
    ang = 2 * np.pi * (np.arange(J)[None, :] + r.uniform(0, 1, size=(B, 1))) / J
    rad = radius * cam["ss"] * (1.0 + 0.15 * r.uniform(-1, 1, size=(B, J)))
    u = (Ws - 1) / 2 + rad * np.cos(ang) + jitter * r.uniform(-1, 1, size=(B, J))
    v = (Hs - 1) / 2 + rad * np.sin(ang) + jitter * r.uniform(-1, 1, size=(B, J))
    return u, v


def _fit_positions(name, cam):
    ss = cam["ss"]
    if name == "quad":          # four images, every pair at least two final pixels apart
        return _ring(cam, 4, 3, name, 2.6, 0.3)
    if name == "overlap":       # two images 1.0 and 1.5 final pixels apart (overlapping boxes), and a wide pair
        u = np.array([[9.3, 9.3 + 1.0 * ss], [8.1, 8.1 + 1.5 * ss * 0.8], [6.2, 15.7]])
        v = np.array([[11.6, 11.6], [10.4, 10.4 + 1.5 * ss * 0.6], [13.3, 7.9]])
        return u, v
    if name == "single":
        return np.array([[11.3]]), np.array([[12.8]])
    if name == "octet":         # eight images on a ring, 65 samples
        return _ring(cam, 8, 65, name, 3.3, 0.2)
    if name == "coincident":    # sample 1: two images at one position
        u = np.array([[3.3, 6.8], [4.6, 4.6], [2.7, 5.9]])
        v = np.array([[4.1, 3.2], [4.2, 4.2], [5.5, 2.4]])
        return u, v
    if name == "masked":        # sample 1: the first image's 4 x 4 footprint lies on masked pixels alone
        u = np.array([[8.3, 2.6], [2.4, 8.7], [9.1, 7.8]])
        v = np.array([[2.5, 8.2], [2.6, 8.4], [3.3, 9.0]])
        return u, v
    raise KeyError(name)


FIT_CASES = {"quad": "ss2_psf5", "overlap": "ss2_psf5", "single": "ss3_psf7", "octet": "rot_even", "coincident": "plain9",
             "masked": "plain12_mask"}
SOLVABLE = ("quad", "overlap", "single", "octet")
SINGULAR = {"coincident": 1, "masked": 1}  # case -> the sample that must come back with ok = False
COND_MAX = 100.0
_FIT = {}


def fit_case(name):
    """``dict(cam, params, packed, x, y, obs, err, B, J)``: float32 inputs as the product receives them (numpy), built once.  The
    data are the float64 model at displaced positions and perturbed lens parameters plus noise, so the residual is not noise alone."""
    if name in _FIT:
        return _FIT[name]
    cam = camera(FIT_CASES[name])
    u, v = _fit_positions(name, cam)
    B, J = u.shape
    x, y = xy_of(cam, u, v)
    x, y = x.astype(np.float32), y.astype(np.float32)
    params = lens_params(B, name)
    packed = packed_of(params)
    r = _rng("data", name)
    with torch.no_grad():
        truth = packed * torch.as_tensor(1.0 + 0.01 * r.normal(size=tuple(packed.shape)))
        xt = torch.as_tensor(x.astype(np.float64) + 0.1 * DELTA_PIX / cam["ss"] * r.normal(size=x.shape))
        yt = torch.as_tensor(y.astype(np.float64) + 0.1 * DELTA_PIX / cam["ss"] * r.normal(size=y.shape))
        flux = torch.as_tensor(r.uniform(30.0, 60.0, size=(B, J)))
        clean = extended(cam, truth) + (flux[:, :, None, None] * unit_images(cam, xt, yt)).sum(dim=1)
    H, W = cam["H"], cam["W"]
    err = (0.3 * (1.0 + 0.2 * r.uniform(-1, 1, size=(H, W)))).astype(np.float32)
    obs = (clean.numpy() + err[None] * r.normal(size=(B, H, W))).astype(np.float32)
    _FIT[name] = dict(name=name, cam=cam, params=params, packed=packed, x=x, y=y, obs=obs, err=err, B=B, J=J)
    return _FIT[name]


_REF = {}


def fit_reference(name, dtype=F64):
    """The fit of a case in ``dtype`` with the gradient of the profiled log_like by autograd THROUGH the solve: ``dict`` of numpy arrays
    (the entries of `fit`, plus grad [B, P], grad_x, grad_y [B, J]); computed once and shared.  float64: the reference; float32: the
    restatement's own float32 run, the yardstick of the gradient gate."""
    if (name, dtype) in _REF:
        return _REF[(name, dtype)]
    c = fit_case(name)
    cam = c["cam"]
    packed = c["packed"].to(dtype).clone().requires_grad_(True)
    x = torch.as_tensor(c["x"]).to(dtype).requires_grad_(True)
    y = torch.as_tensor(c["y"]).to(dtype).requires_grad_(True)
    obs, err = torch.as_tensor(c["obs"]).to(dtype), torch.as_tensor(c["err"]).to(dtype)
    D, E = unit_images(cam, x, y), extended(cam, packed)
    out = fit(cam, D, E, obs, err)
    good = out["ok"]
    g, gx, gy = torch.autograd.grad(out["log_like"][good].sum(), [packed, x, y], allow_unused=True) if bool(good.any()) else (None,) * 3
    res = {k: v.detach().numpy() for k, v in out.items()}
    res["extended_image"] = E.detach().numpy()
    res["D"] = D.detach().numpy()
    zero = lambda t, like: np.zeros(tuple(like.shape)) if t is None else t.numpy()
    res["grad"], res["grad_x"], res["grad_y"] = zero(g, packed), zero(gx, x), zero(gy, y)
    _REF[(name, dtype)] = res
    return res


def envelope_gradient(name):
    """The gradient the product forms, restated in float64: the cotangent w (obs - m) on U pushed through E by autograd (what the
    render's VJP does) and a_j sum_U w (obs - m) dD_j/d(x_j, y_j) with the amplitudes held fixed.  -> grad, grad_x, grad_y"""
    c, o = fit_case(name), fit_reference(name)
    cam = c["cam"]
    B = c["B"]
    used = torch.as_tensor(used_pixels(cam))
    w = torch.where(used, 1.0 / _as_batch(c["err"], B, F64) ** 2, torch.zeros((), dtype=F64))
    good = torch.as_tensor(o["ok"])
    cot = torch.where(good[:, None, None], w * (_as_batch(c["obs"], B, F64) - torch.as_tensor(np.nan_to_num(o["model_image"]))), torch.zeros((), dtype=F64))
    packed = c["packed"].clone().requires_grad_(True)
    (g,) = torch.autograd.grad((extended(cam, packed) * cot).sum(), packed)
    x = torch.as_tensor(c["x"]).double().requires_grad_(True)
    y = torch.as_tensor(c["y"]).double().requires_grad_(True)
    a = torch.as_tensor(np.nan_to_num(o["amplitudes"]))
    gx, gy = torch.autograd.grad(((a[:, :, None, None] * unit_images(cam, x, y)).sum(dim=1) * cot).sum(), [x, y])
    return g.numpy(), gx.numpy(), gy.numpy()


def float32_fit(name, n_orders=3):
    """The restatement in float32 on the CPU with the pixel sums in ``n_orders`` different orders (as stored, reversed, shuffled):
    a list of result dicts (numpy)."""
    c = fit_case(name)
    cam = c["cam"]
    n_used = int(used_pixels(cam).sum())
    orders = [np.arange(n_used), np.arange(n_used)[::-1].copy(), _rng("order", name).permutation(n_used)][:n_orders]
    x, y = torch.as_tensor(c["x"]), torch.as_tensor(c["y"])
    with torch.no_grad():
        D, E = unit_images(cam, x, y), extended(cam, c["packed"].float())
        return [{k: v.numpy() for k, v in fit(cam, D, E, torch.as_tensor(c["obs"]), torch.as_tensor(c["err"]), order=o).items()}
                for o in orders]


def amplitude_error(a, a_ref):
    """[B]: the largest amplitude error of a sample relative to its largest |amplitude|"""
    a, a_ref = np.asarray(a, dtype=np.float64), np.asarray(a_ref, dtype=np.float64)
    return np.abs(a - a_ref).max(axis=1) / np.abs(a_ref).max(axis=1)


AMP_RTOL_CAP = 1e-4
_FLOOR = {}


def float32_amplitude_floor(name):
    """The float32 floor of a case's amplitudes: the worst `amplitude_error` against float64 of the restatement's float32 runs, over
    the three summation orders and every sample.  Computed once per case."""
    if name not in _FLOOR:
        ref64 = fit_reference(name)["amplitudes"]
        _FLOOR[name] = max(float(amplitude_error(f["amplitudes"], ref64).max()) for f in float32_fit(name))
    return _FLOOR[name]
