"""Dense restatement of the pixelated source reconstruction (LensSimulator.reconstruct_source, csrc/gl_pixsrc.hip.h) and the cases
of its tests (tests/test_pixsrc_host.py pins the restatement without a GPU, tests/test_gpu_pixsrc.py runs the kernels against it).

Everything is written from the definitions of DESIGN.md section 7, "Pixelated source", with dense matrices and no stencil, tile or
workspace: ``L`` explicitly, ``F`` by the oracle's PSF + pooling (``oracle.ref_torch.psf_pool``, the post-processing
tests/interp_cases.py composes) applied to every column, ``R`` by Kronecker products, the solve by ``numpy.linalg.cholesky``.  Every
function takes ``dtype``: float64 is the reference, the same code in float32 on the CPU is the yardstick of the value gates."""
import math

import numpy as np
import torch

F64 = torch.float64
REGS = ("identity", "gradient", "curvature")


def _np_dtype(dtype):
    return np.float64 if dtype == F64 else np.float32


def hat(t):
    return torch.clamp(1 - t.abs(), min=0)


def mapping(beta_x, beta_y, n_src, pitch, cx, cy):
    """``L [Q, S]`` of one sample, in the dtype of ``beta_x``: ``L[q, (j, i)] = hat(v_q - j) hat(u_q - i)``; a ``beta`` that is not
    finite or fails the range test of gl_interp.h (``-2 <= u <= nx + 1``, ``-2 <= v <= ny + 1``) has a row of exact zeros."""
    ny, nx = n_src
    dt = beta_x.dtype
    pitch, cx, cy = (torch.as_tensor(float(v), dtype=dt) for v in (pitch, cx, cy))
    u = (beta_x - cx) / pitch + (nx - 1) / 2
    v = (beta_y - cy) / pitch + (ny - 1) / 2
    ok = (u >= -2) & (u <= nx + 1) & (v >= -2) & (v <= ny + 1)
    u, v = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    wu = hat(u[:, None] - torch.arange(nx, dtype=dt))
    wv = hat(v[:, None] - torch.arange(ny, dtype=dt))
    L = (wv[:, :, None] * wu[:, None, :]).reshape(-1, ny * nx)
    return torch.where(ok[:, None], L, torch.zeros_like(L))


def tridiag(n, dtype=np.float64):
    return (2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)).astype(dtype)


def reg_matrix(regularization, n_src, dtype=np.float64):
    """Dense ``R``: identity, ``I_y (x) T_x + T_y (x) I_x`` or ``I_y (x) T_x^2 + T_y^2 (x) I_x`` (node (j, i) at index ``j nx + i``)."""
    ny, nx = n_src
    if regularization == "identity":
        return np.eye(ny * nx, dtype=dtype)
    tx, ty = tridiag(nx), tridiag(ny)
    if regularization == "curvature":
        tx, ty = tx @ tx, ty @ ty
    elif regularization != "gradient":
        raise KeyError(regularization)
    return (np.kron(np.eye(ny), tx) + np.kron(ty, np.eye(nx))).astype(dtype)


def frame_beta(rs, lens_params, deflection_scale=1.0):
    """``beta_x, beta_y [Hs Ws, bs]`` on the whole supersampled frame; NaN outside ``pix_region`` (not rendered by the simulator)."""
    bx, by = rs.beta(rs.img_X, rs.img_Y, lens_params)
    c = float(deflection_scale)
    if c != 1.0:
        bx, by = rs.img_X + c * (bx - rs.img_X), rs.img_Y + c * (by - rs.img_Y)
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    idx = torch.from_numpy(rs.region[:, 0] * Ws + rs.region[:, 1])
    fx = torch.full((Hs * Ws, rs.bs), float("nan"), dtype=rs.dtype)
    fy = fx.clone()
    fx[idx], fy[idx] = bx, by
    return fx, fy


def post(rs, planes):
    """``conversion_factor Pool PSF`` on planes ``[K, Hs, Ws]`` -> ``[K, H, W]`` (NaN -> 0 is not needed: ``L`` has no NaN)."""
    from oracle import ref_torch as ref
    return ref.psf_pool(planes[:, None], rs.flat_kernel, rs.supersample)[:, 0] * rs.conversion_factor


def operator(rs, L):
    """``F [H W, S]`` on every pixel of the image (the caller restricts it to the used ones)."""
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    return post(rs, L.t().reshape(-1, Hs, Ws)).reshape(L.shape[1], -1).t()


def lens_light_image(rs, params):
    """The lens light alone as ``simulate`` renders it, ``[bs, H, W]`` (zeros without a lens light)."""
    from oracle import ref_torch as ref
    pm = rs.phys_model
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    img = torch.zeros((Hs, Ws, rs.bs), dtype=rs.dtype)
    rr, cc = torch.from_numpy(rs.region[:, 0]), torch.from_numpy(rs.region[:, 1])
    for lm, p, c in zip(pm.lens_light, params.get("lens_light", []), rs._consts("lens_light_constants", len(pm.lens_light))):
        img = img.index_put((rr, cc), ref.light_eval(lm, rs.img_X, rs.img_Y, **p, **c), accumulate=True)
    img = torch.where(torch.isnan(img), torch.zeros_like(img), img)
    return post(rs, img.permute(2, 0, 1))


def log_det_reg(regularization, n_src):
    """``log det R`` by a dense ``slogdet`` in float64."""
    sign, val = np.linalg.slogdet(reg_matrix(regularization, n_src))
    assert sign > 0
    return float(val)


def used_pixels(rs, mask):
    used = rs.img_region.numpy() != 0
    if mask is not None:
        used = used & np.asarray(mask, dtype=bool)
    return np.flatnonzero(used.reshape(-1))


def reconstruct_from_rays(rs, fx, fy, lens_light, pix, obs_used, sig_used, *, n_src, pitch, center, regularization, strength,
                          dtype=F64, return_parts=False):
    """The restatement from the rays on: ``rs`` supplies the frame, the supersampling, the PSF and the flux scale only.  ``fx, fy``
    ``[Hs Ws, B]`` (source-plane positions on the supersampled frame), ``lens_light`` ``[B, H W]`` or None, ``pix`` ``[n_used]``,
    ``obs_used``, ``sig_used`` ``[B, n_used]`` (so they may differ per sample); ``pitch``, ``center``: scalars or ``[B]``; ``strength``:
    ``[B]`` or ``[B, L]``.  Every input is taken as the float32 values the library receives and converted to ``dtype``.  Returns as
    ``reconstruct`` does."""
    nd = _np_dtype(dtype)
    lam = np.asarray(strength, dtype=np.float32)
    B = lam.shape[0]
    scan = lam.ndim == 2
    lam = lam.reshape(B, -1).astype(nd)
    ny, nx = n_src
    S, Lk = ny * nx, lam.shape[1]
    H, W = rs.wcs.n_x, rs.wcs.n_y
    fx, fy = torch.as_tensor(fx).to(dtype), torch.as_tensor(fy).to(dtype)
    pix = np.asarray(pix, dtype=np.int64)
    ll = np.zeros((B, H * W), dtype=nd) if lens_light is None else np.asarray(lens_light).astype(nd).reshape(B, H * W)
    obs = np.broadcast_to(np.asarray(obs_used).astype(nd), (B, pix.size))
    sig = np.broadcast_to(np.asarray(sig_used).astype(nd), (B, pix.size))
    pitch = np.broadcast_to(np.asarray(pitch, dtype=np.float32), (B,))
    cx = np.broadcast_to(np.asarray(center[0], dtype=np.float32), (B,))
    cy = np.broadcast_to(np.asarray(center[1], dtype=np.float32), (B,))
    R = reg_matrix(regularization, n_src, nd)
    ldr = nd(log_det_reg(regularization, n_src))
    out = {k: np.full((B, Lk) + s, np.nan, dtype=nd) for k, s in
           (("source", (ny, nx)), ("model_image", (H, W)), ("chi2", ()), ("reg", ()), ("log_det", ()), ("log_evidence", ()), ("cond", ()))}
    out["ok"] = np.zeros((B, Lk), dtype=bool)
    parts = []
    for b in range(B):
        Lm = mapping(fx[:, b], fy[:, b], n_src, pitch[b], cx[b], cy[b])
        F = operator(rs, Lm).numpy()[pix]
        y = obs[b] - ll[b][pix]
        Fw, yw = F / sig[b][:, None], y / sig[b]
        with np.errstate(over="ignore", invalid="ignore"):
            A0, rhs = Fw.T @ Fw, Fw.T @ yw
        parts.append((Lm.numpy(), F, y, A0, rhs))
        with np.errstate(divide="ignore"):  # (an rms whose square underflows: the broken-pivot cases)
            noise = np.sum(np.log(nd(2 * math.pi) * sig[b] ** 2), dtype=nd)
        for l in range(0 if return_parts == "only" else Lk):
            with np.errstate(over="ignore", invalid="ignore"):
                M = A0 + lam[b, l] * R
            try:
                if not np.all(np.isfinite(M)):
                    raise np.linalg.LinAlgError("not finite")
                C = np.linalg.cholesky(M)
            except np.linalg.LinAlgError:
                continue
            s = np.linalg.solve(C.T, np.linalg.solve(C, rhs)).astype(nd)
            fs = F @ s
            chi2 = np.sum(((y - fs) / sig[b]) ** 2, dtype=nd)
            reg = s @ (R @ s)
            log_det = 2 * np.sum(np.log(np.diag(C)), dtype=nd)
            img = ll[b].copy()
            img[pix] += fs
            out["ok"][b, l] = True
            out["source"][b, l] = s.reshape(ny, nx)
            out["model_image"][b, l] = img.reshape(H, W)
            out["chi2"][b, l], out["reg"][b, l], out["log_det"][b, l] = chi2, reg, log_det
            out["log_evidence"][b, l] = (-nd(0.5) * chi2 - nd(0.5) * lam[b, l] * reg - nd(0.5) * log_det + nd(0.5 * S) * np.log(lam[b, l])
                                         + nd(0.5) * ldr - nd(0.5) * noise)
            if dtype == F64:
                ev = np.linalg.eigvalsh(M)  # M is symmetric positive definite: the 2-norm condition number
                out["cond"][b, l] = ev[-1] / ev[0]
    if not scan:
        out = {k: v[:, 0] for k, v in out.items()}
    return (out, parts) if return_parts else out


def reconstruct(phys, cfg, psf, params, observed, err_map, *, n_src, pitch, center, regularization, strength, mask=None,
                deflection_scale=1.0, dtype=F64, return_parts=False):
    """The restatement of ``reconstruct_source``.  ``params``: nested dict of ``[B]`` arrays; ``observed``, ``err_map`` ``[H, W]`` or
    ``[B, H, W]``; ``pitch``, ``center``: scalars or ``[B]``; ``strength``: ``[B]`` or ``[B, L]`` (taken as the float32 values the
    library receives).  Returns numpy arrays in ``dtype``: the keys of the call, with the ``L`` axis where ``strength`` is 2-D,
    plus ``cond`` (the 2-norm condition number of ``M``, float64 runs only).  ``return_parts``: also the per-sample ``(L, F, y, A0, b)``
    (``"only"``: without solving).  A sample whose Cholesky fails has ``ok`` false and NaN outputs.  The rays come from the lens of
    ``params``; everything after them is ``reconstruct_from_rays``."""
    from oracle import ref_torch as ref
    nd = _np_dtype(dtype)
    B = np.asarray(strength).shape[0]
    tparams = {g: [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype).reshape(-1).expand(B) for k, v in d.items()}
                   for d in lst] for g, lst in params.items()}
    rs = ref.RefSimulator(phys, cfg, B, dtype=dtype, supersampled_kernel=psf)
    H, W = rs.wcs.n_x, rs.wcs.n_y
    fx, fy = frame_beta(rs, tparams["lens_mass"], deflection_scale)
    ll = lens_light_image(rs, tparams).numpy().reshape(B, H * W)
    pix = used_pixels(rs, mask)
    obs = np.broadcast_to(np.asarray(observed, dtype=np.float32).astype(nd).reshape(-1, H * W), (B, H * W))[:, pix]
    sig = np.broadcast_to(np.asarray(err_map, dtype=np.float32).astype(nd).reshape(-1, H * W), (B, H * W))[:, pix]
    return reconstruct_from_rays(rs, fx, fy, ll, pix, obs, sig, n_src=n_src, pitch=pitch, center=center,
                                 regularization=regularization, strength=strength, dtype=dtype, return_parts=return_parts)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_pixsrc.py (shapes where the kernels can go wrong, not workload size)
# ---------------------------------------------------------------------------------------------------------------------
def gauss_psf(shape, sigma):
    gy = np.exp(-0.5 * ((np.arange(shape[0]) - (shape[0] - 1) / 2) / sigma) ** 2)
    gx = np.exp(-0.5 * ((np.arange(shape[1]) - (shape[1] - 1) / 2) / sigma) ** 2)
    k = np.outer(gy, gx)
    return (k / k.sum()).astype(np.float32)


def smooth_source(n_src, b):
    """A smooth positive ``s_true``: an off-centre Gaussian blob whose place and width change with the sample."""
    ny, nx = n_src
    jj, ii = np.mgrid[:ny, :nx]
    cy, cx = (ny - 1) * (0.45 + 0.05 * b), (nx - 1) * (0.55 - 0.04 * b)
    w = 0.22 * max(ny, nx) + 0.5
    return (1.0 + 0.2 * b) * np.exp(-0.5 * (((jj - cy) / w) ** 2 + ((ii - cx) / (1.2 * w)) ** 2))


DELTA_PIX = 0.1


def _f32(*v):
    return np.asarray(v, dtype=np.float32)


def case(name):
    """``dict(phys, cfg, psf, params, kw)`` of one case; ``kw`` holds the keywords of ``reconstruct_source`` (numpy, float32) bar
    the data.  The strengths and the noise level are chosen so that, for every sample and strength, ``cond(M) <= 1e4`` and four
    times the float32 yardstick stays under 1e-2 (source) and 1e-3 (the rest): both are asserted by the tests, on the reference."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    sersic_src = {"R_sersic": _f32(0.1), "n_sersic": _f32(1.5), "center_x": _f32(0.0), "center_y": _f32(0.0), "Ie": _f32(1.0)}
    if name == "A":  # SIE + Shear | Sersic lens light; 12 x 10 at supersample 2, 5 x 3 PSF, 7 x 6 nodes, per-sample pose, L-shaped mask
        phys = PhysicalModel([SIE(), Shear()], [Sersic()], [Sersic()])
        cfg = SimulatorConfig(delta_pix=DELTA_PIX, num_pix=(12, 10), supersample=2)
        params = {"lens_mass": [{"theta_E": _f32(0.30, 0.32, 0.28), "e1": _f32(0.10, -0.05, 0.15), "e2": _f32(-0.05, 0.10, 0.02),
                                 "center_x": _f32(0.01, -0.02, 0.0), "center_y": _f32(-0.01, 0.0, 0.02)},
                                {"gamma1": _f32(0.03, -0.02, 0.0), "gamma2": _f32(-0.01, 0.02, 0.03)}],
                  "lens_light": [{"R_sersic": _f32(0.2, 0.25, 0.18), "n_sersic": _f32(2.0, 3.0, 2.5), "center_x": _f32(0.01, -0.02, 0.0),
                                  "center_y": _f32(-0.01, 0.0, 0.02), "Ie": _f32(5.0, 4.0, 6.0)}],
                  "source_light": [sersic_src]}
        mask = np.ones((12, 10), dtype=bool)
        mask[:4, :2] = False
        mask[:2, :5] = False
        kw = dict(n_src=(7, 6), pitch=_f32(0.08, 0.09, 0.075), center=(_f32(0.02, -0.01, 0.0), _f32(-0.01, 0.015, 0.0)),
                  regularization="curvature", strength=_f32(2.0, 1.0, 4.0), mask=mask)
        return dict(phys=phys, cfg=cfg, psf=gauss_psf((5, 3), 1.1), params=params, kw=kw, sigma=0.02, B=3)
    if name == "B":  # EPL + Shear, no lens light; 40 x 36, 3 x 3 PSF, 33 x 31 = 1023 nodes, a [2, 3] scan over two decades
        phys = PhysicalModel([EPL(), Shear()], [], [Sersic()])
        cfg = SimulatorConfig(delta_pix=DELTA_PIX, num_pix=(40, 36), supersample=1)
        params = {"lens_mass": [{"theta_E": _f32(1.1, 1.0), "gamma": _f32(2.0, 2.1), "e1": _f32(0.08, -0.1), "e2": _f32(0.05, 0.04),
                                 "center_x": _f32(0.02, -0.03), "center_y": _f32(0.0, 0.04)},
                                {"gamma1": _f32(0.02, -0.03), "gamma2": _f32(0.01, 0.02)}],
                  "source_light": [sersic_src]}
        kw = dict(n_src=(33, 31), pitch=_f32(0.05), center=(_f32(0.03), _f32(-0.02)), regularization="gradient",
                  strength=np.asarray([[1.0, 10.0, 100.0], [2.0, 20.0, 200.0]], dtype=np.float32), mask=None)
        return dict(phys=phys, cfg=cfg, psf=gauss_psf((3, 3), 0.8), params=params, kw=kw, sigma=0.05, B=2)
    if name in ("C11", "C21"):  # no PSF, supersample 1: 1 x 1 and 2 x 1 nodes, one sample
        phys = PhysicalModel([SIE(), Shear()], [], [Sersic()])
        cfg = SimulatorConfig(delta_pix=DELTA_PIX, num_pix=(9, 8), supersample=1)
        params = {"lens_mass": [{"theta_E": _f32(0.25), "e1": _f32(0.1), "e2": _f32(0.05), "center_x": _f32(0.0), "center_y": _f32(0.0)},
                                {"gamma1": _f32(0.02), "gamma2": _f32(-0.01)}],
                  "source_light": [sersic_src]}
        kw = dict(n_src=(1, 1) if name == "C11" else (2, 1), pitch=_f32(0.15), center=(_f32(0.01), _f32(0.0)),
                  regularization="identity", strength=_f32(0.5), mask=None)
        return dict(phys=phys, cfg=cfg, psf=None, params=params, kw=kw, sigma=0.01, B=1)
    if name == "D":  # a grid half off the rays; sample 1 is an SIE at e = 0 (every deflection NaN), sample 2 an SIE centred exactly on
        # a supersampled pixel (NaN at that pixel alone)
        from gigalens_amd.simulator import LensWCS
        phys = PhysicalModel([SIE(), Shear()], [], [Sersic()])
        cfg = SimulatorConfig(delta_pix=DELTA_PIX, num_pix=(11, 13), supersample=2)
        px, py = LensWCS(n=(11, 13), supersample=2, pix_scale=DELTA_PIX).pix2angle(np.array([12]), np.array([10]))
        params = {"lens_mass": [{"theta_E": _f32(0.3, 0.3, 0.3), "e1": _f32(0.1, 0.0, 0.08), "e2": _f32(-0.05, 0.0, 0.03),
                                 "center_x": _f32(0.0, 0.0, px[0]), "center_y": _f32(0.0, 0.0, py[0])},
                                {"gamma1": _f32(0.02, 0.0, 0.01), "gamma2": _f32(0.0, 0.0, 0.0)}],
                  "source_light": [sersic_src]}
        kw = dict(n_src=(5, 9), pitch=_f32(0.06), center=(_f32(0.27), _f32(0.0)), regularization="gradient",
                  strength=_f32(3.0, 3.0, 3.0), mask=None)
        return dict(phys=phys, cfg=cfg, psf=gauss_psf((3, 3), 0.9), params=params, kw=kw, sigma=0.02, B=3)
    raise KeyError(name)


CASES = ("A", "B", "C11", "C21", "D")
_DATA = {}


def data(name):
    """``(case, observed [B, H, W] float32, err_map [H, W] float32, reference dict (float64), yardstick dict (float32))``, computed
    once.  The observed images are the float64 restatement's ``lens light + F s_true`` plus seeded Gaussian noise at ``err_map``."""
    if name not in _DATA:
        c = case(name)
        B, kw = c["B"], c["kw"]
        H, W = c["cfg"].num_pix
        err = np.full((H, W), c["sigma"], dtype=np.float32)
        zero = np.zeros((H, W), dtype=np.float32)
        lam1 = np.ones(B, dtype=np.float32)
        _, parts = reconstruct(c["phys"], c["cfg"], c["psf"], c["params"], zero, err, **{**kw, "strength": lam1, "mask": None},
                               return_parts="only")
        rng = np.random.default_rng(2006 + sum(ord(ch) for ch in name))
        obs = np.empty((B, H, W), dtype=np.float32)
        for b in range(B):
            s_true = smooth_source(kw["n_src"], b).reshape(-1)
            clean = parts[b][1] @ s_true - parts[b][2]  # F s_true + lens light (y = 0 - lens light there)
            obs[b] = (clean.reshape(H, W) + c["sigma"] * rng.normal(size=(H, W))).astype(np.float32)
        ref = reconstruct(c["phys"], c["cfg"], c["psf"], c["params"], obs, err, **kw)
        f32 = reconstruct(c["phys"], c["cfg"], c["psf"], c["params"], obs, err, **kw, dtype=torch.float32)
        _DATA[name] = (c, obs, err, ref, f32)
    return _DATA[name]


ARRAYS, SCALARS = ("source", "model_image"), ("chi2", "reg", "log_det", "log_evidence")


def errors(got, ref, S):
    """Per quantity the largest error of ``got`` against ``ref``: arrays normalised by the largest absolute element of the reference
    (per sample and strength), scalars by ``|chi2| + |log_det| + S``."""
    out = {}
    for k in ARRAYS:
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        scale = np.abs(r).max(axis=(-2, -1), keepdims=True)
        scale = np.where(scale > 0, scale, 1.0)  # (a source that is exactly zero: absolute error)
        out[k] = float((np.abs(g - r) / scale).max())
    norm = np.abs(ref["chi2"]) + np.abs(ref["log_det"]) + S
    for k in SCALARS:
        out[k] = float((np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]) / norm).max())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix of tests/test_gpu_pixsrc_matrix.py: rays of the tests' own handed to the native call, one case per block, chunk,
# slice, stencil and range edge of csrc/gl_pixsrc.hip.h and csrc/gl_api_pixsrc.hip.  The simulator supplies the frame, the
# supersampling and the PSF alone (pixel scale 1, so the flux scale of the operator is 1).
# ---------------------------------------------------------------------------------------------------------------------
MATRIX_DELTA_PIX = 1.0
PIX_TK, PIX_MAX_L_SLICE, PIX_MAX_PLANES = 32, 4, 4096
PIX_CHUNK_BUDGET, PIX_PLANE_BUDGET = 256 << 20, 32 << 20


def layout(frame, supersample, psf, B, L, S, n_used):
    """``dict(cb, lch, pc, n_pad)``: the host loops' split, restated from the budgets of csrc/gl_api_pixsrc.hip (float32 workspace:
    per sample the operator ``S n_pad``, ``yw``, ``A0``, ``lch`` factors and ``b``; per basis plane the supersampled plane, where the
    model post-processes, and the pooled one)."""
    HW = frame[0] * frame[1]
    HsWs = HW * supersample * supersample
    n_pad = -(-n_used // PIX_TK) * PIX_TK
    lch = min(L, PIX_MAX_L_SLICE)
    per_sample = 4 * (S * n_pad + n_pad + S * S * (1 + lch) + S)
    cb = max(1, min(B, PIX_CHUNK_BUDGET // per_sample))
    per_plane = 4 * ((HsWs if (psf is not None or supersample != 1) else 0) + HW)
    pc = max(1, min(cb * S, PIX_MAX_PLANES, PIX_PLANE_BUDGET // per_plane))
    return dict(cb=cb, lch=lch, pc=pc, n_pad=n_pad)


def splits(total, step):
    """The lengths of the iterations of ``for i0 in range(0, total, step)``."""
    return [min(step, total - i0) for i0 in range(0, total, step)]


def _m(group, n_src, reg, *, frame=(16, 16), ss=1, psf=None, B=1, L=1, n_used=None, lens_light=False, pose="shared", lam=None,
       sigma0=0.05, sits_on=""):
    return dict(group=group, n_src=n_src, reg=reg, frame=frame, ss=ss, psf=psf, B=B, L=L, n_used=n_used, lens_light=lens_light,
                pose=pose, lam=lam, sigma0=sigma0, sits_on=sits_on)


def _matrix():
    m = {}
    # solve blocks: no PSF, supersample 1, all pixels used, B = 2, L = 1
    for n_src, reg, frame, B, on in (((4, 8), "gradient", (16, 16), 2, "one full block, no panel"),
                                     ((3, 11), "curvature", (16, 16), 2, "a panel of one row, a last block of one"),
                                     ((8, 8), "identity", (16, 16), 2, "two full blocks"),
                                     ((5, 13), "gradient", (16, 16), 2, "two full blocks and a last block of one"),
                                     ((16, 18), "gradient", (32, 32), 2, "the last S with one stride of the 256-row loops"),
                                     ((17, 17), "gradient", (32, 32), 2, "the first S with a second stride"),
                                     ((32, 32), "curvature", (32, 32), 1, "the cap: 32 blocks, 528 normal tiles")):
        m[f"solve_S{n_src[0] * n_src[1]}"] = _m("solve", n_src, reg, frame=frame, B=B, sits_on=on)
    # the same 289 nodes under a 3 x 3 PSF: with the recipe's unrelated rays the PSF makes A0 dense (94 % of its entries), where the
    # cases above have a banded M whose rows a second stride of the 256-row loops reaches hold zeros only
    m["dense_S289"] = _m("solve", (17, 17), "gradient", frame=(32, 32), psf=gauss_psf((3, 3), 0.8), B=2,
                         sits_on="the second stride of the 256-row loops on non-zero rows")
    # stencil ends: every branch of pix_r1 (n = 1, 2, >= 3; corner and interior diagonals; |d| = 1 and 2 along either axis)
    for reg in ("gradient", "curvature"):
        for n_src in ((1, 1), (1, 2), (2, 1), (1, 33), (33, 1)):
            m[f"stencil_{reg}_{n_src[0]}x{n_src[1]}"] = _m("stencil", n_src, reg)
    for n_src in ((2, 16), (16, 2), (3, 3), (3, 11)):
        m[f"stencil_curvature_{n_src[0]}x{n_src[1]}"] = _m("stencil", n_src, "curvature")
    # pixel counts against the tile of 32: S = 40, 12 x 10 at supersample 2 with a 3 x 3 PSF; n_used < S leaves A0 singular
    for n in (5, 31, 32, 33, 64, 95, 120):
        m[f"pixels_{n}"] = _m("pixels", (5, 8), "gradient", frame=(12, 10), ss=2, psf=gauss_psf((3, 3), 0.8), B=2, n_used=n,
                              lens_light=n != 33, sits_on="n_used < S" if n < 40 else f"n_used % 32 = {n % 32}")
    m["frame_255"] = _m("pixels", (5, 8), "gradient", frame=(15, 17), B=2, sits_on="HsWs = 255: the q guard of the planes kernel")
    # rays placed by hand (matrix_inputs), B = 3
    for reg in ("identity", "curvature"):
        m[f"hand_{reg}"] = _m("hand", (5, 9), reg, B=3, pose="hand")
    # host loops
    for L in (5, 8, 9):
        m[f"slices_{L}"] = _m("loops", (3, 11), "gradient", B=3, L=L, sits_on="slices of " + " + ".join(map(str, splits(L, 4))))
    m["planes_budget"] = _m("loops", (5, 9), "gradient", frame=(64, 64), ss=2, psf=gauss_psf((3, 3), 0.8), B=10,
                            sigma0=0.5, sits_on="the 32 MB of planes: a launch ends inside a sample")
    m["planes_cap"] = _m("loops", (10, 10), "gradient", frame=(10, 10), B=41, sits_on="4096 planes per launch")
    cb = layout((32, 32), 1, None, 65535, 5, 1024, 1024)["cb"]
    m["chunks"] = _m("loops", (32, 32), "gradient", frame=(32, 32), B=cb + 1, L=5, lens_light=True, pose="per_sample",
                     sits_on="a second chunk of samples and a second slice together")
    # a pivot failure after the first block (matrix_inputs); a harder system with a gate of its own
    m["pivot"] = _m("pivot", (5, 8), "gradient", frame=(12, 10), B=2, sits_on="a pivot that is not finite in the second block")
    m["hard"] = _m("hard", (17, 17), "gradient", B=2, lam=HARD_STRENGTH, sits_on="cond(M) in [1e3, 1e4]")
    return m


# planes_budget: at the recipe's rms of 0.05 the float32 sums over its 4096 used pixels put the yardstick of the source at 1.2e-5,
# past the cap of the main gates; at 0.5 it is 1.2e-6.  hard: 256 rays on 289 nodes leave A0 singular, and the strength is lowered on
# the float64 reference until cond(M) lies in [1e3, 1e4] (2e3 and 4e3; asserted by the tests).
HARD_STRENGTH = 0.2
PIVOT_NODE = 35
MATRIX = _matrix()
MAIN = tuple(n for n, c in MATRIX.items() if c["group"] not in ("pivot", "hard"))  # the cases that share the main gates
LOOPS = tuple(n for n, c in MATRIX.items() if c["group"] == "loops")
_MDATA = {}


def matrix_sim_args(name):
    """``(phys, cfg, psf)`` of the simulator of a case: any one-lens model does, its lens is not used."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    c = MATRIX[name]
    return (PhysicalModel([SIE()], [], [Sersic()]), SimulatorConfig(delta_pix=MATRIX_DELTA_PIX, num_pix=c["frame"], supersample=c["ss"]),
            c["psf"])


def _hand_uv(n_src, Q, rng):
    """Sample 0 of the hand-placed cases: ``u, v [Q]`` (float64; exact in float32 under the dyadic pose of these cases).  Node
    ``(2, 4)`` is touched by no ray: no ray lies in its support ``(3, 5) x (1, 3)``."""
    ny, nx = n_src
    u, v = [], []
    for j in range(ny):  # exactly on every node bar (2, 4): unit rows
        for i in range(nx):
            if (j, i) != (2, 4):
                u.append(float(i)), v.append(float(j))
    steps = []  # (ray, axis, edge, direction): matrix_inputs moves the ray's beta to the first float32 past the edge
    for axis, n in ((0, nx), (1, ny)):
        for e, d in ((-2.0, 0), (-1.0, 0), (float(n), 0), (n + 1.0, 0), (-2.0, -1), (-2.0, 1), (n + 1.0, -1), (n + 1.0, 1)):
            if d:
                steps.append((len(u), axis, e, d))
            u.append(e if axis == 0 else 0.5), v.append(0.5 if axis == 0 else e)
    for e in (-0.75, -0.25, nx - 0.75, nx - 0.25):  # inside (-1, 0) and (nx - 1, nx): half-supported border cells
        u.append(e), v.append(1.25)
    for e in (-0.75, -0.25, ny - 0.75, ny - 0.25):
        u.append(0.25), v.append(e)
    for bad in (float("nan"), float("inf"), float("-inf")):
        u.append(bad), v.append(1.0)
        u.append(1.0), v.append(bad)
    n = Q - len(u)
    assert n > 0
    uu, vv = rng.uniform(-1, nx, size=4 * n), rng.uniform(-1, ny, size=4 * n)
    keep = ~((uu > 3) & (uu < 5) & (vv > 1) & (vv < 3))
    return np.concatenate([u, uu[keep][:n]]), np.concatenate([v, vv[keep][:n]]), steps


def grid_coordinate(beta, pitch, c, n):
    """``u`` (or ``v``) of a float32 ``beta`` in the float32 arithmetic of the planes kernel."""
    return (np.float32(beta) - np.float32(c)) / np.float32(pitch) + np.float32(0.5) * np.float32(n - 1)


def matrix_inputs(name):
    """The float32 inputs of the native call for a case, as numpy: ``beta_x, beta_y [B, Hs Ws]``, ``obs, sigma [B, n_used]``,
    ``lens_light [B, H W]`` or None, ``pix [n_used]`` int32, ``pose [B, 3]``, ``strength [B, L]``; plus the float64 ``u, v`` they
    were made from.  The recipe: seeded uniform rays with ``u`` in ``[-1, nx]``, ``v`` in ``[-1, ny]``; ``sigma = 0.05 (1 + 0.1 b)``;
    strengths between 10 and 100; ``obs = lens light + F s_true + noise`` formed in float64 (by ``matrix_data``)."""
    import zlib
    c = MATRIX[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    (ny, nx), B, L = c["n_src"], c["B"], c["L"]
    (H, W), ss = c["frame"], c["ss"]
    HW, Q = H * W, H * W * ss * ss
    u, v = rng.uniform(-1, nx, size=(B, Q)), rng.uniform(-1, ny, size=(B, Q))
    bidx = np.arange(B)
    if c["pose"] == "per_sample":
        pose = np.stack([0.5 * (1 + 0.02 * bidx), 0.1 * bidx - 0.3, 0.2 - 0.05 * bidx], axis=1)
    elif c["pose"] == "hand":  # dyadic: u and v of the hand-placed rays are exact in float32 and float64 alike
        pose = np.stack([np.full(B, 0.5), np.full(B, 0.25), np.full(B, -0.5)], axis=1)
    else:
        pose = np.stack([np.full(B, 0.37), np.full(B, 0.11), np.full(B, -0.07)], axis=1)
    pose = pose.astype(np.float32)
    if c["group"] == "hand":
        u[0], v[0], steps = _hand_uv(c["n_src"], Q, rng)
        u[1] = np.where(rng.uniform(size=Q) < 0.5, rng.uniform(-40, -1, size=Q), rng.uniform(nx, nx + 40, size=Q))  # every ray misses
    pix = np.arange(HW)
    if c["n_used"] is not None and c["n_used"] < HW:  # scattered, keeping the first and the last pixel
        pix = np.sort(np.concatenate([[0, HW - 1], 1 + rng.choice(HW - 2, size=c["n_used"] - 2, replace=False)]))
    sigma = np.repeat((c["sigma0"] * (1 + 0.1 * bidx))[:, None], pix.size, axis=1)
    if c["group"] == "pivot":  # sample 0: the ray of used pixel 7 sits exactly on node PIVOT_NODE, and that pixel's rms is 1e-25
        u[0, 7], v[0, 7] = PIVOT_NODE % nx, PIVOT_NODE // nx
        sigma[0, 7] = 1e-25
    with np.errstate(invalid="ignore"):
        bx = pose[:, 1:2].astype(np.float64) + (u - (nx - 1) / 2) * pose[:, 0:1].astype(np.float64)
        by = pose[:, 2:3].astype(np.float64) + (v - (ny - 1) / 2) * pose[:, 0:1].astype(np.float64)
    bx, by = bx.astype(np.float32), by.astype(np.float32)
    if c["group"] == "hand":  # one float32 step either side of -2 and n + 1: the first beta whose float32 u lies past the edge
        for q, axis, e, d in steps:
            beta, n = (bx, nx) if axis == 0 else (by, ny)
            while not (grid_coordinate(beta[0, q], pose[0, 0], pose[0, 1 + axis], n) - np.float32(e)) * d > 0:
                beta[0, q] = np.nextafter(beta[0, q], np.float32(d * np.inf))
    if c["lam"] is not None:
        lam = np.full((B, L), c["lam"])
    else:
        lam = (np.geomspace(10, 90, L) if L > 1 else np.asarray([30.0]))[None, :] * (1 + 0.1 * bidx / max(B - 1, 1))[:, None]
    ll = None
    if c["lens_light"]:
        jj, ii = np.mgrid[:H, :W]
        ll = np.stack([(2.0 + 0.1 * b) * np.exp(-0.5 * (((jj - H / 2) / (0.3 * H)) ** 2 + ((ii - W / 2) / (0.3 * W)) ** 2))
                       for b in range(B)]).reshape(B, HW).astype(np.float32)
    noise = rng.normal(size=(B, pix.size))
    return dict(beta_x=bx, beta_y=by, sigma=sigma.astype(np.float32), lens_light=ll,
                pix=pix.astype(np.int32), pose=pose, strength=lam.astype(np.float32), u=u, v=v, noise=noise)


def matrix_rs(name, B, dtype=F64):
    from oracle import ref_torch as ref
    phys, cfg, psf = matrix_sim_args(name)
    return ref.RefSimulator(phys, cfg, B, dtype=dtype, supersampled_kernel=psf)


def matrix_reference(name, inp, dtype=F64, samples=None, return_parts=False):
    """``reconstruct_from_rays`` on the inputs of ``matrix_inputs`` (``inp["obs"]`` included), for all or some ``samples``."""
    c = MATRIX[name]
    sel = np.arange(c["B"]) if samples is None else np.asarray(samples)
    rs = matrix_rs(name, len(sel), dtype)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel].T))
    return reconstruct_from_rays(rs, t(inp["beta_x"]), t(inp["beta_y"]), None if inp["lens_light"] is None else inp["lens_light"][sel],
                                 inp["pix"], inp["obs"][sel], inp["sigma"][sel], n_src=c["n_src"], pitch=inp["pose"][sel, 0],
                                 center=(inp["pose"][sel, 1], inp["pose"][sel, 2]), regularization=c["reg"],
                                 strength=inp["strength"][sel], dtype=dtype, return_parts=return_parts)


def matrix_data(name):
    """``(case, inputs with obs, reference dict (float64), yardstick dict (float32))`` of a case of ``MATRIX``, computed once and left
    unchanged.  Every output carries the ``L`` axis."""
    if name not in _MDATA:
        c = MATRIX[name]
        inp = matrix_inputs(name)
        B, n_used = c["B"], inp["pix"].size
        inp["obs"] = np.zeros((B, n_used), dtype=np.float32)
        _, parts = matrix_reference(name, {**inp, "sigma": np.ones_like(inp["sigma"])}, return_parts="only")
        ll = np.zeros((B, n_used)) if inp["lens_light"] is None else inp["lens_light"].astype(np.float64)[:, inp["pix"]]
        clean = np.stack([parts[b][1] @ smooth_source(c["n_src"], b % 3).reshape(-1) for b in range(B)])  # F s_true, float64
        inp["obs"] = (ll + clean + inp["sigma"].astype(np.float64).clip(max=1.0) * inp["noise"]).astype(np.float32)
        _MDATA[name] = (c, inp, matrix_reference(name, inp), matrix_reference(name, inp, dtype=torch.float32))
    return _MDATA[name]


def _case_layout(name):
    c = MATRIX[name]
    n_used = c["n_used"] or c["frame"][0] * c["frame"][1]
    return layout(c["frame"], c["ss"], c["psf"], c["B"], c["L"], c["n_src"][0] * c["n_src"][1], n_used)


def check_split(name, lay):
    """Asserts on a layout (the library's ``pixsrc_layout`` or the restatement ``layout``) that the host loop a case of ``LOOPS`` is
    named for makes at least two iterations, with the split the case states."""
    c = MATRIX[name]
    B, L, S = c["B"], c["L"], c["n_src"][0] * c["n_src"][1]
    if name.startswith("slices_"):
        assert splits(L, lay["lch"]) == {5: [4, 1], 8: [4, 4], 9: [4, 4, 1]}[L]
    elif name == "planes_budget":
        assert lay["cb"] == B and lay["pc"] < B * S and lay["pc"] % S != 0  # a launch ends inside a sample
        assert len(splits(B * S, lay["pc"])) >= 2
    elif name == "planes_cap":
        assert lay["cb"] == B and lay["pc"] == PIX_MAX_PLANES and len(splits(B * S, lay["pc"])) == 2
    elif name == "chunks":
        assert lay["cb"] < B and lay["lch"] < L  # b0 and l0 are non-zero together
        assert splits(B, lay["cb"]) == [B - 1, 1] and splits(L, lay["lch"]) == [4, 1]
        assert len(splits(lay["cb"] * S, lay["pc"])) >= 2
    else:
        raise KeyError(name)


def alone_samples(name):
    """The samples of a host-loop case that are run again alone: the first, one in the middle, the last (for ``chunks`` the one in
    the second chunk) and the one inside which the first launch of planes ends."""
    c, lay = MATRIX[name], _case_layout(name)
    return sorted({0, c["B"] // 2, c["B"] - 1, min(lay["pc"] // (c["n_src"][0] * c["n_src"][1]), c["B"] - 1)})
