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


def reconstruct(phys, cfg, psf, params, observed, err_map, *, n_src, pitch, center, regularization, strength, mask=None,
                deflection_scale=1.0, dtype=F64, return_parts=False):
    """The restatement of ``reconstruct_source``.  ``params``: nested dict of ``[B]`` arrays; ``observed``, ``err_map`` ``[H, W]`` or
    ``[B, H, W]``; ``pitch``, ``center``: scalars or ``[B]``; ``strength``: ``[B]`` or ``[B, L]`` (taken as the float32 values the
    library receives).  Returns numpy arrays in ``dtype``: the keys of the call, with the ``L`` axis where ``strength`` is 2-D,
    plus ``cond`` (the 2-norm condition number of ``M``, float64 runs only).  ``return_parts``: also the per-sample ``(L, F, y, A0, b)``
    (``"only"``: without solving).  A sample whose Cholesky fails has ``ok`` false and NaN outputs."""
    from oracle import ref_torch as ref
    nd = _np_dtype(dtype)
    lam = np.asarray(strength, dtype=np.float32)
    B = lam.shape[0]
    scan = lam.ndim == 2
    lam = lam.reshape(B, -1).astype(nd)
    tparams = {g: [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype).reshape(-1).expand(B) for k, v in d.items()}
                   for d in lst] for g, lst in params.items()}
    rs = ref.RefSimulator(phys, cfg, B, dtype=dtype, supersampled_kernel=psf)
    ny, nx = n_src
    S, Lk = ny * nx, lam.shape[1]
    H, W = rs.wcs.n_x, rs.wcs.n_y
    fx, fy = frame_beta(rs, tparams["lens_mass"], deflection_scale)
    ll = lens_light_image(rs, tparams).numpy()
    pix = used_pixels(rs, mask)
    obs = np.broadcast_to(np.asarray(observed, dtype=np.float32).astype(nd).reshape(-1, H * W), (B, H * W))
    sig = np.broadcast_to(np.asarray(err_map, dtype=np.float32).astype(nd).reshape(-1, H * W), (B, H * W))[:, pix]
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
        y = obs[b, pix] - ll[b].reshape(-1)[pix]
        Fw, yw = F / sig[b][:, None], y / sig[b]
        with np.errstate(over="ignore", invalid="ignore"):
            A0, rhs = Fw.T @ Fw, Fw.T @ yw
        parts.append((Lm.numpy(), F, y, A0, rhs))
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
            img = ll[b].reshape(-1).copy()
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
