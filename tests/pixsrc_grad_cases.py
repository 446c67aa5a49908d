"""Two-stage float64 oracle of the evidence gradient (LensSimulator.source_evidence_and_grad), in torch, on the restatement of
tests/pixsrc_cases.py.

Stage 1: per sample the rays are leaf tensors (rays that are not finite are replaced by an out-of-range constant, so they get
exact zero rows and exact zero cotangents), the pose and the lens-light image are leaves too; E is formed with
``torch.linalg.cholesky`` and autograd gives dE/dbeta, dE/dpose, dE/d(lens light image).
Stage 2: for every sample ``RefSimulator.beta`` is evaluated only on the pixels that have finite rays and a non-zero cotangent;
autograd through it gives the lens-mass gradient; the lens-light gradient comes from autograd through the lens-light render.
The same code in float32 is the yardstick."""
import math

import numpy as np
import torch

from tests import pixsrc_cases as PC

F64 = torch.float64
FAR = 1.0e6  # a ray that fails the range test of any grid: a row of exact zeros


def mapping_d(beta_x, beta_y, n_src, pitch, cx, cy):
    """``PC.mapping`` with the pose as tensors (differentiable in it)."""
    ny, nx = n_src
    dt = beta_x.dtype
    u = (beta_x - cx) / pitch + (nx - 1) / 2
    v = (beta_y - cy) / pitch + (ny - 1) / 2
    ok = (u >= -2) & (u <= nx + 1) & (v >= -2) & (v <= ny + 1)
    u, v = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    wu = PC.hat(u[:, None] - torch.arange(nx, dtype=dt))
    wv = PC.hat(v[:, None] - torch.arange(ny, dtype=dt))
    L = (wv[:, :, None] * wu[:, None, :]).reshape(-1, ny * nx)
    return torch.where(ok[:, None], L, torch.zeros_like(L))


def evidence(rs, bx, by, pose, ll, pix, obs_u, sig_u, n_src, regularization, lam, return_parts=False):
    """E of one sample as a torch scalar: log_evidence of the restatement, every term.  ``bx, by`` [Hs Ws] (finite), ``pose`` [3]
    (pitch, cx, cy), ``ll`` [H W] lens-light image, ``obs_u, sig_u`` [n_used], ``lam`` a float."""
    dt = bx.dtype
    S = n_src[0] * n_src[1]
    L = mapping_d(bx, by, n_src, pose[0], pose[1], pose[2])
    F = PC.operator(rs, L)[pix]
    y = obs_u - ll[pix]
    Fw, yw = F / sig_u[:, None], y / sig_u
    R = torch.as_tensor(PC.reg_matrix(regularization, n_src, np.float64)).to(dt)
    M = Fw.t() @ Fw + lam * R
    C = torch.linalg.cholesky(M)
    s = torch.cholesky_solve((Fw.t() @ yw)[:, None], C)[:, 0]
    rw = yw - Fw @ s
    log_det = 2 * torch.log(torch.diagonal(C)).sum()
    noise = torch.log(2 * math.pi * sig_u ** 2).sum()
    E = (-0.5 * (rw * rw).sum() - 0.5 * lam * (s @ (R @ s)) - 0.5 * log_det + 0.5 * S * math.log(lam)
         + 0.5 * PC.log_det_reg(regularization, n_src) - 0.5 * noise)
    if return_parts:
        return E, dict(Fw=Fw, rw=rw, s=s, M=M, F=F)
    return E


def _tparams(params, B, dtype):
    """The case's parameters (float32 values) as ``[B]`` tensors in ``dtype``; float64 arrays are taken as they are (the steps of the
    central differences must not be rounded to float32)."""
    as_np = lambda v: np.asarray(v) if np.asarray(v).dtype == np.float64 else np.asarray(v, dtype=np.float32)
    return {g: [{k: torch.as_tensor(as_np(v)).to(dtype).reshape(-1).expand(B).clone() for k, v in d.items()}
                for d in lst] for g, lst in params.items()}


def _per(v, B):
    return np.broadcast_to(np.asarray(v, dtype=np.float32), (B,))


def oracle(c, obs, err, strength=None, dtype=F64, rays=None, params=None):
    """The gradient of the evidence of case dict ``c`` on data ``obs [B, H, W]``, ``err [H, W]``: a dict of numpy float64 arrays
    ``E [B]``, ``grad_beta [2, B, Hs Ws]``, ``grad_pose [B, 3]``, ``grad_lens`` / ``grad_light`` (lists, one dict name -> [B] per
    profile), ``min_line_dist`` (least distance of a ray inside the grid to a grid line, in u, v) and ``rays`` (fx, fy).
    ``strength``: [B], default the case's.  ``rays``: (fx, fy) [Hs Ws, B] to use in place of the ray-shoot (stage 1 only matters then:
    ``grad_lens`` is still taken at the case's parameters).  ``params``: other parameters than the case's."""
    from oracle import ref_torch as ref
    kw, B = c["kw"], c["B"]
    params = c["params"] if params is None else params
    lam = _per(kw["strength"] if strength is None else strength, B).astype(np.float64)
    rs = ref.RefSimulator(c["phys"], c["cfg"], B, dtype=dtype, supersampled_kernel=c["psf"])
    rs1 = ref.RefSimulator(c["phys"], c["cfg"], 1, dtype=dtype, supersampled_kernel=c["psf"])
    H, W = rs.wcs.n_x, rs.wcs.n_y
    Hs, Ws = H * rs.supersample, W * rs.supersample
    tp = _tparams(params, B, dtype)
    with torch.no_grad():
        fx, fy = PC.frame_beta(rs, tp["lens_mass"], 1.0) if rays is None else (torch.as_tensor(rays[0]).to(dtype), torch.as_tensor(rays[1]).to(dtype))
        ll_all = PC.lens_light_image(rs, tp).reshape(B, H * W)
    pix = torch.from_numpy(PC.used_pixels(rs, kw["mask"]).astype(np.int64))
    obs_t = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(dtype).reshape(B, H * W)[:, pix]
    sig_t = torch.as_tensor(np.asarray(err, dtype=np.float32)).to(dtype).reshape(-1)[pix]
    pitch, cx, cy = _per(kw["pitch"], B), _per(kw["center"][0], B), _per(kw["center"][1], B)
    ny, nx = kw["n_src"]
    region_idx = rs.region[:, 0] * Ws + rs.region[:, 1]
    out = dict(E=np.zeros(B), grad_beta=np.zeros((2, B, Hs * Ws)), grad_pose=np.zeros((B, 3)), min_line_dist=np.inf,
               grad_lens=[{k: np.zeros(B) for k in d} for d in params["lens_mass"]],
               grad_light=[{k: np.zeros(B) for k in d} for d in params.get("lens_light", [])], rays=(fx.numpy(), fy.numpy()))
    for b in range(B):
        finite = torch.isfinite(fx[:, b]) & torch.isfinite(fy[:, b])
        far = torch.full_like(fx[:, b], FAR)
        bx = torch.where(finite, fx[:, b], far).clone().requires_grad_(True)
        by = torch.where(finite, fy[:, b], far).clone().requires_grad_(True)
        pose = torch.tensor([float(pitch[b]), float(cx[b]), float(cy[b])], dtype=dtype, requires_grad=True)
        ll = ll_all[b].clone().requires_grad_(True)
        E = evidence(rs1, bx, by, pose, ll, pix, obs_t[b], sig_t, (ny, nx), kw["regularization"], float(lam[b]))
        gbx, gby, gpose, gll = torch.autograd.grad(E, (bx, by, pose, ll))
        out["E"][b] = float(E.detach())
        out["grad_beta"][0, b], out["grad_beta"][1, b] = gbx.double().numpy(), gby.double().numpy()
        out["grad_pose"][b] = gpose.double().numpy()
        # distance of the rays inside the grid to the nearest grid line
        u = (bx.detach().double() - float(cx[b])) / float(pitch[b]) + (nx - 1) / 2
        v = (by.detach().double() - float(cy[b])) / float(pitch[b]) + (ny - 1) / 2
        inside = finite & (u > -1) & (u < nx) & (v > -1) & (v < ny)
        if inside.any():
            d = torch.minimum((u - torch.round(u)).abs(), (v - torch.round(v)).abs())[inside]
            out["min_line_dist"] = min(out["min_line_dist"], float(d.min()))
        # stage 2: the ray-shoot on the pixels with finite rays and a non-zero cotangent
        sel_full = finite & ((gbx != 0) | (gby != 0))
        sel = sel_full[torch.from_numpy(region_idx)]  # (rays outside pix_region are NaN: never selected)
        lp = [{k: v[b:b + 1].clone().requires_grad_(True) for k, v in d.items()} for d in tp["lens_mass"]]
        if sel.any():
            rx, ry = rs1.beta(rs1.img_X[sel], rs1.img_Y[sel], lp)
            idx = torch.from_numpy(region_idx)[sel]
            tot = (gbx[idx] * rx[:, 0] + gby[idx] * ry[:, 0]).sum()
            leaves = [v for d in lp for v in d.values()]
            g = torch.autograd.grad(tot, leaves, allow_unused=True)
            it = iter(g)
            for i, d in enumerate(lp):
                for k in d:
                    gv = next(it)
                    out["grad_lens"][i][k][b] = 0.0 if gv is None else float(gv)
        if params.get("lens_light"):
            tl = {"lens_mass": [{k: v[b:b + 1] for k, v in d.items()} for d in tp["lens_mass"]],
                  "lens_light": [{k: v[b:b + 1].clone().requires_grad_(True) for k, v in d.items()} for d in tp["lens_light"]]}
            img = PC.lens_light_image(rs1, tl).reshape(-1)
            leaves = [v for d in tl["lens_light"] for v in d.values()]
            g = torch.autograd.grad((img * gll).sum(), leaves, allow_unused=True)
            it = iter(g)
            for i, d in enumerate(tl["lens_light"]):
                for k in d:
                    gv = next(it)
                    out["grad_light"][i][k][b] = 0.0 if gv is None else float(gv)
    return out


def packed_grad(sim, o):
    """The oracle's parameter gradient ``[B, P]`` in the packed order of ``sim`` (source-light columns 0)."""
    B = o["E"].shape[0]
    g = np.zeros((B, sim._model.P))
    for col, slot in enumerate(sim._layout.slots):
        grp, i, name = slot[0], slot[1], slot[2]
        if grp == "lens_mass":
            g[:, col] = o["grad_lens"][i][name]
        elif grp == "lens_light":
            g[:, col] = o["grad_light"][i][name]
    return g


def evidence_at(c, obs, err, params, strength=None):
    """E [B] (float64) of the restatement at other parameters: ``PC.reconstruct``'s log_evidence (central differences)."""
    kw = dict(c["kw"])
    if strength is not None:
        kw["strength"] = strength
    kw["strength"] = _per(kw["strength"], c["B"])
    return PC.reconstruct(c["phys"], c["cfg"], c["psf"], params, obs, err, **kw)["log_evidence"]


_ORACLE = {}


def case_oracle(name):
    """``(case, obs, err, strength [B], float64 oracle, float32 oracle)`` of a case of ``PC.CASES`` on its ``data()``, computed once;
    for B (a [2, 3] scan) column 1 of the strengths."""
    if name not in _ORACLE:
        c, obs, err, _, _ = PC.data(name)
        lam = np.asarray(c["kw"]["strength"], dtype=np.float32)
        lam = lam[:, 1] if lam.ndim == 2 else _per(lam, c["B"])
        _ORACLE[name] = (c, obs, err, lam, oracle(c, obs, err, lam), oracle(c, obs, err, lam, dtype=torch.float32))
    return _ORACLE[name]


def evidence_only(c, obs, err, lam, params=None, dpose=(0.0, 0.0, 0.0)):
    """E [B] in float64 at ``params`` (default: the case's) and the pose moved by ``dpose``, without any gradient: what the
    central differences evaluate.  Rays that are not finite get rows of zeros, as in the oracle."""
    from oracle import ref_torch as ref
    kw, B = c["kw"], c["B"]
    params = c["params"] if params is None else params
    rs = ref.RefSimulator(c["phys"], c["cfg"], B, dtype=F64, supersampled_kernel=c["psf"])
    H, W = rs.wcs.n_x, rs.wcs.n_y
    tp = _tparams(params, B, F64)
    pix = torch.from_numpy(PC.used_pixels(rs, kw["mask"]).astype(np.int64))
    obs_t = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(F64).reshape(B, H * W)[:, pix]
    sig_t = torch.as_tensor(np.asarray(err, dtype=np.float32)).to(F64).reshape(-1)[pix]
    pitch, cx, cy = _per(kw["pitch"], B), _per(kw["center"][0], B), _per(kw["center"][1], B)
    out = np.zeros(B)
    with torch.no_grad():
        fx, fy = PC.frame_beta(rs, tp["lens_mass"], 1.0)
        ll_all = PC.lens_light_image(rs, tp).reshape(B, H * W)
        for b in range(B):
            finite = torch.isfinite(fx[:, b]) & torch.isfinite(fy[:, b])
            far = torch.full_like(fx[:, b], FAR)
            pose = torch.tensor([float(pitch[b]) + dpose[0], float(cx[b]) + dpose[1], float(cy[b]) + dpose[2]], dtype=F64)
            out[b] = float(evidence(rs, torch.where(finite, fx[:, b], far), torch.where(finite, fy[:, b], far), pose, ll_all[b], pix,
                                    obs_t[b], sig_t, kw["n_src"], kw["regularization"], float(lam[b])))
    return out
