"""float64 restatement of the critical-curve contouring (gl_critical_curves) in numpy, and the float64 fields it runs on.

`contour64` follows the specification of the native call step by step: D = det(I - H) at the (n+1)^2 vertices of a regular grid;
an edge whose two finite endpoint values differ in sign (sign = D < 0) is crossing and is bisected ON the edge; marching squares
per cell in row-major order with D < 0 on the left of every segment; the ambiguous cases joined when the mean of the four vertex
values is < 0; a segment is tangential when the mean of 1 - kappa at its endpoints is > 0.

The 16-case table below is, by design, the table the kernel uses: the restatement is independent of the kernel in its numerics
(float64 fields from the oracle), its edge listing, bisection and ordering, not in the table.  The table's orientation and the
loop topology are pinned independently by the closed-form tests (SIS: one loop of positive area pi theta_E^2; NFW: a radial loop
inside the tangential one).

The module also holds the small helpers the critical-curve GPU tests share (simulator, packed rows, the oracle's view of them)."""
import numpy as np

# a user-written SIS (p = theta_E, center_x, center_y), for the refusal test
SIS_BODY = """
template <class R> __device__ void deriv(R x, R y, const R* p, R& fx, R& fy) {
  R dx = x - p[1], dy = y - p[2];
  R r = sqrt(dx * dx + dy * dy);
  fx = p[0] * dx / r;
  fy = p[0] * dy / r;
}
"""


def simulator(lenses, num_pix, delta_pix, bs, constants=None):
    """A LensSimulator over ``lenses`` with one Sersic source (the critical-curve calls read the lens columns only)."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.simulator import LensSimulator, SimulatorConfig
    phys = PhysicalModel(lenses, [], [Sersic()], lenses_constants=constants)
    return LensSimulator(phys, SimulatorConfig(delta_pix=delta_pix, num_pix=num_pix), bs=bs)


def packed_rows(sim, lens_cols):
    """Packed [B, P] rows from the lens columns; the source columns get a valid Sersic."""
    import torch
    B = lens_cols.shape[0]
    src = np.tile(np.array([[0.2, 2.0, 0.0, 0.0, 1.0]], np.float32), (B, 1))
    return torch.tensor(np.concatenate([np.asarray(lens_cols, np.float32), src], 1), device=sim.device)


def lens_rows(sim, packed):
    """Per-lens dicts of float64 CPU columns (the oracle's view of the packed rows)."""
    from tests import helpers as H
    return H.struct_from_packed(sim.phys_model, packed.detach().double().cpu())["lens_mass"]

# corner bits (set when D < 0): 1 = (r, c), 2 = (r, c+1), 4 = (r+1, c+1), 8 = (r+1, c); cell edges 0 = bottom, 1 = right, 2 = top,
# 3 = left; (from, to) pairs walked with the D < 0 corners on the left (x to the right, y upwards)
CASES = {0: [], 1: [(0, 3)], 2: [(1, 0)], 3: [(1, 3)], 4: [(2, 1)], 5: [(0, 3), (2, 1)], 6: [(2, 0)], 7: [(2, 3)], 8: [(3, 2)],
         9: [(0, 2)], 10: [(1, 0), (3, 2)], 11: [(1, 2)], 12: [(3, 1)], 13: [(0, 1)], 14: [(3, 0)], 15: []}
JOINED = {5: [(0, 1), (2, 3)], 10: [(3, 0), (1, 2)]}


def contour64(fields, window, n, tol=1e-13):
    """``fields(x, y) -> (D, beta_x, beta_y, 1 - kappa)`` on float64 arrays.  Returns a dict: ``seg``, ``cau`` [K, 2, 2], ``kind``
    [K], ``edges`` (crossing edge id -> refined (x, y, beta_x, beta_y, 1 - kappa)), ``D`` (vertex plane), ``open``, ``n_flagged``,
    ``n_ambiguous`` and ``area`` (tangential, radial in the image plane, then in the source plane; signed as the native call)."""
    x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
    hx, hy = (x_hi - x_lo) / n, (y_hi - y_lo) / n
    xs, ys = x_lo + np.arange(n + 1) * hx, y_lo + np.arange(n + 1) * hy
    X, Y = np.meshgrid(xs, ys)  # [row = y, col = x]
    D = fields(X.ravel(), Y.ravel())[0].reshape(n + 1, n + 1)
    D = np.where(np.isfinite(D), D, np.nan)
    fin, neg = np.isfinite(D), np.nan_to_num(D, nan=1.0) < 0
    H = (n + 1) * n
    hz = fin[:, :-1] & fin[:, 1:] & (neg[:, :-1] != neg[:, 1:])  # [n+1, n]
    vt = fin[:-1, :] & fin[1:, :] & (neg[:-1, :] != neg[1:, :])  # [n, n+1]
    ids = np.concatenate([np.flatnonzero(hz.ravel()), H + np.flatnonzero(vt.ravel())])
    is_h = ids < H
    r = np.where(is_h, ids // n, (ids - H) // (n + 1))
    c = np.where(is_h, ids % n, (ids - H) % (n + 1))
    x0, y0, length = xs[c], ys[r], np.where(is_h, hx, hy)
    neg0 = neg[r, c]
    t_lo, t_hi = np.zeros(len(ids)), np.ones(len(ids))
    point = lambda t: (np.where(is_h, x0 + t * length, x0), np.where(is_h, y0, y0 + t * length))
    while len(ids) and np.max((t_hi - t_lo) * length) > tol:
        t = 0.5 * (t_lo + t_hi)
        d = fields(*point(t))[0]
        same = (d < 0) == neg0
        t_lo, t_hi = np.where(same, t, t_lo), np.where(same, t_hi, t)
    px, py = point(0.5 * (t_lo + t_hi))
    edges = {}
    if len(ids):
        _, bx, by, omk = fields(px, py)
        edges = {int(e): (px[k], py[k], bx[k], by[k], omk[k]) for k, e in enumerate(ids)}
    is_open = bool(hz[0].any() or hz[n].any() or vt[:, 0].any() or vt[:, n].any())
    seg, cau, kind = [], [], []
    n_flagged = n_ambiguous = 0
    area = np.zeros(4)
    cx = 0.5 * (x_lo + x_hi)
    cell_fin = fin[:-1, :-1] & fin[:-1, 1:] & fin[1:, 1:] & fin[1:, :-1]
    code = neg[:-1, :-1] * 1 + neg[:-1, 1:] * 2 + neg[1:, 1:] * 4 + neg[1:, :-1] * 8
    for rr, cc in zip(*np.nonzero(~cell_fin)):
        d = np.array([D[rr, cc], D[rr, cc + 1], D[rr + 1, cc + 1], D[rr + 1, cc]])
        f = d[np.isfinite(d)]
        n_flagged += int(len(f) > 0 and (f < 0).any() and not (f < 0).all())
    for rr, cc in zip(*np.nonzero(cell_fin & (code > 0) & (code < 15))):  # row-major
        k = int(code[rr, cc])
        pairs = CASES[k]
        if k in JOINED:
            n_ambiguous += 1
            if 0.25 * (D[rr, cc] + D[rr, cc + 1] + D[rr + 1, cc + 1] + D[rr + 1, cc]) < 0:
                pairs = JOINED[k]
        cell_edge = [rr * n + cc, H + rr * (n + 1) + cc + 1, (rr + 1) * n + cc, H + rr * (n + 1) + cc]
        for a, b in pairs:
            p1, p2 = edges[cell_edge[a]], edges[cell_edge[b]]
            seg.append([[p1[0], p1[1]], [p2[0], p2[1]]])
            cau.append([[p1[2], p1[3]], [p2[2], p2[3]]])
            kd = 0 if p1[4] + p2[4] > 0 else 1
            kind.append(kd)
            area[kd] += 0.5 * ((p1[0] - cx) + (p2[0] - cx)) * (p2[1] - p1[1])
            area[2 + kd] += 0.5 * ((p1[2] - cx) + (p2[2] - cx)) * (p2[3] - p1[3])
    return {"seg": np.array(seg).reshape(-1, 2, 2), "cau": np.array(cau).reshape(-1, 2, 2), "kind": np.array(kind, dtype=np.int64),
            "edges": edges, "D": D, "open": is_open, "n_flagged": n_flagged, "n_ambiguous": n_ambiguous, "area": area}


def sis_fields(theta_E, cx, cy):
    """Closed form of the SIS: D = 1 - theta_E / r, beta = theta - theta_E theta_hat, 1 - kappa = 1 - theta_E / (2 r)."""
    def fields(x, y):
        dx, dy = np.asarray(x, np.float64) - cx, np.asarray(y, np.float64) - cy
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.hypot(dx, dy)
            return 1 - theta_E / r, x - theta_E * dx / r, y - theta_E * dy / r, 1 - 0.5 * theta_E / r
    return fields


def oracle_fields(phys, lens_rows, b):
    """float64 fields of sample ``b`` from the oracle's restatement of every profile (``oracle.ref_torch.mass_deriv`` and
    ``mass_hessian``, summed over the lenses).  ``lens_rows``: per-lens dicts of float64 CPU columns."""
    import torch
    from oracle import ref_torch as ref

    def hessian(x, y):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))
        y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64))
        ax = ay = fxx = fxy = fyx = fyy = 0
        for prof, p, c in zip(phys.lenses, lens_rows, phys.lenses_constants):
            kw = {k: v[b] for k, v in p.items()}
            kw.update({k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(torch.float64) for k, v in c.items()})
            with torch.no_grad():
                dx, dy = ref.mass_deriv(prof, x, y, **kw)
            h = [t.detach() for t in ref.mass_hessian(prof, x, y, **kw)]
            ax, ay = ax + dx, ay + dy
            fxx, fxy, fyx, fyy = fxx + h[0], fxy + h[1], fyx + h[2], fyy + h[3]
        to = lambda t: t.numpy() if torch.is_tensor(t) else np.zeros(x.shape)
        return x.numpy() - to(ax), y.numpy() - to(ay), to(fxx), to(fxy), to(fyx), to(fyy)

    def fields(x, y):
        bx, by, fxx, fxy, fyx, fyy = hessian(x, y)
        return (1 - fxx) * (1 - fyy) - fxy * fyx, bx, by, 1 - 0.5 * (fxx + fyy)
    fields.hessian = hessian
    return fields


def grad_D(fields, x, y, step=1e-6):
    """|grad D| by central differences in float64."""
    gx = (fields(x + step, y)[0] - fields(x - step, y)[0]) / (2 * step)
    gy = (fields(x, y + step)[0] - fields(x, y - step)[0]) / (2 * step)
    return np.hypot(gx, gy)


def count_loops(seg):
    """Number of closed loops and of open arcs of a segment soup whose shared endpoints are bitwise equal."""
    from gigalens_amd.simulator import LensSimulator
    res = {"critical": seg[None], "caustic": seg[None], "kind": np.zeros((1, len(seg)), np.int64), "n": np.array([len(seg)])}
    chains = LensSimulator.chain_curves(res, 0)
    return sum(1 for c in chains if c[1]), sum(1 for c in chains if not c[1])
