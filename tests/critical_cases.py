"""float64 restatement of the critical-curve contouring (gl_critical_curves) in numpy, and the float64 fields it runs on.

`contour64` follows the specification of the native call step by step: D = det(I - H) at the (n+1)^2 vertices of a regular grid;
an edge whose two finite endpoint values differ in sign (sign = D < 0) is crossing and is bisected ON the edge; marching squares
per cell in row-major order with D < 0 on the left of every segment; the ambiguous cases joined when the mean of the four vertex
values is < 0; a segment is tangential when the mean of 1 - kappa at its endpoints is > 0.

The 16-case table below is, by design, the table the kernel uses: the restatement is independent of the kernel in its numerics
(float64 fields from the oracle), its edge listing, bisection and ordering, not in the table.  The table is pinned independently,
row by row: `orientation_violations` checks D < 0 on the left of every segment from the vertex plane alone, `physical_loops`
counts the closed curves without contouring (the joined rows 16 and 17 against the separated rows 5 and 10, on the AMBIGUOUS
cases), and the closed-form tests fix the overall sign (SIS: one loop of positive area pi theta_E^2; NFW: a radial loop inside
the tangential one).  `with_capacity` restates the overflow accounting of a call with too few segment or edge slots.

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
    [K], ``seg_edges`` [K, 2] (the grid edges that carry the two endpoints), ``edges`` (crossing edge id -> refined (x, y, beta_x, beta_y, 1 - kappa)), ``D`` (vertex plane), ``open``, ``n_flagged``,
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
    seg, cau, kind, seg_edges = [], [], [], []
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
            seg_edges.append((cell_edge[a], cell_edge[b]))
            area[kd] += 0.5 * ((p1[0] - cx) + (p2[0] - cx)) * (p2[1] - p1[1])
            area[2 + kd] += 0.5 * ((p1[2] - cx) + (p2[2] - cx)) * (p2[3] - p1[3])
    return {"seg": np.array(seg).reshape(-1, 2, 2), "cau": np.array(cau).reshape(-1, 2, 2), "kind": np.array(kind, dtype=np.int64),
            "seg_edges": np.array(seg_edges, dtype=np.int64).reshape(-1, 2), "edges": edges, "D": D, "open": is_open, "n_flagged": n_flagged, "n_ambiguous": n_ambiguous, "area": area}


def sis_fields(theta_E, cx, cy):
    """Closed form of the SIS: D = 1 - theta_E / r, beta = theta - theta_E theta_hat, 1 - kappa = 1 - theta_E / (2 r)."""
    def fields(x, y):
        dx, dy = np.asarray(x, np.float64) - cx, np.asarray(y, np.float64) - cy
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.hypot(dx, dy)
            return 1 - theta_E / r, x - theta_E * dx / r, y - theta_E * dy / r, 1 - 0.5 * theta_E / r
    return fields


def multi_sis_fields(lenses, scale=1.0):
    """Closed form of a sum of SIS lenses ``[(theta_E, cx, cy), ...]`` on the plane of deflection scale ``scale``:
    alpha = theta_E r_hat, H = theta_E / r^3 [[dy^2, -dx dy], [-dx dy, dx^2]], kappa = theta_E / (2 r), each times ``scale``."""
    def fields(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        ax = ay = fxx = fxy = fyy = kap = 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            for te, cx, cy in lenses:
                dx, dy = x - cx, y - cy
                r = np.hypot(dx, dy)
                ax, ay = ax + te * dx / r, ay + te * dy / r
                fxx, fxy, fyy = fxx + te * dy * dy / r ** 3, fxy - te * dx * dy / r ** 3, fyy + te * dx * dx / r ** 3
                kap = kap + 0.5 * te / r
            fxx, fxy, fyy, kap = scale * fxx, scale * fxy, scale * fyy, scale * kap
            return (1 - fxx) * (1 - fyy) - fxy * fxy, x - scale * ax, y - scale * ay, 1 - kap
    return fields


def scaled_fields(fields, scale):
    """The fields of the source plane with deflection scale c from oracle fields that carry ``hessian``: D = det(I - c H),
    beta = theta - c sum alpha, 1 - c kappa."""
    def out(x, y):
        bx, by, fxx, fxy, fyx, fyy = fields.hessian(x, y)
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return ((1 - scale * fxx) * (1 - scale * fyy) - scale * scale * fxy * fyx, x + scale * (bx - x), y + scale * (by - y),
                1 - 0.5 * scale * (fxx + fyy))

    def hessian(x, y):
        bx, by, fxx, fxy, fyx, fyy = fields.hessian(x, y)
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return x + scale * (bx - x), y + scale * (by - y), scale * fxx, scale * fxy, scale * fyx, scale * fyy
    out.hessian = hessian
    return out


def cell_codes(D):
    """Marching-squares code of every cell of a vertex plane (corner bits as CASES has them); -1 where a vertex is not finite."""
    fin, neg = np.isfinite(D), np.nan_to_num(D, nan=1.0) < 0
    code = neg[:-1, :-1] * 1 + neg[:-1, 1:] * 2 + neg[1:, 1:] * 4 + neg[1:, :-1] * 8
    return np.where(fin[:-1, :-1] & fin[:-1, 1:] & fin[1:, 1:] & fin[1:, :-1], code, -1)


def ambiguous_cells(D):
    """[(row, col, code, joined, margin)] of the cells with code 5 or 10: ``joined`` = mean of the four vertex values < 0, ``margin``
    = the smallest of |mean| and the four |vertex value|."""
    out = []
    code = cell_codes(D)
    for r, c in zip(*np.nonzero((code == 5) | (code == 10))):
        d = np.array([D[r, c], D[r, c + 1], D[r + 1, c + 1], D[r + 1, c]])
        out.append((int(r), int(c), int(code[r, c]), bool(d.mean() < 0), float(min(abs(d.mean()), np.abs(d).min()))))
    return out


def edge_of(p, window, n):
    """Id of the grid edge that carries the point p: the coordinate that sits on a grid line (to 2e-5 of a cell: the float32 grid of
    the kernel is off the float64 one by a few 1e-6 of a cell at 127 cells) says which; horizontal edges first, row by row."""
    x_lo, x_hi, y_lo, y_hi = window
    fx, fy = (p[0] - x_lo) / ((x_hi - x_lo) / n), (p[1] - y_lo) / ((y_hi - y_lo) / n)
    ox, oy = abs(fx - round(fx)), abs(fy - round(fy))
    assert min(ox, oy) < 2e-5, p
    if oy <= ox:  # y on a grid line: a horizontal edge
        return int(round(fy)) * n + min(max(int(np.floor(fx)), 0), n - 1)
    return (n + 1) * n + min(max(int(np.floor(fy)), 0), n - 1) * (n + 1) + int(round(fx))


def orientation_violations(seg, D, window, n):
    """Independently of the table: D < 0 lies on the LEFT of every directed segment.  For each endpoint take the D < 0 vertex of the
    grid edge that carries it (from the float64 vertex plane ``D``); cross(p2 - p1, v_neg - p1) must be > 0.  Returns the offenders."""
    x_lo, x_hi, y_lo, y_hi = window
    hx, hy = (x_hi - x_lo) / n, (y_hi - y_lo) / n
    H, bad = (n + 1) * n, []
    for s, (p1, p2) in enumerate(np.asarray(seg, np.float64)):
        for p in (p1, p2):
            e = edge_of(p, window, n)
            if e < H:
                r, c = divmod(e, n)
                ends = [(r, c), (r, c + 1)]
            else:
                r, c = divmod(e - H, n + 1)
                ends = [(r, c), (r + 1, c)]
            neg = [v for v in ends if D[v] < 0]
            assert len(neg) == 1, (s, e, [D[v] for v in ends])
            vx, vy = x_lo + neg[0][1] * hx, y_lo + neg[0][0] * hy
            cross = (p2[0] - p1[0]) * (vy - p1[1]) - (p2[1] - p1[1]) * (vx - p1[0])
            if not cross > 0:
                bad.append((s, e, cross))
    return bad


def _components(mask):
    """Number of 4-connected regions of a boolean plane."""
    n_r, n_c = mask.shape
    seen, regions = np.zeros_like(mask), 0
    for r0, c0 in zip(*np.nonzero(mask)):
        if seen[r0, c0]:
            continue
        regions += 1
        stack = [(r0, c0)]
        seen[r0, c0] = True
        while stack:
            r, c = stack.pop()
            for rr, cc in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)):
                if 0 <= rr < n_r and 0 <= cc < n_c and mask[rr, cc] and not seen[rr, cc]:
                    seen[rr, cc] = True
                    stack.append((rr, cc))
    return regions


def physical_loops(fields, window, n_fine=256):
    """The number of closed critical curves inside the window, found without contouring: the regions of D < 0 and of D >= 0 on a
    fine grid of cell centres (4-connectivity) are the nodes of a tree whose links are the curves between them (closed curves nest),
    so their number is regions - 1.  Returns (curves, regions of D < 0)."""
    x_lo, x_hi, y_lo, y_hi = window
    xs = x_lo + (np.arange(n_fine) + 0.5) * (x_hi - x_lo) / n_fine
    ys = y_lo + (np.arange(n_fine) + 0.5) * (y_hi - y_lo) / n_fine
    X, Y = np.meshgrid(xs, ys)
    neg = np.nan_to_num(fields(X.ravel(), Y.ravel())[0].reshape(n_fine, n_fine), nan=-1.0) < 0
    n_neg = _components(neg)
    return n_neg + _components(~neg) - 1, n_neg


# Two SIS lenses whose critical curves nearly touch along the (1, 1) diagonal (code 5) or the (1, -1) diagonal (code 10), one sample
# per variant of the ambiguous cell, found by a random search with hill climbing on the margin (window (-3, 3)^2, 12 cells, i.e.
# cells of 0.5): name -> (lenses [(theta_E, cx, cy)] as float32 values, code, joined, closed curves).  Separated: the mean of the
# four vertex values is > 0 and the two D < 0 regions stay apart (two curves); joined: it is < 0 and they are one region (one curve).
AMBIGUOUS_WINDOW, AMBIGUOUS_N, AMBIGUOUS_MARGIN = (-3.0, 3.0, -3.0, 3.0), 12, 5e-3
AMBIGUOUS = {
    "code5_separated": ([(0.5378, -1.0550, -1.0400), (0.5381, 0.5871, 0.5170)], 5, False, 2),
    "code5_joined": ([(0.5, -0.5200, -0.5266), (0.5, 0.8072, 0.8104)], 5, True, 1),
    "code10_separated": ([(0.5009, -0.9036, 1.0759), (0.5028, 0.5240, -0.4852)], 10, False, 2),
    "code10_joined": ([(0.5, -0.8155, 0.8259), (0.5, 0.4905, -0.5028)], 10, True, 1),
}


def ambiguous_case(name):
    """(lenses as the float64 values of their float32 parameters, code, joined, curves) of AMBIGUOUS[name]."""
    lenses, code, joined, curves = AMBIGUOUS[name]
    return [tuple(float(np.float32(v)) for v in lens) for lens in lenses], code, joined, curves


def with_capacity(ref, max_segments):
    """What the native call returns of the contour ``ref`` (contour64) with room for ``max_segments`` segments and 2 max_segments
    crossing edges: the edge list keeps the smallest ids; the first min(T, max_segments) segments in cell order take their slots,
    a slot whose endpoint's edge was not kept is padding and counts as dropped, as does every segment beyond the slots.
    Returns (n, keep [n] bool: the slot holds its segment, n_dropped)."""
    kept = set(sorted(ref["edges"])[:2 * max_segments])
    T = len(ref["seg"])
    n = min(T, max_segments)
    keep = np.array([a in kept and b in kept for a, b in ref["seg_edges"][:n].tolist()], dtype=bool).reshape(n)
    return n, keep, (T - n) + int((~keep).sum())


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
