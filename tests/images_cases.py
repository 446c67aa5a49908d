"""float64 restatements for the lens-equation solver (gl_image_positions): the scan stage in numpy, and the float64 Newton
reference on the oracle's deflections that the GPU tests compare the final images with.

`scan64` follows gl_img_scan_kernel / img_tri_hit step by step: beta at the (n+1)^2 vertices of the grid (row-major, y rows), moved
to the plane of a source with deflection scale c as theta + c (beta - theta); cell (ci, cj) holds triangle k = 0: (v00, v10, v11)
and k = 1: (v00, v11, v01); the edge function of every edge is evaluated with the vertex of lower index first and negated when the
triangle walks the edge the other way; a triangle whose signed area W (the sum of its three edge functions) is zero or not finite
-- a flagged (NaN) vertex makes it so -- is skipped; after orientation by the sign of W a source is inside when every edge function
is > 0, and on an edge (== 0) it belongs to the triangle whose oriented direction d along that edge has d.y > 0, or d.y == 0 and
d.x > 0.  Hits are listed in triangle order with the barycentric preimage of the source as the seed, and counted per wave of the
kernel's quartering (wave w walks triangles [w per, (w + 1) per), per = ceil(2 n^2 / 4)).

On dyadic inputs (grid, map and source exactly representable with a few bits) every product and sum above is exact in float32
and in float64 alike, so the restatement and the kernel must agree bit for bit: that is what makes the tie rule testable.

The window the scan claims is HALF-OPEN.  A boundary side belongs to one triangle only, which walks it counter-clockwise around the
window (bottom: +x, right: +y, top: -x, left: -y); it is claimed when that triangle owns it: with A the Jacobian of the map and
u the counter-clockwise direction, d = sign(det A) A u must have d.y > 0, or d.y == 0 and d.x > 0.  Opposite sides have opposite
u, so exactly one of bottom / top and one of left / right is claimed; a corner is claimed when both sides that meet there are.
For the identity: bottom (y = y_lo) and right (x = x_hi), the corner (x_hi, y_lo) with them, the other three corners not.
`claimed_sides` states this rule on its own, without the triangles."""
import math

import numpy as np

IMG_MAXC = 64  # candidates per (sample, source), gl_images.hip.h
NW = 4         # waves of the scan workgroup


def grid_vertices(window, n):
    x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
    hx, hy = (x_hi - x_lo) / n, (y_hi - y_lo) / n
    return x_lo + np.arange(n + 1) * hx, y_lo + np.arange(n + 1) * hy


def scan64(beta, window, n, sx, sy, scale=1.0):
    """``beta(x, y) -> (bx, by)`` on float64 arrays (the reference plane's map).  Returns a dict: ``hits`` (triangle ids, ascending),
    ``seeds`` [K, 2], ``per_wave`` (hits of each of the four waves), ``n_cand``, ``n_over`` as the kernel stores them, and
    ``margin``: per triangle, the distance (source plane) by which its inside / outside decision holds -- for a hit the smallest
    oriented edge distance, for a miss the largest distance outside an edge; NaN for skipped triangles, 0 where a tie decided."""
    xs, ys = grid_vertices(window, n)
    X, Y = np.meshgrid(xs, ys)
    with np.errstate(all="ignore"):
        bx, by = beta(X, Y)
        bx, by = np.asarray(bx, np.float64), np.asarray(by, np.float64)
        bad = ~(np.isfinite(bx) & np.isfinite(by))
        bx, by = np.where(bad, np.nan, bx), np.where(bad, np.nan, by)
        if scale != 1.0:
            bx, by = X + scale * (bx - X), Y + scale * (by - Y)
    bx, by = bx.ravel(), by.ravel()
    V1, T = n + 1, 2 * n * n
    t = np.arange(T)
    cell, k = t >> 1, t & 1
    cj, ci = cell // n, cell % n
    v00 = cj * V1 + ci
    vi = np.stack([v00, np.where(k == 1, v00 + V1 + 1, v00 + 1), np.where(k == 1, v00 + V1, v00 + V1 + 1)])
    w, dx, dy = np.empty((3, T)), np.empty((3, T)), np.empty((3, T))
    with np.errstate(all="ignore"):
        for e in range(3):
            p, q = vi[e], vi[(e + 1) % 3]
            fwd = p < q
            lo, hi = np.where(fwd, p, q), np.where(fwd, q, p)
            f = np.where(fwd, 1.0, -1.0)
            w[e] = f * ((bx[hi] - bx[lo]) * (sy - by[lo]) - (by[hi] - by[lo]) * (sx - bx[lo]))
            dx[e], dy[e] = f * (bx[hi] - bx[lo]), f * (by[hi] - by[lo])
        W = w[0] + w[1] + w[2]
        live = np.isfinite(W) & (W != 0)
        o = np.where(W > 0, 1.0, -1.0)
        we, dex, dey = o * w, o * dx, o * dy
        owned = (dey > 0) | ((dey == 0) & (dex > 0))
        inside = live & np.all((we > 0) | ((we == 0) & owned), axis=0)
        dist = we / np.hypot(dx, dy)
        margin = np.where(inside, dist.min(0), (-dist).max(0))
        margin = np.where(live, margin, np.nan)
        hits = np.flatnonzero(inside)
        l0, l1, l2 = (w[1] / W)[hits], (w[2] / W)[hits], (w[0] / W)[hits]
    x0, x1, y0, y1 = xs[ci[hits]], xs[ci[hits] + 1], ys[cj[hits]], ys[cj[hits] + 1]
    kk = k[hits] == 1
    seeds = np.stack([l0 * x0 + l1 * x1 + l2 * np.where(kk, x0, x1), l0 * y0 + l1 * np.where(kk, y1, y0) + l2 * y1], 1)
    per = (T + NW - 1) // NW
    per_wave = [int(np.sum((hits >= wv * per) & (hits < min(T, (wv + 1) * per)))) for wv in range(NW)]
    n_cand = min(sum(min(c, IMG_MAXC) for c in per_wave), IMG_MAXC)
    return {"hits": hits, "seeds": seeds, "per_wave": per_wave, "n_cand": n_cand, "n_over": len(hits) - n_cand, "margin": margin}


def claimed_sides(jac):
    """Which sides of the window the scan claims under a linear map with Jacobian ``jac`` [[a, b], [c, d]] (module docstring):
    a dict bottom / right / top / left -> bool."""
    (a, b), (c, d) = jac
    s = 1.0 if a * d - b * c > 0 else -1.0
    out = {}
    for name, (ux, uy) in (("bottom", (1, 0)), ("right", (0, 1)), ("top", (-1, 0)), ("left", (0, -1))):
        ex, ey = s * (a * ux + b * uy), s * (c * ux + d * uy)
        out[name] = ey > 0 or (ey == 0 and ex > 0)
    return out


def boundary_claim(jac, window, x, y):
    """0 or 1: is the boundary point (x, y) of the window claimed under the linear map (sides from ``claimed_sides``; a corner needs both)?"""
    x_lo, x_hi, y_lo, y_hi = window
    sides = claimed_sides(jac)
    on = [name for name, hit in (("bottom", y == y_lo), ("right", x == x_hi), ("top", y == y_hi), ("left", x == x_lo)) if hit]
    assert on, (x, y)
    return int(all(sides[name] for name in on))


# ---- the linear maps of the tie-rule tests: a Shear alone, alpha = (g1 x + g2 y, g2 x - g1 y), on the plane of scale c ----------
SHEAR_MAPS = [(0.0, 0.0), (0.0, 0.5), (1.5, 0.0)]


def shear_jacobian(g1, g2, c=1.0):
    return ((1.0 - c * g1, -c * g2), (-c * g2, 1.0 + c * g1))


def shear_beta(g1, g2):
    """The reference-plane map of the Shear (scan64 moves it to the plane of scale c itself, as the kernel does)."""
    return lambda x, y: (x - (g1 * x + g2 * y), y - (g2 * x - g1 * y))


def apply_jac(jac, x, y):
    (a, b), (c, d) = jac
    return a * x + b * y, c * x + d * y


def quarter_lattice(window, n):
    """theta on the quarter-cell lattice of the grid (vertices, edge and diagonal midpoints, interiors): x [K], y [K], boundary [K]."""
    x_lo, x_hi, y_lo, y_hi = (float(v) for v in window)
    qx = x_lo + np.arange(4 * n + 1) * ((x_hi - x_lo) / (4 * n))
    qy = y_lo + np.arange(4 * n + 1) * ((y_hi - y_lo) / (4 * n))
    X, Y = (a.ravel() for a in np.meshgrid(qx, qy))
    return X, Y, (X == x_lo) | (X == x_hi) | (Y == y_lo) | (Y == y_hi)


def triangle_centroids(window, n):
    """Centroids of the 2 n^2 triangles in the kernel's order: x [T], y [T]."""
    xs, ys = grid_vertices(window, n)
    t = np.arange(2 * n * n)
    cell, k = t >> 1, t & 1
    cj, ci = cell // n, cell % n
    x0, x1, y0, y1 = xs[ci], xs[ci + 1], ys[cj], ys[cj + 1]
    return (x0 + x1 + np.where(k == 1, x0, x1)) / 3, (y0 + np.where(k == 1, y1, y0) + y1) / 3


def sis_beta(theta_E, cx, cy):
    def beta(x, y):
        dx, dy = x - cx, y - cy
        r = np.hypot(dx, dy)
        return x - theta_E * dx / r, y - theta_E * dy / r
    return beta


# SIS centres (float32 values; theta_E = 1, window (-2, 2)^2) for the candidate-list tests, a source bit-identically on the centre:
# grid -> (center_x, center_y).  Picked on the CPU so that every triangle's decision holds by at least RING_MARGIN in float64
# (tests/test_images_host.py asserts it, and the hit counts beside them).
RING_MARGIN = 1e-5
RING_WINDOW = (-2.0, 2.0, -2.0, 2.0)
# n: (centre, hits, hits per wave).  16: below the list; 32: no wave above 64 but 65 in all (the concatenation clip); 72: two waves
# above 64 (the in-wave clip).  The margin of a source on the centre shrinks like the cube of the cell side (an edge along a grid
# line that passes the centre at distance delta maps to a chord at ~ delta h^2 from it): 5.2e-5, 1.9e-5 and 1.26e-5 here; no centre
# on a 1e-4 lattice within +-0.06 reaches 1e-5 at n = 96 (best 4.2e-6 of 3000 draws), so the in-wave grid is 72, not 96.
RING_CASES = {16: ((0.013, -0.021), 29, [1, 15, 13, 0]),
              32: ((0.013, -0.021), 65, [5, 31, 29, 0]),
              72: ((0.0193, -0.0189), 145, [9, 65, 71, 0])}


def ring_scan(n):
    """scan64 of RING_CASES[n] on the float32 values of its centre, and those values."""
    (cx, cy), _, _ = RING_CASES[n]
    cx, cy = float(np.float32(cx)), float(np.float32(cy))
    return scan64(sis_beta(1.0, cx, cy), RING_WINDOW, n, cx, cy), cx, cy


# ---- float64 Newton reference on the oracle's deflections (moved here unchanged from tests/test_gpu_image_positions.py) ---------
EPS32 = float(np.finfo(np.float32).eps)


def _lens_rows(sim, packed):
    """Per-lens dicts of float64 CPU columns (the oracle's view of the packed rows)."""
    from tests import helpers as H
    struct = H.struct_from_packed(sim.phys_model, packed.detach().double().cpu())
    return struct["lens_mass"]


def _deriv64(sim, lens_rows, b):
    """float64 deflection (sum over the lenses) of sample b, on the oracle's restatement of every profile."""
    import torch
    from oracle import ref_torch as ref
    phys = sim.phys_model

    def f(x, y):
        ax = ay = 0
        for prof, p, c in zip(phys.lenses, lens_rows, phys.lenses_constants):
            kw = {k: v[b] for k, v in p.items()}
            kw.update({k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(torch.float64) for k, v in c.items()})
            fx, fy = ref.mass_deriv(prof, x, y, **kw)
            ax, ay = ax + fx, ay + fy
        return ax, ay
    return f


def _beta_jac(deriv, x, y):
    import torch
    x = x.detach().clone().requires_grad_(True)
    y = y.detach().clone().requires_grad_(True)
    ax, ay = deriv(x, y)
    gxx, gxy = torch.autograd.grad(ax.sum(), (x, y), retain_graph=True)
    gyx, gyy = torch.autograd.grad(ay.sum(), (x, y))
    return (x - ax).detach(), (y - ay).detach(), gxx, gxy, gyx, gyy


def _solve64(deriv, sx, sy, window, n):
    """float64 reference: seeds = centroids of the triangles of an n x n grid whose source-plane image contains the source,
    then Newton to 1e-11; duplicates (1e-6) merged; images outside the window dropped.  Returns [K, 3] (x, y, mu) sorted by x."""
    import torch
    F64 = torch.float64
    x_lo, x_hi, y_lo, y_hi = window
    xs = torch.linspace(x_lo, x_hi, n + 1, dtype=F64)
    ys = torch.linspace(y_lo, y_hi, n + 1, dtype=F64)
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    with torch.no_grad():
        ax, ay = deriv(X.reshape(-1), Y.reshape(-1))
    bx, by = (X.reshape(-1) - ax).reshape(n + 1, n + 1), (Y.reshape(-1) - ay).reshape(n + 1, n + 1)
    v = lambda t, dj, di: t[dj:dj + n, di:di + n].reshape(-1)
    pos = lambda t, dj, di: t[dj:dj + n, di:di + n].reshape(-1)
    tris = [((0, 0), (0, 1), (1, 1)), ((0, 0), (1, 1), (1, 0))]
    seeds_x, seeds_y = [], []
    for tri in tris:
        P = [(v(bx, *o), v(by, *o)) for o in tri]
        cross = []
        for e in range(3):
            (px, py), (qx, qy) = P[e], P[(e + 1) % 3]
            cross.append((qx - px) * (sy - py) - (qy - py) * (sx - px))
        inside = ((cross[0] > 0) & (cross[1] > 0) & (cross[2] > 0)) | ((cross[0] < 0) & (cross[1] < 0) & (cross[2] < 0))
        inside &= torch.isfinite(cross[0] + cross[1] + cross[2])
        seeds_x.append(sum(pos(X, *o) for o in tri)[inside] / 3)
        seeds_y.append(sum(pos(Y, *o) for o in tri)[inside] / 3)
    x, y = torch.cat(seeds_x), torch.cat(seeds_y)
    for _ in range(60):
        b_x, b_y, fxx, fxy, fyx, fyy = _beta_jac(deriv, x, y)
        rx, ry = sx - b_x, sy - b_y
        a00, a01, a10, a11 = 1 - fxx, -fxy, -fyx, 1 - fyy
        det = a00 * a11 - a01 * a10
        dx, dy = (a11 * rx - a01 * ry) / det, (a00 * ry - a10 * rx) / det
        step = torch.hypot(dx, dy).clamp(min=1e-300)
        lim = torch.clamp(0.2 / step, max=1.0)
        x, y = x + dx * lim, y + dy * lim
    b_x, b_y, fxx, fxy, fyx, fyy = _beta_jac(deriv, x, y)
    ok = (torch.hypot(sx - b_x, sy - b_y) < 1e-11) & (x >= x_lo) & (x <= x_hi) & (y >= y_lo) & (y <= y_hi)
    mu = 1 / ((1 - fxx) * (1 - fyy) - fxy * fyx)
    found = []
    for xi, yi, mi in zip(x[ok].tolist(), y[ok].tolist(), mu[ok].tolist()):
        if all(math.hypot(xi - a, yi - b) > 1e-6 for a, b, _ in found):
            found.append((xi, yi, mi))
    return np.array(sorted(found), dtype=np.float64).reshape(-1, 3)


def _default_tol(window):
    from gigalens_amd.simulator import LensSimulator
    return LensSimulator.IMAGE_TOL_EPS * EPS32 * max(abs(v) for v in window)


def _residual64(deriv, x, y, sx, sy):
    import torch
    with torch.no_grad():
        ax, ay = deriv(torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64))
    return np.hypot(np.asarray(x, np.float64) - ax.numpy() - sx, np.asarray(y, np.float64) - ay.numpy() - sy)


def _check_against_f64(sim, packed, srcx, srcy, window, n_cells, mu_min=0.02, fold_cells=2.0):
    """Compare the solver's images with the float64 solver; returns (number of (sample, source) pairs compared, counts seen)."""
    x, y, mu, n = sim.image_positions(packed, srcx, srcy, window=window, num_cells=n_cells)
    x, y, mu, n = (t.cpu().numpy() for t in (x, y, mu, n))
    rows = _lens_rows(sim, packed)
    tol = _default_tol(window)
    cell = (window[1] - window[0]) / n_cells
    compared, counts = 0, []
    for b in range(packed.shape[0]):
        deriv = _deriv64(sim, rows, b)
        for s in range(srcx.shape[1]):
            sx, sy = float(srcx[b, s]), float(srcy[b, s])
            ref = _solve64(deriv, sx, sy, window, 2 * n_cells)
            k = int(n[b, s])
            got = np.stack([x[b, s, :k], y[b, s, :k], mu[b, s, :k]], axis=1)
            assert np.all(np.isfinite(got)) and np.all(np.isnan(x[b, s, k:]))
            # lens-equation residual of every returned image, in float64
            res = _residual64(deriv, got[:, 0], got[:, 1], sx, sy)
            assert np.all(res <= 2 * tol), (b, s, res, tol)
            # what the solver does not promise: two images closer than ~a cell at a fold
            if len(ref) > 1:
                d = np.hypot(ref[:, None, 0] - ref[None, :, 0], ref[:, None, 1] - ref[None, :, 1]) + np.eye(len(ref)) * 1e9
                if d.min() < fold_cells * cell:
                    continue
            # highly demagnified central images sit within a cell of a cusp or singularity: compared above mu_min
            ref_m, got_m = ref[np.abs(ref[:, 2]) >= mu_min], got[np.abs(got[:, 2]) >= mu_min]
            assert len(ref_m) == len(got_m), (b, s, ref, got)
            for r in ref_m:
                j = np.argmin(np.hypot(got_m[:, 0] - r[0], got_m[:, 1] - r[1]))
                # (beyond |mu| = 30 the root itself is conditioned by mu: float32 rounding of beta times |mu|)
                assert math.hypot(got_m[j, 0] - r[0], got_m[j, 1] - r[1]) <= max(5e-5, 2e-6 * abs(r[2])), (b, s, r, got_m[j])
                if abs(r[2]) < 30:
                    assert abs(got_m[j, 2] - r[2]) <= 1e-3 * abs(r[2]), (b, s, r, got_m[j])
            compared += 1
            counts.append(len(ref_m))
    return compared, counts
