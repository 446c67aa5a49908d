"""Critical curves, caustics and the effective Einstein radius on lens planes (csrc/gl_multiplane_critical.hip.h;
``LensSimulator.critical_curves / einstein_radius(source_redshifts=...)``) on the GPU, against the closed form (SIS | Shear) and
``critical_cases.contour64`` on the float64 recursion fields of tests/mp_critical_cases.py.

Gates, in the form of tests/test_gpu_critical_curves.py.  Endpoint gate = 4 x yardstick + bracket: the yardstick is the float32 error
of D = det A_t from the existing multi-plane lens maps (gl_mp_maps_kernel, ``Model.multiplane_maps`` with the target's couplings) at
the returned endpoints against the float64 recursion, divided by |grad D64|; the bracket is 4 float32 spacings of the window's
largest |coordinate|, where the bisection stops.  Beta gate = 4 x the float32 beta error of the same call.  The bisection stops on a
float32 sign of D, up to one float32 error of D on either side of the root; 4 x still catches a refinement that does not converge
(one cell is 0.125: four orders of magnitude more).  Every test prints its yardsticks and maxima before it asserts.

Measured on one MI355X (the largest over the samples and sources of each case; arcsec; YARD below holds the yardsticks):
    case             yardstick D   yardstick beta   endpoint gate   endpoint distance max
    sis|shear          2.93e-7        1.77e-7          2.60e-6          5.36e-7   (radius against the closed form)
    epl_shear|sie      4.37e-7        4.26e-7          3.19e-6          7.28e-7
    nfw|dpie|sis       1.57e-6        1.09e-6          7.71e-6          1.14e-6
    nfw|dpie|sis>      1.12e-6        6.82e-7          5.97e-6          1.33e-6
    shared             1.38e-7        9.24e-8          2.00e-6          5.49e-7
    dpis|sie           2.30e-7        1.60e-7          2.35e-6          6.21e-7   (D of maps_hessian at the endpoints)
    four_planes        1.55e-7        1.16e-7          2.05e-6          5.57e-7
    between the planes (epl_shear|sie, z = 0.8, against the single-plane float64 curve)     4.51e-7
Every observed distance lies below the bracket alone (1.43e-6 to 1.48e-6).  Over the four general cases 1378 crossing edges, none
differs from the float64 reference; the offset along the edge reaches 0.28 of its gate and the caustic error 0.12 of its gate.
"""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

from tests import critical_cases as CC
from tests import mp_critical_cases as C
from tests import mp_images_cases as IC
from tests import multilens_cases as MC
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
EPS32 = C.EPS32
# case -> (yardstick of D / |grad D64|, yardstick of beta), measured on the MI355X as the header says
YARD = {
    "sis|shear": (2.93e-7, 1.77e-7),
    "epl_shear|sie": (4.37e-7, 4.26e-7),
    "nfw|dpie|sis": (1.57e-6, 1.09e-6),
    "nfw|dpie|sis>": (1.12e-6, 6.82e-7),
    "shared": (1.38e-7, 9.24e-8),
    "dpis|sie": (2.30e-7, 1.60e-7),
    "four_planes": (1.55e-7, 1.16e-7),
}
_SIMS = {}


def _gates(case, window):
    bracket = 4 * EPS32 * max(abs(v) for v in window)
    return 4 * YARD[case][0] + bracket, 4 * YARD[case][1]


def _sim(gl, key, phys_mp, B):
    from gigalens_amd.simulator import SimulatorConfig
    if (key, B) not in _SIMS:
        _SIMS[key, B] = gl.LensSimulator(phys_mp, SimulatorConfig(delta_pix=0.1, num_pix=8), bs=B)
    return _SIMS[key, B]


def _lens_t(lens_params):
    return [{k: torch.as_tensor(v) for k, v in d.items()} for d in lens_params]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _maps_error(sim, packed, b, target, fields, pts, grad_D):
    """float32 error of D and of beta from gl_mp_maps_kernel at ``pts`` [K, 2] (float32) of sample b against the float64 ``fields``;
    D's divided by |grad D64| (``grad_D(fields, x, y)``)."""
    x = torch.tensor(pts[:, 0], device=sim.device)[:, None]
    y = torch.tensor(pts[:, 1], device=sim.device)[:, None]
    m = MC.as_jacobian(sim._model.multiplane_maps(packed[b:b + 1], x, y, np.asarray(target, dtype=np.float32)).double().cpu().numpy())[:, :, 0]
    d32 = m[2] * m[5] - m[3] * m[4]
    x64, y64 = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    d64, bx64, by64, _ = fields(x64, y64)
    return np.abs(d32 - d64) / grad_D(fields, x64, y64), np.hypot(m[0] - bx64, m[1] - by64)


def _got_edges(res, b, window, n_cells):
    """``({edge id: (point, caustic point)}, [[edge of end 0, edge of end 1] per segment])`` of sample b of a result."""
    n = int(res["n"][b])
    got, per_seg = {}, []
    for s in range(n):
        ids = [CC.edge_of(res["critical"][b, s, e].astype(np.float64), window, n_cells) for e in (0, 1)]
        per_seg.append(ids)
        for e in (0, 1):
            got[ids[e]] = (res["critical"][b, s, e].astype(np.float64), res["caustic"][b, s, e].astype(np.float64))
    return got, per_seg


def _compare(sim, packed, res, b, target, fields, ref, window, n_cells, case, fails, expect_closed=True):
    """Sample b of the result ``res`` of one source (numpy dict) against ``ref`` = contour64 on the float64 ``fields`` of that source's
    plane: the logic of ``test_gpu_critical_curves._compare_with_restatement`` with the yardstick from the multi-plane lens maps.
    Accuracy failures are collected in ``fails`` (every figure is printed first).  Returns (edges, differing edges, max endpoint
    distance, yardstick D, yardstick beta)."""
    endpoint_gate, beta_gate = _gates(case, window)
    n = int(res["n"][b])
    kind = res["kind"][b, :n]
    if expect_closed:
        assert not ref["open"] and ref["n_flagged"] == 0 and bool(res["closed"][b])
    hx, hy = (window[1] - window[0]) / n_cells, (window[3] - window[2]) / n_cells
    got, got_edges = _got_edges(res, b, window, n_cells)
    differ = set(got) ^ set(ref["edges"])
    common = sorted(set(got) & set(ref["edges"]))
    assert common, (case, b, n, len(ref["seg"]))
    pts = np.array([got[e][0] for e in common])
    dist = np.abs(fields(pts[:, 0], pts[:, 1])[0]) / CC.grad_D(fields, pts[:, 0], pts[:, 1])
    d_yard, b_yard = _maps_error(sim, packed, b, target, fields, pts.astype(np.float32), CC.grad_D)
    check = lambda ok, *what: None if ok else fails.append((case, b) + what)
    check(dist.max() <= endpoint_gate, "endpoint distance", dist.max(), endpoint_gate)
    # both endpoints lie on the same grid edge: their offset is measured ALONG the edge, where a distance d to the curve shows as
    # d |grad D| / |dD/dt| (the curve may cross the edge obliquely)
    ref_pts = np.array([ref["edges"][e][:2] for e in common])
    horizontal = np.array(common) < (n_cells + 1) * n_cells
    st = 1e-6
    ddt = np.where(horizontal, fields(ref_pts[:, 0] + st, ref_pts[:, 1])[0] - fields(ref_pts[:, 0] - st, ref_pts[:, 1])[0],
                   fields(ref_pts[:, 0], ref_pts[:, 1] + st)[0] - fields(ref_pts[:, 0], ref_pts[:, 1] - st)[0]) / (2 * st)
    along_gate = endpoint_gate * CC.grad_D(fields, ref_pts[:, 0], ref_pts[:, 1]) / np.abs(ddt)
    off = np.hypot(*(pts - ref_pts).T)
    check(np.all(off <= along_gate), "offset along the edge", np.max(off / along_gate))
    # caustic: beta error plus the endpoint offset carried through |d beta / d theta| <= 1 + |I - A|
    hess = np.stack(fields.hessian(ref_pts[:, 0], ref_pts[:, 1])[2:], 1)
    scale_h = 1 + np.sqrt((hess ** 2).sum(1))
    cau_err = np.hypot(*(np.array([got[e][1] for e in common]) - np.array([ref["edges"][e][2:4] for e in common])).T)
    cau_rel = np.max(cau_err / (beta_gate + scale_h * along_gate))
    check(cau_rel <= 1.0, "caustic", cau_rel)
    print(f"{case} sample {b}: {n} segments, {len(common)} edges, {len(differ)} differ, endpoint distance max {dist.max():.3e} "
          f"(gate {endpoint_gate:.3e}), along-edge offset / gate max {np.max(off / along_gate):.3f}, caustic error / gate max {cau_rel:.3f}, "
          f"yardstick D {d_yard.max():.3e}, beta {b_yard.max():.3e}")
    if not differ:  # the same segments in the same (row-major cell) order, each between the same two grid edges
        assert n == len(ref["seg"]) and np.array_equal(kind, ref["kind"]), (case, b)
        assert np.array_equal(np.array(got_edges).reshape(-1, 2), ref["seg_edges"]), (case, b)
    # where the crossing-edge sets differ (|D64| at a vertex below the float32 error of D) the two polygons differ by at most the two
    # cells beside each such edge
    slack = 2 * len(differ) * hx * hy
    for q, name in enumerate(("area_tangential", "area_radial", "caustic_area_tangential", "caustic_area_radial")):
        want = abs(ref["area"][q])
        extra = slack * (1 if q < 2 else float(scale_h.max()) ** 2)
        if not expect_closed and np.isnan(res[name][b]):
            assert not res["closed"][b]
            continue
        assert abs(res[name][b] - want) <= 1e-4 * max(want, abs(ref["area"][0])) + extra, (case, b, name, res[name][b], want)
    return len(common), len(differ), dist.max(), d_yard.max(), b_yard.max()


# ---- 1. SIS | Shear against the closed form ----------------------------------------------------------------------------------------------
def test_sis_shear_closed_form(gl):
    c = C.sis_shear_case()
    sim = _sim(gl, "sis|shear", c["phys_mp"], 3)
    packed = sim._pack_partial({"lens_mass": _lens_t(c["lens_params"])})
    kw = dict(window=C.CF_WINDOW, num_cells=C.CF_CELLS, source_redshifts=C.CF_Z)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        raw = sim.critical_curves(packed, strict=True, **kw)
        theta = sim.einstein_radius(packed, **kw).double().cpu().numpy()
    res = _np(raw)
    assert res["critical"].shape == (3, 8 * C.CF_CELLS, 2, 2) and theta.shape == (3,)
    endpoint_gate, beta_gate = _gates("sis|shear", C.CF_WINDOW)
    cell = (C.CF_WINDOW[1] - C.CF_WINDOW[0]) / C.CF_CELLS
    fails = []
    for b in range(3):
        cf = C.sis_shear_closed_form(b)
        n = int(res["n"][b])
        assert res["closed"][b] and n > 0
        assert np.all(res["kind"][b, :n] == 0) and np.all(res["kind"][b, n:] == -1)
        p = res["critical"][b, :n].astype(np.float64).reshape(-1, 2)
        d = p - cf["centre"]
        phi = np.arctan2(d[:, 1], d[:, 0])
        # (the curve is within 1e-2 of a circle: the radial offset is the distance to the curve to 1e-4 of itself)
        r_err = np.abs(np.hypot(d[:, 0], d[:, 1]) - cf["radius"](phi))
        fields = C.recursion_fields(c["phys"], c["mp"], c["lens_params"], b, c["target"])
        d_yard, b_yard = _maps_error(sim, packed, b, c["target"], fields, p.astype(np.float32), CC.grad_D)
        cau = res["caustic"][b, :n].astype(np.float64).reshape(-1, 2)
        # beta = M theta - N theta_E rhat: an endpoint offset of d along the curve's normal moves it by at most |M| d (rhat turns by d / r)
        cau_err = np.hypot(*(cau - cf["caustic"](phi).T).T)
        cau_gate = beta_gate + (np.linalg.norm(cf["M"], 2) + np.linalg.norm(cf["N"], 2) * cf["theta_E"] / cf["radius"](phi).min()) * endpoint_gate
        R = math.sqrt(cf["area"] / math.pi)
        rel = (R - theta[b]) / R
        # from below: the polygon is inscribed in a convex curve; a chord of length L <= sqrt(2) h cuts off L^3 kappa / 12, and the
        # curvature integrates to 2 pi, so the area lacks at most pi h^2 / 3 and the radius h^2 / (6 R^2) of itself; the endpoints' own
        # error moves the area by at most perimeter x gate
        slack = endpoint_gate * cf["perimeter"] / (2 * math.pi * R * R)
        print(f"SIS | Shear sample {b}: {n} segments, radius error max {r_err.max():.3e} (gate {endpoint_gate:.3e}), caustic error max "
              f"{cau_err.max():.3e} (gate {cau_gate:.3e}), einstein radius {theta[b]:.6f} (closed form {R:.6f}, rel {rel:.3e}); "
              f"yardstick D {d_yard.max():.3e}, beta {b_yard.max():.3e}")
        if not r_err.max() <= endpoint_gate:
            fails.append((b, "radius", r_err.max()))
        if not cau_err.max() <= cau_gate:
            fails.append((b, "caustic", cau_err.max()))
        if not -slack <= rel <= cell ** 2 / (6 * R * R) + slack:
            fails.append((b, "einstein radius", rel))
        chains = sim.chain_curves(raw, b)
        assert len(chains) == 1 and chains[0][0] == 0 and chains[0][1] and len(chains[0][2]) == n
    assert not fails, fails


# ---- 2. general lenses against contour64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.GENERAL))
def test_general_lenses_against_float64(gl, name):
    c = MC.map_case(name)
    z, T = C.general_targets(name)
    _, window, n_cells = C.GENERAL[name]
    sim = _sim(gl, name, c["phys_mp"], 3)
    packed = sim._pack_partial({"lens_mass": _lens_t(c["lens_params"])})
    out = sim.critical_curves(packed, window=window, num_cells=n_cells, source_redshifts=list(z), strict=True)
    assert isinstance(out, list) and len(out) == len(z)
    theta = sim.einstein_radius(packed, window=window, num_cells=n_cells, source_redshifts=list(z)).cpu().numpy()
    assert theta.shape == (3, len(z))
    edges = differ = 0
    worst = d_yard = b_yard = 0.0
    fails = []
    for s in range(len(z)):
        res = _np(out[s])
        for b in range(3):
            fields, ref = C.general_reference(name, b, s)
            e, d, dist, dy, by = _compare(sim, packed, res, b, T[s], fields, ref, window, n_cells, name, fails)
            edges, differ, worst, d_yard, b_yard = edges + e, differ + d, max(worst, dist), max(d_yard, dy), max(b_yard, by)
            want = math.sqrt(abs(ref["area"][0]) / math.pi)  # (d differing edges move the area by at most 2 d cells)
            cell2 = (window[1] - window[0]) * (window[3] - window[2]) / n_cells ** 2
            assert abs(theta[b, s] - want) <= 1e-4 * want + 2 * d * cell2 / (2 * math.pi * want), (name, b, s, theta[b, s], want)
    print(f"{name}: {edges} crossing edges, {differ} differ; endpoint distance max {worst:.3e} (gate {_gates(name, window)[0]:.3e}); "
          f"yardsticks: D {d_yard:.3e}, beta {b_yard:.3e}")
    assert not fails, fails
    assert differ <= 0.01 * edges, (differ, edges)


# ---- 3. the dPIS convergence excess ----------------------------------------------------------------------------------------------------------
def test_dpis_excess_enters_the_curve(gl):
    name, z, window, n_cells = C.DPIS
    c = MC.map_case(name)
    T = c["mp"].target_scales(z[0])
    sim = _sim(gl, name, c["phys_mp"], 3)
    packed = sim._pack_partial({"lens_mass": _lens_t(c["lens_params"])})
    res = _np(sim.critical_curves(packed, window=window, num_cells=n_cells, source_redshifts=z[0], strict=True))
    endpoint_gate, _ = _gates(name, window)
    fails = []
    for b in range(3):
        n = int(res["n"][b])
        assert n > 0 and res["closed"][b]
        pts = np.unique(res["critical"][b, :n].reshape(-1, 2), axis=0)
        ref = C.maps_fields(MC.maps_hessian, c["phys"], c["mp"], c["lens_params"], b, T)      # with the excess: the reference
        plain = C.maps_fields(MC.maps, c["phys"], c["mp"], c["lens_params"], b, T)            # without it
        dist = np.abs(ref(pts[:, 0], pts[:, 1])[0]) / C.grad_D32(ref, pts[:, 0], pts[:, 1])
        apart = np.abs(plain(pts[:, 0], pts[:, 1])[0]) / C.grad_D32(plain, pts[:, 0], pts[:, 1])
        d_yard, b_yard = _maps_error(sim, packed, b, T, ref, pts, C.grad_D32)
        print(f"{name} sample {b}: {len(pts)} endpoints, distance to D = 0 of maps_hessian max {dist.max():.3e} (gate {endpoint_gate:.3e}), "
              f"to D = 0 without the excess max {apart.max():.3e}; yardstick D {d_yard.max():.3e}, beta {b_yard.max():.3e}")
        if not dist.max() <= endpoint_gate:
            fails.append((b, dist.max()))
        assert apart.max() > 100 * endpoint_gate  # the excess moves the curve: a kernel without it would miss the gate
    assert not fails, fails


# ---- 4. a source between the planes: only the front plane acts ------------------------------------------------------------------------------
def test_source_between_the_planes_equals_the_scaled_front_plane(gl):
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    name = "epl_shear|sie"
    c = MC.map_case(name)
    _, window, n_cells = C.GENERAL[name]
    T = c["mp"].target_scales(0.8)
    assert T[0] > 0 and T[1] == 0
    sim = _sim(gl, name, c["phys_mp"], 3)
    front = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:2], [], []), SimulatorConfig(delta_pix=0.1, num_pix=8), bs=3)
    lt = _lens_t(c["lens_params"])
    a = _np(sim.critical_curves(lt, window=window, num_cells=n_cells, source_redshifts=0.8, strict=True))
    f = _np(front.critical_curves(lt[:2], window=window, num_cells=n_cells, deflection_scale=float(np.float32(T[0])), strict=True))
    endpoint_gate, _ = _gates(name, window)
    assert np.array_equal(a["n"], f["n"]) and np.array_equal(a["kind"], f["kind"]) and a["closed"].all() and f["closed"].all()
    for b in range(3):
        (ga, ea), (gf, ef) = _got_edges(a, b, window, n_cells), _got_edges(f, b, window, n_cells)
        assert ea == ef and len(ea) >= 20, b  # the same segments between the same grid edges, in the same order
        # the single-plane path in float64: the oracle's fields of the two front lenses on the plane of scale T_0
        rows = [{k: torch.as_tensor(np.asarray(v, np.float32)).double() for k, v in d.items()} for d in c["lens_params"][:2]]
        fields = CC.scaled_fields(CC.oracle_fields(front.phys_model, rows, b), float(np.float32(T[0])))
        pts = np.array([ga[e][0] for e in sorted(ga)])
        dist = np.abs(fields(pts[:, 0], pts[:, 1])[0]) / CC.grad_D(fields, pts[:, 0], pts[:, 1])
        both = np.hypot(*(pts - np.array([gf[e][0] for e in sorted(ga)])).T)
        print(f"between the planes, sample {b}: {len(pts)} edges, distance to the single-plane float64 curve max {dist.max():.3e} "
              f"(gate {endpoint_gate:.3e}), between the two kernels max {both.max():.3e}")
        assert dist.max() <= endpoint_gate, (b, dist.max())


# ---- 5. one call for three sources = three calls for one --------------------------------------------------------------------------------------
def test_three_sources_in_one_call_bit_for_bit(gl):
    name = "epl_shear|sie"
    c = MC.map_case(name)
    _, window, n_cells = C.GENERAL[name]
    sim = _sim(gl, name, c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"])
    zs = [2.0, 0.8, 1.5]  # (0.8: between the planes)
    kw = dict(window=window, num_cells=n_cells)
    many = sim.critical_curves(lt, source_redshifts=zs, **kw)
    radii = sim.einstein_radius(lt, source_redshifts=zs, **kw)
    assert isinstance(many, list) and len(many) == 3 and tuple(radii.shape) == (3, 3)
    for s, z in enumerate(zs):
        one = sim.critical_curves(lt, source_redshifts=z, **kw)
        assert isinstance(one, dict) and tuple(one["critical"].shape) == (3, 8 * n_cells, 2, 2) and tuple(one["n"].shape) == (3,)
        for k in one:
            assert torch.equal(_bits(many[s][k]), _bits(one[k])), (s, k)
        assert torch.equal(_bits(radii[:, s]), _bits(sim.einstein_radius(lt, source_redshifts=z, **kw)))
        assert len(sim.chain_curves(many[s], 1)) == len(sim.chain_curves(one, 1)) >= 1
    # views of one [B, S, ...] result
    assert many[0]["critical"].data_ptr() != many[1]["critical"].data_ptr() and many[0]["critical"]._base is many[1]["critical"]._base
    assert not torch.equal(many[0]["n"], many[1]["n"])  # different redshifts: different curves


# ---- 6. K = 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_four_planes(gl):
    phys, phys_mp, mp, lp = IC.four_plane_case()
    sim = _sim(gl, "four_planes", phys_mp, 1)
    packed = sim._pack_partial({"lens_mass": _lens_t(lp)})
    res = _np(sim.critical_curves(packed, window=C.FOUR_WINDOW, num_cells=C.FOUR_CELLS, source_redshifts=2.0, strict=True))
    fields, ref = C.four_plane_reference()
    fails = []
    e, d, *_ = _compare(sim, packed, res, 0, mp.target_scales(2.0), fields, ref, C.FOUR_WINDOW, C.FOUR_CELLS, "four_planes", fails)
    assert not fails, fails
    assert e >= 40 and d <= 0.01 * e


# ---- 7. bookkeeping per (sample, source) ---------------------------------------------------------------------------------------------------------
def test_bookkeeping_per_sample_and_source(gl):
    name = "epl_shear|sie"
    c = MC.map_case(name)
    (z, window, n_cells) = C.GENERAL[name]
    sim = _sim(gl, name, c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"])
    kw = dict(window=window, num_cells=n_cells, source_redshifts=list(z))
    a, b2 = sim.critical_curves(lt, **kw), sim.critical_curves(lt, **kw)
    for s in range(2):
        for k in a[s]:
            assert torch.equal(_bits(a[s][k]), _bits(b2[s][k])), (s, k)
        n = a[s]["n"].cpu().numpy()
        for q in range(3):  # padding
            assert torch.isnan(a[s]["critical"][q, n[q]:]).all() and torch.isnan(a[s]["caustic"][q, n[q]:]).all()
            assert torch.isfinite(a[s]["critical"][q, :n[q]]).all() and (a[s]["kind"][q, n[q]:] == -1).all()
    # too few slots for the far source alone (98 to 142 segments against 28 to 44): reported for its rows, never silent
    n_far, n_near = a[0]["n"].cpu().numpy(), a[1]["n"].cpu().numpy()
    M = 60
    assert n_far.min() > M > n_near.max()
    with pytest.warns(RuntimeWarning, match=r"not returned over 3 \(sample, source\) pair"):
        small = sim.critical_curves(lt, max_segments=M, **kw)
    assert tuple(small[0]["critical"].shape) == (3, M, 2, 2)
    assert not bool(small[0]["closed"].any()) and bool(torch.isnan(small[0]["area_tangential"]).all())
    assert bool(small[1]["closed"].all()) and bool(torch.isfinite(small[1]["area_tangential"]).all())
    for k in small[1]:  # the near source's rows are those of the roomy call
        assert torch.equal(_bits(small[1][k]), _bits(a[1][k][:, :M] if a[1][k].dim() > 1 else a[1][k])), k
    T = np.stack(C.general_targets(name)[1])
    native = sim._model.multiplane_critical_curves(sim._pack_partial({"lens_mass": lt}), T, window, n_cells, M)
    assert tuple(native[0].shape) == (3, 2, M, 2, 2) and tuple(native[7].shape) == (3, 2, 4)
    # (beyond the slots, a kept slot whose endpoint fell off the list of 2 M crossing edges counts as dropped: with_capacity)
    want_dropped = [CC.with_capacity(C.general_reference(name, q, 0)[1], M)[2] for q in range(3)]
    assert native[4].cpu().numpy()[:, 0].tolist() == want_dropped and min(want_dropped) > 0 and not native[4].cpu().numpy()[:, 1].any()
    with pytest.raises(RuntimeError, match="not returned"):
        sim.critical_curves(lt, max_segments=M, strict=True, **kw)
    with warnings.catch_warnings(record=True) as seen:  # (two warnings: the dropped segments, then the radii)
        warnings.simplefilter("always")
        theta = sim.einstein_radius(lt, max_segments=M, **kw)
    assert any("open or absent in 3 of 6 (sample, source) pair(s)" in str(w.message) for w in seen), [str(w.message) for w in seen]
    assert bool(torch.isnan(theta[:, 0]).all()) and bool(torch.isfinite(theta[:, 1]).all())
    # a window that cuts the curves: `open` per (sample, source), as the float64 reference has it
    cut_window = (0.0, 3.0, window[2], window[3])
    cut = sim.critical_curves(lt, **{**kw, "window": cut_window, "num_cells": 24})
    for s in range(2):
        for q in range(3):
            ref = CC.contour64(C.recursion_fields(c["phys"], c["mp"], c["lens_params"], q, T[s]), cut_window, 24)
            assert ref["open"] and not bool(cut[s]["closed"][q]) and bool(torch.isnan(cut[s]["area_tangential"][q]))
        assert any(not ch[1] for ch in sim.chain_curves(cut[s], 0))


# ---- 8. singular vertices -------------------------------------------------------------------------------------------------------------------------
def _dmap(sim, B, S, n_cells):
    """The map of D of the last call, [B, S, n+1, n+1], out of its workspace (the map is the first array of the layout)."""
    V = (n_cells + 1) ** 2
    ws = sim._model._scratch_bufs["multiplane_critical_curves"]
    return ws[:4 * B * S * V].view(torch.float32).reshape(B, S, n_cells + 1, n_cells + 1).cpu().numpy()


def test_vertex_on_an_sis_centre_of_plane_one(gl):
    """The SIS of plane 1 sits bit for bit on vertex (row 22, column 25) of the grid: D there is NaN for every source, its four cells
    are skipped, and -- the centre lies inside D < 0 -- nothing is flagged: the curve is that of contour64, whose float64 field is
    not finite there either."""
    c = C.sis_shear_case()
    window, n = C.CF_WINDOW, C.CF_CELLS  # cells of 0.125: vertex (25, 22) = (0.125, -0.25) in float32 and in float64
    lp = [{"theta_E": MC._f32(1.2, 0.9, 1.5), "center_x": MC._f32(0.125, 0.125, 0.125), "center_y": MC._f32(-0.25, -0.25, -0.25)},
          c["lens_params"][1]]
    sim = _sim(gl, "sis|shear", c["phys_mp"], 3)
    packed = sim._pack_partial({"lens_mass": _lens_t(lp)})
    zs = [2.0, 0.7]  # (0.7: between the planes)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sim.critical_curves(packed, window=window, num_cells=n, source_redshifts=zs, strict=True)
    D = _dmap(sim, 3, 2, n)
    assert np.isnan(D[:, :, 22, 25]).all() and np.isfinite(np.delete(D.reshape(3, 2, -1), 22 * (n + 1) + 25, axis=2)).all()
    for s, z in enumerate(zs):
        res = _np(out[s])
        for b in range(3):
            ref = CC.contour64(C.recursion_fields(c["phys"], c["mp"], lp, b, c["mp"].target_scales(z)), window, n)
            assert np.isnan(ref["D"][22, 25]) and ref["n_flagged"] == 0 and not ref["open"]
            got, per_seg = _got_edges(res, b, window, n)
            assert set(got) == set(ref["edges"]) and np.array_equal(np.array(per_seg), ref["seg_edges"]), (s, b)
            assert res["closed"][b] and int(res["n"][b]) == len(ref["seg"])


def test_ray_on_a_lens_centre_of_plane_two(gl):
    """A Shear (gamma_1 = 1/2) on plane 1 and an SIS on plane 2.  At the vertex (0.25, -0.5) the deflection of plane 1 is (1/8, 1/4)
    exactly, so theta_2 = theta - C_12 a_1 is ONE float32 rounding however the kernel contracts it, and the SIS is centred on that
    float32 value: the ray lands bit for bit on its centre.  The vertex is NaN for the source behind both planes and finite for
    the source between them (a flagged plane at or behind a source does not flag it).  The float64 field is finite there (the ray
    passes the float32 centre at 1e-8) and negative like its neighbours, so the reference crosses the same edges."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    mp = MC._mp([0.4, 1.0])
    C12 = np.float32(mp.lens_scales[0, 1])
    cx, cy = np.float32(np.float64(0.25) - np.float64(C12) * 0.125), np.float32(np.float64(-0.5) - np.float64(C12) * 0.25)
    lp = [{"gamma1": MC._f32(0.5), "gamma2": MC._f32(0.0)}, {"theta_E": MC._f32(1.0), "center_x": MC._f32(cx), "center_y": MC._f32(cy)}]
    lenses = [Shear(), SIS()]
    phys, phys_mp = PhysicalModel(lenses, [], []), PhysicalModel(lenses, [], [], multiplane=mp)
    sim = _sim(gl, "shear|sis", phys_mp, 1)
    window, n = (-3.0, 3.0, -3.0, 3.0), 48
    zs = [2.0, 0.7]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (a shear of 1/2 sends the curve of the far source out of the window)
        out = sim.critical_curves(_lens_t(lp), window=window, num_cells=n, source_redshifts=zs)
    D = _dmap(sim, 1, 2, n)
    row, col = 20, 26  # (-3 + 20 / 8, -3 + 26 / 8) = (-0.5, 0.25)
    assert np.isnan(D[0, 0, row, col]) and np.isfinite(D[0, 1, row, col])
    assert np.isfinite(np.delete(D[0, 0].ravel(), row * (n + 1) + col)).all() and np.isfinite(D[0, 1]).all()
    native = sim._model.multiplane_critical_curves(sim._pack_partial({"lens_mass": _lens_t(lp)}), np.stack([mp.target_scales(v) for v in zs]),
                                                   window, n, 8 * n)
    for s, z in enumerate(zs):
        res = _np(out[s])
        ref = CC.contour64(C.recursion_fields(phys, mp, lp, 0, mp.target_scales(z)), window, n)
        assert np.isfinite(ref["D"][row, col])
        got, _ = _got_edges(res, 0, window, n)
        assert set(got) == set(ref["edges"]), s
        # the cells of the NaN vertex are skipped; they count as flagged only where their finite vertices differ in sign
        cells = [(r, c) for r in (row - 1, row) for c in (col - 1, col)]
        corners = lambda r, c: [v for v in ((r, c), (r, c + 1), (r + 1, c + 1), (r + 1, c)) if v != (row, col)]
        want_flagged = sum(len({bool(ref["D"][v] < 0) for v in corners(r, c)}) == 2 for r, c in cells) if s == 0 else 0
        assert int(native[5][0, s]) == want_flagged + ref["n_flagged"], (s, int(native[5][0, s]), want_flagged)
        assert bool(native[6][0, s]) == ref["open"], s


# ---- rules that need a model ------------------------------------------------------------------------------------------------------------------------
def test_python_rules(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    name = "epl_shear|sie"
    c = MC.map_case(name)
    _, window, n_cells = C.GENERAL[name]
    sim = _sim(gl, name, c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"])
    kw = dict(window=window, num_cells=n_cells)
    for call in (sim.critical_curves, sim.einstein_radius):
        with pytest.raises(_native.UnsupportedLensError, match=r"critical_curves\(source_redshifts"):  # planes, and no redshift names one
            call(lt, **kw)
        with pytest.raises(_native.UnsupportedLensError):
            call(lt, deflection_scale=0.9, **kw)
        with pytest.raises(ValueError, match="deflection_scale"):
            call(lt, source_redshifts=2.0, deflection_scale=0.9, **kw)
        for bad_z in (float("nan"), float("inf"), 0.5, 0.3, [2.0, 0.5], [2.0, float("nan")], [], [[2.0, 2.0]]):
            with pytest.raises(ValueError, match="source_redshifts"):
                call(lt, source_redshifts=bad_z, **kw)
        with pytest.raises(NotImplementedError):
            call(sim._pack_partial({"lens_mass": lt}).clone().requires_grad_(True), source_redshifts=2.0, **kw)
        for bad in (dict(num_cells=0), dict(max_segments=0), dict(window=(1.0, 1.0, -1.0, 1.0))):
            with pytest.raises(_native.NativeLibraryError):
                call(lt, source_redshifts=2.0, **{**kw, **bad})
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    plain = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:2], [], []), cfg, bs=3)
    with pytest.raises(ValueError, match="deflection_scale"):  # no MultiPlane: the keyword of that model is deflection_scale
        plain.critical_curves(lt[:2], source_redshifts=2.0, **kw)
    # a one-plane MultiPlane: every redshift becomes the deflection scale of the existing path, bit for bit
    from gigalens_amd.profiles.light.sersic import Sersic
    mp1 = MC._mp([0.5, 0.5], [2.0])
    single = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:2], [], [Sersic()], multiplane=mp1), cfg, bs=3)
    got = single.critical_curves(lt[:2], source_redshifts=[0.8, 2.0], **kw)
    one = single.critical_curves(lt[:2], source_redshifts=0.8, **kw)
    assert isinstance(got, list) and len(got) == 2 and isinstance(one, dict)
    for s, z in enumerate((0.8, 2.0)):
        want = single.critical_curves(lt[:2], deflection_scale=float(mp1.target_scales(z)[0]), **kw)
        for k in want:
            assert torch.equal(_bits(got[s][k]), _bits(want[k])), (s, k)
    assert tuple(single.einstein_radius(lt[:2], source_redshifts=[0.8, 2.0], **kw).shape) == (3, 2)


def test_native_rules_and_workspace(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    L = _native.lib()
    GL_EINVAL, GL_ENOMEM = -1, -4
    c2, c3 = MC.map_case("epl_shear|sie"), MC.map_case("nfw|dpie|sis")
    sim2, sim3 = _sim(gl, "epl_shear|sie", c2["phys_mp"], 3), _sim(gl, "nfw|dpie|sis", c3["phys_mp"], 3)
    plain = gl.LensSimulator(PhysicalModel(c2["phys"].lenses[:2], [], []), SimulatorConfig(delta_pix=0.1, num_pix=8), bs=3)
    h2, h3, h1 = sim2._model._h, sim3._model._h, plain._model._h
    wsb, wsb1 = L.gl_multiplane_critical_curves_workspace_bytes, L.gl_critical_curves_workspace_bytes
    for bad in ((h2, 0, 2, 32, 64), (h2, 3, 0, 32, 64), (h2, 3, 2, 0, 64), (h2, 3, 2, 8193, 64), (h2, 3, 2, 32, 0),
                (h2, 3, 2, 32, (1 << 20) + 1), (h2, 1 << 16, 1 << 16, 32, 64), (h1, 3, 2, 32, 64), (None, 3, 2, 32, 64)):
        assert wsb(*bad) == 0, bad
    # the single-plane workspace of B S samples + the coupling rows
    up = lambda v: (v + 255) // 256 * 256
    for B, S, n, M in ((3, 2, 32, 64), (1, 3, 5, 7), (4, 1, 64, 512)):
        for h, K in ((h2, 2), (h3, 3)):
            assert wsb(h, B, S, n, M) == wsb1(h1, B * S, n, M) + up(S * K * 4), (B, S, n, M, K)
    packed = sim2._pack_partial({"lens_mass": _lens_t(c2["lens_params"])})
    dev = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=sim2.device)
    M = 64
    seg, cau, kind, area = dev(3, 2, M, 2, 2), dev(3, 2, M, 2, 2), dev(3, 2, M, dtype=torch.int32), dev(3, 2, 4)
    cnt = [dev(3, 2, dtype=torch.int32) for _ in range(4)]
    ws = dev(wsb(h2, 3, 2, 32, M), dtype=torch.uint8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    good_T = np.ascontiguousarray(np.stack([c2["mp"].target_scales(0.8), c2["mp"].target_scales(2.0)]), dtype=np.float32)

    def call(h=h2, T=good_T, K=2, window=(-2.4, 2.4, -2.4, 2.4), n=32, max_segments=M, nbytes=None, B=3, S=2):
        T = np.ascontiguousarray(T, dtype=np.float32)
        return L.gl_multiplane_critical_curves(h, ptr(packed), B, T.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), S, K, *window, n,
                                               max_segments, ptr(seg), ptr(cau), ptr(kind), *(ptr(t) for t in cnt), ptr(area), ptr(ws),
                                               ws.numel() if nbytes is None else nbytes, None)

    assert call() == 0
    assert call(h=h1) == GL_EINVAL and b"gl_model_set_lens_planes has not been called" in L.gl_last_error()
    assert call(K=3, T=np.ones((2, 3))) == GL_EINVAL and b"lens planes" in L.gl_last_error()
    for bad_T in ([[np.nan, 0.5], [1, 0.5]], [[1, 0.5], [np.inf, 0.5]], [[-0.1, 0.5], [1, 0.5]], [[1, 0.5], [0, 0.5]], [[0, 0], [1, 0.5]]):
        assert call(T=bad_T) == GL_EINVAL, bad_T
    for kw in (dict(B=0), dict(S=0), dict(n=0), dict(n=8193), dict(max_segments=0), dict(max_segments=(1 << 20) + 1),
               dict(window=(1.0, 1.0, -1.0, 1.0)), dict(window=(-1.0, 1.0, 2.0, 1.0)), dict(window=(-np.inf, 1.0, -1.0, 1.0))):
        assert call(**kw) == GL_EINVAL, kw
    # more than 2^31 - 1 workgroups in the refine launch: B S ceil(2 max_segments / 64) (checked before the workspace)
    assert call(B=1 << 10, S=1 << 7, max_segments=1 << 20, T=np.tile(good_T[:1], (1 << 7, 1))) == GL_EINVAL
    assert b"too many" in L.gl_last_error()
    assert call(nbytes=ws.numel() - 1) == GL_ENOMEM
    # the single-plane entries keep refusing a model with planes
    ws1 = dev(max(wsb1(h2, 3, 32, M), 256), dtype=torch.uint8)
    one = [t[:, 0].contiguous() for t in (seg, cau, kind, *cnt, area)]
    rc = L.gl_critical_curves(h2, ptr(packed), 3, -2.4, 2.4, -2.4, 2.4, 32, M, *(ptr(t) for t in one), ptr(ws1), ws1.numel(), None)
    assert rc == _native.GL_EUNSUPPORTED and b"lens planes" in L.gl_last_error()
    torch.cuda.synchronize()
