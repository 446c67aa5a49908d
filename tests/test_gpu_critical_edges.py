"""Critical curves at their grid and list edges (gl_critical.hip.h: map -> scan -> refine -> cells): every split of the edge and
cell ranges over the four waves from one cell to 127 x 127, a rectangular off-centre window, the ambiguous marching-squares rows
(5, 10 and their joined forms 16, 17), flagged cells around a singular vertex, and the segment / edge capacity accounted for
exactly -- each against the float64 restatement of tests/critical_cases.py on closed-form or oracle fields, with the orientation of
every segment and the number of closed curves checked independently of the marching-squares table.

Endpoint gate for these windows, in the form of tests/test_gpu_critical_curves.py: 4 x yardstick + 4 eps32 max |window coordinate|,
the yardstick being the float32 error of D from gl_lens_maps_kernel against the float64 fields at the returned endpoints, divided
by |grad D64|, measured in each test over all its samples and printed before anything is asserted."""
import functools
import warnings

import numpy as np
import pytest

from tests import critical_cases as CC
from tests.critical_cases import packed_rows as _rows, simulator as _sim
from tests.test_gpu_critical_curves import EPS32, _compare_with_restatement, _lens_maps_error

pytestmark = pytest.mark.gpu

# RECT: off-centre, cells wider than tall (hx = 5/24, hy = 1/6); TALL: cells taller than wide (hx = 1/6, hy = 5/24), the one on which
# a bisection of a vertical edge over hx instead of hy stops short of the crossing
SQUARE, RECT, TALL = (-2.0, 2.0, -2.0, 2.0), (-1.5, 3.5, -2.0, 2.0), (-2.0, 2.0, -2.5, 2.5)
D_MARGIN = 1e-4  # min |D64| over the vertices: float32 and float64 signs agree for the right reason
# theta_E, center_x, center_y / theta_E, gamma, e1, e2, center_x, center_y, gamma1, gamma2: each row drawn (SIS: theta_E in
# (1.1, 1.45), centre within 0.15; EPL + Shear: the ranges of tests/test_gpu_critical_curves.py with theta_E in (1.0, 1.3)) until
# D_MARGIN holds on every grid below and no curve reaches a window edge
SIS_ROWS = [[1.277, 0.11, 0.047], [1.241, -0.029, -0.032], [1.412, 0.126, 0.063], [1.132, 0.103, 0.09]]
EPL_ROWS = [[1.27, 2.226, 0.097, 0.09, -0.041, 0.006, -0.003, 0.072], [1.136, 2.198, -0.085, 0.255, 0.07, 0.098, -0.044, 0.059],
            [1.089, 1.885, 0.102, 0.162, -0.079, 0.086, 0.041, 0.049], [1.08, 2.274, -0.151, 0.264, 0.098, 0.015, -0.061, -0.026]]
GRIDS = [(n, SQUARE) for n in (1, 2, 3, 7, 16, 23, 32, 127)] + [(24, RECT), (24, TALL)]


@functools.lru_cache(maxsize=None)
def _model(lens):
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    if lens == "SIS":
        sim = _sim([SIS()], 16, 0.25, 4)
        return sim, _rows(sim, np.array(SIS_ROWS))
    if lens == "SIS2":
        return _sim([SIS(), SIS()], 16, 0.25, 1), None
    sim = _sim([EPL(), Shear()], 16, 0.25, 4)
    return sim, _rows(sim, np.array(EPL_ROWS))


def _fields(lens, sim, packed, b, scale=1.0):
    if lens == "SIS":
        te, cx, cy = (float(v) for v in packed[b, :3].double().cpu())
        return CC.multi_sis_fields([(te, cx, cy)], scale)
    f = CC.oracle_fields(sim.phys_model, CC.lens_rows(sim, packed), b)
    return f if scale == 1.0 else CC.scaled_fields(f, scale)


def _call(sim, packed, window, n, max_segments=None, scale=1.0):
    """(the public result as numpy, the raw counters n_dropped, n_flagged, open) of one call; warnings are the caller's business."""
    kw = {} if scale == 1.0 else {"deflection_scale": scale}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        raw = sim.critical_curves(packed, window=window, num_cells=n, max_segments=max_segments, **kw)
    M = raw["critical"].shape[1]
    counters = sim._model.critical_curves(packed, window, n, M, scale=None if scale == 1.0 else scale)[4:7]
    return raw, {k: v.cpu().numpy() for k, v in raw.items()}, [c.cpu().numpy() for c in counters]


def _gates(sim, packed, res, fields, window, scale=1.0):
    """Endpoint and beta gates of this call from the yardsticks measured at its own endpoints over all samples (printed)."""
    d_yard = b_yard = 0.0
    for b, f in enumerate(fields):
        pts = res["critical"][b, :int(res["n"][b])].reshape(-1, 2)
        pts = pts[np.isfinite(pts).all(1)]
        d, bb = _lens_maps_error(sim, packed, b, f, pts, scale)
        if len(d):
            d_yard, b_yard = max(d_yard, float(d.max())), max(b_yard, float(bb.max()))
    bracket = 4 * EPS32 * max(abs(v) for v in window)
    print(f"yardsticks over {len(fields)} samples: D {d_yard:.3e}, beta {b_yard:.3e}; endpoint gate {4 * d_yard + bracket:.3e}")
    return 4 * d_yard + bracket, 4 * b_yard + bracket


def _left_is_negative(res, b, ref, window, n):
    """Orientation independently of the table, on the kernel's own segments against the float64 vertex plane."""
    k = int(res["n"][b])
    live = res["kind"][b, :k] >= 0
    assert CC.orientation_violations(res["critical"][b, :k][live], ref["D"], window, n) == []


def _check_grid(lens, n, window, scale=1.0):
    sim, packed = _model(lens)
    B = packed.shape[0]
    fields = [_fields(lens, sim, packed, b, scale) for b in range(B)]
    raw, res, (dropped, flagged, opened) = _call(sim, packed, window, n, scale=scale)
    gates = _gates(sim, packed, res, fields, window, scale)
    fails, codes = [], set()
    for b in range(B):
        e, differ, dist, _, _, ref = _compare_with_restatement(sim, packed, res, b, deferred=fails, window=window, n_cells=n,
                                                               fields=fields[b], gates=gates, scale=scale)
        assert np.nanmin(np.abs(ref["D"])) >= D_MARGIN, (b, np.nanmin(np.abs(ref["D"])))
        assert differ == 0, (b, differ)
        assert int(res["n"][b]) == len(ref["seg"]) and dropped[b] == 0 and flagged[b] == ref["n_flagged"] == 0
        assert bool(opened[b]) == ref["open"] and not ref["open"] and bool(res["closed"][b])
        _left_is_negative(res, b, ref, window, n)
        loops = sum(1 for c in sim.chain_curves(raw, b) if c[1])
        assert (loops, 0) == CC.count_loops(ref["seg"]) and all(c[1] for c in sim.chain_curves(raw, b))
        codes |= set(CC.cell_codes(ref["D"]).ravel().tolist())
        print(f"  sample {b}: {len(ref['seg'])} segments on {len(ref['edges'])} of {2 * n * (n + 1)} edges, {loops} closed curve(s)")
    print(f"{lens} n = {n} window {window}: codes seen {sorted(codes - {0, 15})}")
    assert not fails, fails


# ---- a. grid sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,window", GRIDS)
@pytest.mark.parametrize("lens", ["SIS", "EPL+Shear"])
def test_grid_sizes_and_windows(lens, n, window):
    _check_grid(lens, n, window)


# ---- e. one of them on the plane of deflection scale 0.6 -----------------------------------------------------------------------
def test_scaled_plane_on_an_odd_grid():
    _check_grid("EPL+Shear", 23, SQUARE, scale=0.6)


# ---- b. ambiguous cells -------------------------------------------------------------------------------------------------------------
def test_ambiguous_cells_topology_and_orientation():
    sim, _ = _model("SIS2")
    window, n = CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N
    names = sorted(CC.AMBIGUOUS)
    cases = [CC.ambiguous_case(name) for name in names]
    packed = _rows(sim, np.array([[v for lens in c[0] for v in lens] for c in cases]))
    assert [n for p in sim.phys_model.lenses for n in p._native_params()] == ["theta_E", "center_x", "center_y"] * 2
    fields = [CC.multi_sis_fields(c[0]) for c in cases]
    raw, res, (dropped, flagged, opened) = _call(sim, packed, window, n)
    gates = _gates(sim, packed, res, fields, window)
    fails, codes = [], set()
    for b, (name, (lenses, code, joined, curves)) in enumerate(zip(names, cases)):
        ref = _compare_with_restatement(sim, packed, res, b, deferred=fails, window=window, n_cells=n, fields=fields[b], gates=gates)
        assert ref[1] == 0
        ref = ref[-1]
        amb = CC.ambiguous_cells(ref["D"])
        assert ref["n_ambiguous"] == 1 and amb[0][2:4] == (code, joined) and amb[0][4] >= CC.AMBIGUOUS_MARGIN, (name, amb)
        assert np.abs(ref["D"]).min() >= CC.AMBIGUOUS_MARGIN
        assert dropped[b] == 0 and flagged[b] == 0 and not opened[b] and res["closed"][b]
        # topology independently of the table: closed loops only, as many as the regions of D on a fine grid imply
        chains = sim.chain_curves(raw, b)
        assert all(c[1] for c in chains) and len(chains) == curves == CC.physical_loops(fields[b], window)[0], (name, len(chains))
        _left_is_negative(res, b, ref, window, n)
        codes |= set(CC.cell_codes(ref["D"]).ravel().tolist())
        print(f"  {name}: cell {amb[0][:2]}, margin {amb[0][4]:.4f}, {len(ref['seg'])} segments, {len(chains)} closed curve(s)")
    assert codes >= set(range(1, 15)), sorted(codes)
    assert not fails, fails


# ---- c. flagged cells ---------------------------------------------------------------------------------------------------------------
def test_flagged_cells_around_a_singular_vertex():
    from gigalens_amd.profiles.mass.sis import SIS
    window, n, h = SQUARE, 16, 0.25
    cx, cy = -0.25, 0.5  # bit-exactly the interior vertex (row 10, column 7)
    sim = _sim([SIS()], 16, 0.25, 2)
    packed = _rows(sim, np.array([[0.3, cx, cy], [0.7, cx, cy]]))  # h < 0.3 < h sqrt(2);  0.7 > 2 h
    fields = [CC.sis_fields(float(packed[b, 0]), cx, cy) for b in range(2)]
    raw, res, (dropped, flagged, opened) = _call(sim, packed, window, n)
    gates = _gates(sim, packed, res, fields, window)
    refs = [_compare_with_restatement(sim, packed, res, b, window=window, n_cells=n, fields=fields[b], gates=gates,
                                      expect_closed=False) for b in range(2)]
    assert all(r[1] == 0 for r in refs)
    small, big = refs[0][-1], refs[1][-1]
    assert np.isnan(small["D"][10, 7]) and np.isnan(big["D"][10, 7])
    # the axial neighbours D < 0, the diagonal ones D > 0: the four cells around the vertex are skipped and counted; no segment lies
    # in them (the cells beyond the axial neighbours still cut their corner off: four open arcs, which the restatement has too)
    assert flagged.tolist() == [small["n_flagged"], big["n_flagged"]] == [4, 0]
    assert dropped.tolist() == [0, 0] and opened.tolist() == [0, 0]
    assert res["closed"].tolist() == [False, True]
    k = int(res["n"][0])
    assert k == len(small["seg"]) == 8
    mid = res["critical"][0, :k].astype(np.float64).mean(1)
    assert np.all(np.maximum(np.abs(mid[:, 0] - cx), np.abs(mid[:, 1] - cy)) > h)
    assert not any(c[1] for c in sim.chain_curves(raw, 0)) and np.isnan(res["area_tangential"][0])
    with pytest.raises(RuntimeError, match="skipped"):
        sim.critical_curves(packed[:1], window=window, num_cells=n, strict=True)
    # theta_E > 2 h: the finite vertices of the four cells agree, nothing is flagged and the curve is contoured as usual
    assert [c[1] for c in sim.chain_curves(raw, 1)] == [True] and int(res["n"][1]) == len(big["seg"]) > 0
    _left_is_negative(res, 1, big, window, n)
    sim.critical_curves(packed[1:], window=window, num_cells=n, strict=True)


# ---- d. capacity, exact ----------------------------------------------------------------------------------------------------------------
def test_capacity_is_accounted_for_exactly():
    from gigalens_amd.profiles.mass.sis import SIS
    window, n = SQUARE, 32
    sim = _sim([SIS()], 16, 0.25, 1)
    packed = _rows(sim, np.array([[1.3, 0.11, -0.23]]))
    te, cx, cy = (float(v) for v in packed[0, :3].double().cpu())
    ref = CC.contour64(CC.sis_fields(te, cx, cy), window, n)
    assert np.abs(ref["D"]).min() >= D_MARGIN
    T = len(ref["seg"])
    assert T == len(ref["edges"]) and CC.count_loops(ref["seg"]) == (1, 0)
    fields = CC.sis_fields(te, cx, cy)
    _, full, (dropped, _, _) = _call(sim, packed, window, n, max_segments=4 * T)
    assert int(full["n"][0]) == T and dropped[0] == 0
    assert _compare_with_restatement(sim, packed, full, 0, window=window, n_cells=n, fields=fields,
                                     gates=_gates(sim, packed, full, [fields], window))[1] == 0
    seen = []
    for M in (1, T // 2 - 1, T - 1, T, T + 1, 3 * T // 10):  # (the last: some slots keep their segment, some are padding)
        raw, res, (dropped, flagged, opened) = _call(sim, packed, window, n, max_segments=M)
        k, keep, want_dropped = CC.with_capacity(ref, M)
        assert res["critical"].shape == (1, M, 2, 2)
        assert int(res["n"][0]) == k == min(T, M), (M, res["n"])
        pad = res["kind"][0] == -1
        assert np.array_equal(~pad[:k], keep), (M, np.flatnonzero(~pad[:k] != keep))
        assert pad[k:].all() and np.isnan(res["critical"][0][pad]).all() and np.isnan(res["caustic"][0][pad]).all()
        # a kept slot holds the segment the unlimited call has there, bit for bit
        for name in ("critical", "caustic", "kind"):
            assert np.array_equal(res[name][0, :k][keep], full[name][0, :k][keep]), (M, name)
        assert dropped[0] == want_dropped == (T - k) + int((~keep).sum()), (M, dropped, want_dropped)
        anything = want_dropped > 0
        assert bool(res["closed"][0]) == (not anything)
        for name in ("area_tangential", "area_radial", "caustic_area_tangential", "caustic_area_radial"):
            assert bool(np.isnan(res[name][0])) == anything, (M, name)
        if anything:
            with pytest.raises(RuntimeError, match="not returned"):
                sim.critical_curves(packed, window=window, num_cells=n, max_segments=M, strict=True)
        seen.append((M, k, int(keep.sum()), int(dropped[0])))
    print(f"T = {T}; (max_segments, n, slots holding a segment, n_dropped): {seen}")
    assert any(0 < kept < k for _, k, kept, _ in seen) and any(kept == 0 for _, _, kept, _ in seen)
