"""Critical curves: the C ABI's argument checks, the host-side chaining of segments and the float64 restatement of the contouring
(tests/critical_cases.py) on the closed form of the SIS.  No device needed."""
import ctypes
import math

import numpy as np
import pytest

from tests import critical_cases as CC


@pytest.fixture(scope="module")
def native():
    from gigalens_amd import _native
    try:
        _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))
    return _native


def test_critical_curves_refuses_bad_arguments(native):
    lib = native.lib()
    assert lib.gl_critical_curves_workspace_bytes(None, 4, 64, 512) == 0
    null = ctypes.c_void_p(0)
    rc = lib.gl_critical_curves(None, null, 4, -1.0, 1.0, -1.0, 1.0, 64, 512, null, null, null, null, null, null, null, null, null,
                                0, null)
    assert rc == -1  # GL_EINVAL
    assert b"null" in lib.gl_last_error()


def _loop(cx, cy, radius, k, kind):
    phi = np.linspace(0, 2 * np.pi, k, endpoint=False)
    pts = np.stack([cx + radius * np.cos(phi), cy + radius * np.sin(phi)], 1).astype(np.float32)
    return [(pts[i], pts[(i + 1) % k], kind) for i in range(k)]


def test_chain_curves_on_a_segment_soup():
    from gigalens_amd.simulator import LensSimulator
    outer, inner = _loop(0.1, -0.2, 1.5, 40, 0), _loop(0.1, -0.2, 0.4, 17, 1)
    arc_pts = np.stack([np.linspace(2.0, 3.0, 9), np.linspace(-1.0, 0.5, 9) ** 2], 1).astype(np.float32)
    arc = [(arc_pts[i], arc_pts[i + 1], 0) for i in range(8)]
    soup = outer + inner + arc
    g = np.random.default_rng(12)
    order = g.permutation(len(soup))
    flip = g.random(len(soup)) < 0.4
    M = len(soup) + 5
    seg = np.full((1, M, 2, 2), np.nan, np.float32)
    kind = np.full((1, M), -1, np.int32)
    for slot, i in enumerate(order):
        p, q, k = soup[i]
        seg[0, slot] = [q, p] if flip[i] else [p, q]
        kind[0, slot] = k
    res = {"critical": seg, "caustic": 2 * seg, "kind": kind, "n": np.array([len(soup)])}
    chains = LensSimulator.chain_curves(res, 0)
    assert len(chains) == 3
    by_len = {len(c[2]): c for c in chains}
    assert set(by_len) == {40, 17, 9}
    for k, closed, want_kind, pts in ((40, True, 0, outer), (17, True, 1, inner), (9, False, 0, None)):
        ck, cclosed, xy, beta = by_len[k]
        assert (ck, cclosed) == (want_kind, closed)
        np.testing.assert_array_equal(beta, 2 * xy)
        ref = arc_pts if pts is None else np.array([p for p, _, _ in pts])
        # the same points in the same cyclic order, in either direction
        start = int(np.flatnonzero((ref == xy[0]).all(1))[0])
        fwd = np.roll(ref, -start, 0) if closed else ref
        bwd = np.roll(ref[::-1], -(len(ref) - 1 - start), 0) if closed else ref[::-1]
        assert np.array_equal(xy, fwd) or np.array_equal(xy, bwd)


def test_float64_restatement_on_the_sis():
    theta_E, cx, cy, n, half = 1.3, 0.11, -0.23, 256, 4.0
    out = CC.contour64(CC.sis_fields(theta_E, cx, cy), (-half, half, -half, half), n)
    h = 2 * half / n
    assert not out["open"] and out["n_flagged"] == 0 and out["n_ambiguous"] == 0
    assert len(out["seg"]) > 0 and np.all(out["kind"] == 0)
    # every endpoint on the circle, the caustic a point
    r = np.hypot(out["seg"][..., 0] - cx, out["seg"][..., 1] - cy)
    assert np.max(np.abs(r - theta_E)) < 1e-12
    assert np.max(np.hypot(out["cau"][..., 0] - cx, out["cau"][..., 1] - cy)) < 1e-12
    # an inscribed polygon with chords of at most sqrt(2) h: area in [(1 - h^2 / (3 theta_E^2)), 1] pi theta_E^2, positive (D < 0 inside)
    exact = math.pi * theta_E ** 2
    assert (1 - h * h / (3 * theta_E ** 2)) * exact <= out["area"][0] <= exact
    assert out["area"][1] == 0.0 and abs(out["area"][2]) < 1e-12
    assert CC.count_loops(out["seg"]) == (1, 0)
    # D < 0 (inside the ring) on the left of every segment, from the vertex plane alone
    assert CC.orientation_violations(out["seg"], out["D"], (-half, half, -half, half), n) == []
    assert CC.physical_loops(CC.sis_fields(theta_E, cx, cy), (-half, half, -half, half)) == (1, 1)


@pytest.mark.parametrize("name", sorted(CC.AMBIGUOUS))
def test_ambiguous_variants_have_their_margin_topology_and_orientation(name):
    lenses, code, joined, curves = CC.ambiguous_case(name)
    fields = CC.multi_sis_fields(lenses)
    out = CC.contour64(fields, CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N)
    amb = CC.ambiguous_cells(out["D"])
    assert len(amb) == 1 == out["n_ambiguous"] and amb[0][2:4] == (code, joined), amb
    assert amb[0][4] >= CC.AMBIGUOUS_MARGIN and np.abs(out["D"]).min() >= CC.AMBIGUOUS_MARGIN
    assert not out["open"] and out["n_flagged"] == 0
    # topology, independently of the table: closed loops only, as many as the regions of D < 0 and D > 0 imply on a fine grid
    # (two resolutions agree), and that is the variant's: separated = two curves, joined = one
    assert CC.physical_loops(fields, CC.AMBIGUOUS_WINDOW, 256) == CC.physical_loops(fields, CC.AMBIGUOUS_WINDOW, 512) == (curves, curves)
    assert CC.count_loops(out["seg"]) == (curves, 0)
    # orientation, independently of the table
    assert CC.orientation_violations(out["seg"], out["D"], CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N) == []
    # the other variant of the same cell has the wrong number of curves: the mean rule decides the topology here
    wrong = dict(CC.JOINED) if not joined else {5: CC.CASES[5], 10: CC.CASES[10]}
    segs = []
    H = (CC.AMBIGUOUS_N + 1) * CC.AMBIGUOUS_N
    r, c = amb[0][:2]
    cell_edge = [r * CC.AMBIGUOUS_N + c, H + r * (CC.AMBIGUOUS_N + 1) + c + 1, (r + 1) * CC.AMBIGUOUS_N + c, H + r * (CC.AMBIGUOUS_N + 1) + c]
    mine = {tuple(e) for e in out["seg_edges"].tolist()}
    theirs = (mine - {(cell_edge[a], cell_edge[b]) for a, b in (CC.JOINED if joined else CC.CASES)[code]}) | \
             {(cell_edge[a], cell_edge[b]) for a, b in wrong[code]}
    for a, b in theirs:
        segs.append([out["edges"][a][:2], out["edges"][b][:2]])
    assert CC.count_loops(np.array(segs)) == (3 - curves, 0)


def test_ambiguous_cases_cover_every_nontrivial_code():
    seen = set()
    for name in CC.AMBIGUOUS:
        out = CC.contour64(CC.multi_sis_fields(CC.ambiguous_case(name)[0]), CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N)
        seen |= set(CC.cell_codes(out["D"]).ravel().tolist())
    assert seen >= set(range(1, 15)), sorted(seen)


def test_orientation_check_bites_on_a_swapped_table_row():
    """The invariant is independent of the table: a restatement whose rows 5 and 16 are swapped (separated <-> joined) still has
    D < 0 on the left, but the wrong number of curves; one whose row is reversed has the right curves and the wrong side."""
    lenses, code, joined, curves = CC.ambiguous_case("code5_joined")
    fields = CC.multi_sis_fields(lenses)
    saved = CC.JOINED[5]
    try:
        CC.JOINED[5] = CC.CASES[5]
        out = CC.contour64(fields, CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N)
        assert CC.count_loops(out["seg"]) == (2, 0) != (curves, 0)
        CC.JOINED[5] = [(b, a) for a, b in saved]
        out = CC.contour64(fields, CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N)
        assert len(CC.orientation_violations(out["seg"], out["D"], CC.AMBIGUOUS_WINDOW, CC.AMBIGUOUS_N)) == 4
    finally:
        CC.JOINED[5] = saved


def test_flagged_cells_of_an_sis_centred_on_a_vertex():
    window, n = (-2.0, 2.0, -2.0, 2.0), 16  # h = 0.25; the centre on the interior vertex (row 10, column 7)
    cx, cy, h = -0.25, 0.5, 0.25
    small = CC.contour64(CC.sis_fields(0.3, cx, cy), window, n)  # h < theta_E < h sqrt(2): axial neighbours D < 0, diagonal D > 0
    assert np.isnan(small["D"][10, 7]) and int(np.isnan(small["D"]).sum()) == 1
    # the four cells around the centre are skipped and counted; the cells beyond the axial neighbours still cut their corner off:
    # eight segments, four open arcs
    assert small["n_flagged"] == 4 and not small["open"] and len(small["edges"]) == 12
    assert len(small["seg"]) == 8 and CC.count_loops(small["seg"]) == (0, 4)
    mid = small["seg"].mean(1)
    assert np.all(np.maximum(np.abs(mid[:, 0] - cx), np.abs(mid[:, 1] - cy)) > h)  # none inside the four flagged cells
    big = CC.contour64(CC.sis_fields(0.7, cx, cy), window, n)  # theta_E > 2 h: the finite vertices of the four cells agree
    assert big["n_flagged"] == 0 and len(big["seg"]) > 0 and CC.count_loops(big["seg"]) == (1, 0)
    assert CC.orientation_violations(big["seg"], big["D"], window, n) == []


def test_capacity_restatement():
    ref = CC.contour64(CC.sis_fields(1.3, 0.11, -0.23), (-2.0, 2.0, -2.0, 2.0), 32)
    T = len(ref["seg"])
    assert T == len(ref["edges"])  # a closed curve: as many crossing edges as segments
    for M in (T, T + 1):
        n, keep, dropped = CC.with_capacity(ref, M)
        assert (n, dropped) == (T, 0) and keep.all()
    n, keep, dropped = CC.with_capacity(ref, T - 1)
    assert (n, dropped) == (T - 1, 1) and keep.all()  # 2 (T - 1) >= T: every edge kept, one segment beyond the slots
    # 2 (T / 2 - 1) < T: the edge list overflows, by the two largest ids (vertical edges of the top row), which none of the first
    # T / 2 - 1 segments touches
    n, keep, dropped = CC.with_capacity(ref, T // 2 - 1)
    assert n == T // 2 - 1 and keep.all() and dropped == T - n
    # fewer edges: slots whose endpoint fell off the list are padding and count as dropped, the others hold their segment
    n, keep, dropped = CC.with_capacity(ref, 3 * T // 10)
    assert n == 3 * T // 10 and 0 < keep.sum() < n and dropped == (T - n) + int((~keep).sum())
    n, keep, dropped = CC.with_capacity(ref, 1)  # two horizontal edges kept; the first segment ends on a vertical one
    assert n == 1 and not keep[0] and dropped == T
