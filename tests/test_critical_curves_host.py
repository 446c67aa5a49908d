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
