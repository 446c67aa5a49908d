"""The interpolated lens (gigalens_amd/csrc/gl_interp_mass.h) without a GPU: its float64 and Dual<double, 2> instantiations
(tests/hostmath/interpmass_host.cpp, a host build of its own) against the float64 restatement of the formula
(tests/interpmass_cases.py), known answers that pin sign, pitch, the row / column convention and the centre, the stand-alone host
program (a sanitizer build) over huge, negative and non-finite coordinates, the Python-side validation and the packing."""
import subprocess

import numpy as np
import pytest
import torch

from tests import interpmass_cases as MC

SHAPES = [(1, 1), (2, 3), (5, 4), (16, 16)]
GATE = 1e-11  # of the case's scale: both sides evaluate the same polynomial in float64 (the gate of tests/test_interp_host.py)


def _points(shape, pitch, p, r, nodes, clear):
    """Sky points whose pixel coordinates cover the inside of the maps, their apron and the sky beyond; ``nodes``: the nodes
    themselves as well (values only); ``clear``: every point keeps 1e-3 px from the node lines (second derivatives jump there)."""
    h, w = shape
    u = np.concatenate([r.uniform(0, max(w - 1, 1e-3), 40), r.uniform(-2, 0, 25), r.uniform(w - 1, w + 1, 25), r.uniform(-6, w + 5, 30)])
    v = np.concatenate([r.uniform(0, max(h - 1, 1e-3), 40), r.uniform(-2, h + 1, 50), r.uniform(-6, h + 5, 30)])
    if nodes:
        jj, ii = np.mgrid[-2:h + 2, -2:w + 2]
        u, v = np.concatenate([u, ii.ravel().astype(float)]), np.concatenate([v, jj.ravel().astype(float)])
    if clear:
        for a in (u, v):
            near = np.abs(a - np.round(a)) < 1e-3
            a[near] += 3e-3
    return p[1] + (u - 0.5 * (w - 1)) * pitch, p[2] + (v - 0.5 * (h - 1)) * pitch


def _case(shape, trial):
    r = np.random.default_rng(31 * shape[0] + shape[1] + 100 * trial)
    pitch = float(r.uniform(0.03, 0.3))
    ax, ay = MC.make_maps(*shape, pitch, seed=5 + trial)
    p = np.array([r.uniform(0.5, 2.0), r.normal(0, 0.2), r.normal(0, 0.2)])
    return r, pitch, ax, ay, p


@pytest.mark.parametrize("shape", SHAPES)
def test_double_instantiation_matches_the_restatement(shape):
    """fwd, vjp (parameter gradient and the cotangent of the evaluation point) and finalize in float64 against torch float64 autograd
    of the dense restatement: 1e-11 of scale_factor max|map| (gradients: of their own largest entry, at least that scale)."""
    for trial in range(3):
        r, pitch, ax, ay, p = _case(shape, trial)
        for grad in (False, True):
            x, y = _points(shape, pitch, p, r, nodes=not grad, clear=False)
            gx, gy = r.normal(size=x.size), r.normal(size=x.size)
            hx, hy, g, gpx, gpy = MC.host_deflection(ax, ay, pitch, p, x, y, gx, gy)
            pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
            tx, ty = MC.deflection(xt, yt, ax, ay, pitch, pt[0], pt[1], pt[2])
            scale = p[0] * float(max(np.abs(ax).max(), np.abs(ay).max()))
            assert np.abs(hx - tx.detach().numpy()).max() <= GATE * scale
            assert np.abs(hy - ty.detach().numpy()).max() <= GATE * scale
            if grad:
                gp, dx, dy = torch.autograd.grad((tx * torch.tensor(gx) + ty * torch.tensor(gy)).sum(), [pt, xt, yt])
                for got, want in ((g, gp.numpy()), (gpx, dx.numpy()), (gpy, dy.numpy())):
                    assert np.abs(got - want).max() <= GATE * max(np.abs(want).max(), scale), (shape, trial)


@pytest.mark.parametrize("shape", SHAPES)
def test_dual_derivatives_are_the_hessian_of_the_restatement(shape):
    """Dual<double, 2> through interpmass_fwd: values as the plain instantiation, d alpha / d (x, y) as autograd of the restatement."""
    for trial in range(2):
        r, pitch, ax, ay, p = _case(shape, trial)
        x, y = _points(shape, pitch, p, r, nodes=False, clear=True)
        jet = MC.host_jet(ax, ay, pitch, p, x, y)
        want = MC.lens_maps(_One(ax, ay, pitch), torch.tensor(p[None]), x, y)[:, :, 0].numpy()
        scale = p[0] * float(max(np.abs(ax).max(), np.abs(ay).max()))
        assert np.abs((x - jet[0]) - want[0]).max() <= GATE * max(scale, np.abs(x).max())
        assert np.abs((y - jet[1]) - want[1]).max() <= GATE * max(scale, np.abs(y).max())
        for k in range(4):
            assert np.abs(jet[2 + k] - want[2 + k]).max() <= GATE * max(np.abs(want[2:]).max(), scale), (shape, trial, k)


class _One:
    """A one-lens model as ``interpmass_cases.maps_of`` reads it."""
    def __init__(self, ax, ay, pitch):
        self.lenses = [type("L", (), dict(name=MC.NAME, params=["scale_factor", "center_x", "center_y"], alpha_x=ax, alpha_y=ay, pitch=pitch))()]


@pytest.mark.parametrize("field", ["linear", "quadratic"])
def test_known_fields_are_reproduced(field):
    """Keys' kernel reproduces quadratics: maps sampled from a linear (shear) and from a quadratic field give the field and its
    first derivatives back wherever 1 <= u <= W - 2 and 1 <= v <= H - 2 -- with the centre moved, a scale factor and +x = increasing
    column, +y = increasing row.  Every sample is exact in float32 (dyadic coefficients and pitch), so the gate is float64 rounding
    of the sixteen-term sum alone: 1e-13 of the largest field value on the map (~450 eps; a convention error is of order 1)."""
    shape, pitch = (7, 9), 0.25
    g1, g2, q = 0.125, -0.0625, 0.03125
    if field == "linear":
        fn = lambda X, Y: (g1 * X + g2 * Y, g2 * X - g1 * Y)
        hess = lambda X, Y: (g1 + 0 * X, g2 + 0 * X, g2 + 0 * X, -g1 + 0 * X)
    else:
        fn = lambda X, Y: (q * X * X - 2 * q * X * Y + g1 * Y, 0.5 * q * Y * Y + q * X * Y - g2 * X + 0.25)
        hess = lambda X, Y: (2 * q * X - 2 * q * Y, -2 * q * X + g1, q * Y - g2, q * Y + q * X)
    ax, ay = MC.sampled(shape, pitch, fn)
    X, Y = MC.node_coords(shape, pitch)
    assert np.array_equal(ax.astype(np.float64), fn(X, Y)[0]) and np.array_equal(ay.astype(np.float64), fn(X, Y)[1])
    r = np.random.default_rng(3)
    cx, cy, sf = 0.375, -0.625, 1.5
    u, v = r.uniform(1, shape[1] - 2, 300), r.uniform(1, shape[0] - 2, 300)
    dx, dy = (u - 0.5 * (shape[1] - 1)) * pitch, (v - 0.5 * (shape[0] - 1)) * pitch
    jet = MC.host_jet(ax, ay, pitch, [sf, cx, cy], cx + dx, cy + dy)
    scale = sf * float(max(np.abs(ax).max(), np.abs(ay).max()))
    wx, wy = fn(dx, dy)
    assert np.abs(jet[0] - sf * wx).max() <= 1e-13 * scale
    assert np.abs(jet[1] - sf * wy).max() <= 1e-13 * scale
    for k, want in enumerate(hess(dx, dy)):  # a derivative carries 1 / pitch
        assert np.abs(jet[2 + k] - sf * want).max() <= 1e-13 * scale / pitch, k


def test_out_of_range_is_exactly_zero_with_zero_gradient():
    ax, ay = MC.make_maps(5, 4, 0.1)
    p = np.array([1.2, 0.1, -0.2])
    x = np.array([50.0, -50.0, 1e30, -1e300, np.inf, -np.inf, np.nan, 0.1])
    y = np.array([0.0, 50.0, 0.0, 1e300, 0.0, np.nan, 0.0, np.nan])
    hx, hy, g, gpx, gpy = MC.host_deflection(ax, ay, 0.1, p, x, y, np.ones_like(x), np.ones_like(x))
    assert not hx.any() and not hy.any() and not g.any() and not gpx.any() and not gpy.any()
    assert not MC.host_jet(ax, ay, 0.1, p, x, y).any()


def test_stand_alone_host_program_under_the_sanitizers():
    """The same source as a program of its own, built with -fsanitize=address,undefined: the float and Dual<float, 2>
    instantiations over coordinates from -3.4e38 to +3.4e38, infinities and NaN; it exits non-zero on a sanitizer report or on a
    non-zero value outside the range."""
    out = subprocess.run([MC.host_program()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 bad" in out.stdout


def test_python_validation():
    from gigalens_amd import _native
    from gigalens_amd.profiles.mass import Interpolated
    from gigalens_amd.profiles.mass.scaling_relation import ScalingRelation
    good = np.ones((3, 4), dtype=np.float32)
    p = Interpolated(good, 2 * good, 0.1)
    assert p.name == "INTERPOL_SCALED" and p.params == ["scale_factor", "center_x", "center_y"]
    assert p._component() == (14, 0, 0) and p.alpha_x.dtype == np.float32 and p.pitch == 0.1
    for bad in (np.ones(4), np.ones((2, 3, 4)), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            Interpolated(bad, bad, 0.1)
    with pytest.raises(ValueError):
        Interpolated(good, np.ones((4, 3), dtype=np.float32), 0.1)
    for v in (np.nan, np.inf):
        b = good.copy()
        b[1, 2] = v
        with pytest.raises(ValueError):
            Interpolated(b, good, 0.1)
        with pytest.raises(ValueError):
            Interpolated(good, b, 0.1)
    for pitch in (0.0, -0.1, np.nan, np.inf, 1e-60, "x"):
        with pytest.raises(ValueError):
            Interpolated(good, good, pitch)
    big = np.ones((1, 2049), dtype=np.float32)
    with pytest.raises(ValueError):
        Interpolated(big, big, 0.1)
    with pytest.raises(_native.UnsupportedLensError, match="INTERPOL_SCALED"):
        p.potential([0.0], [0.0], scale_factor=1.0, center_x=0.0, center_y=0.0)
    with pytest.raises(_native.UnsupportedLensError, match="INTERPOL_SCALED"):
        ScalingRelation(p, ["scale_factor"], 1.0, {"scale_factor": 0.5}, {"lum": [1.0], "center_x": [0.0], "center_y": [0.0]})


def test_packing_has_three_columns_in_params_order():
    wl, rows = MC.case("IS", "7x9")
    lay = wl.phys_model._packing()
    assert lay.P == rows.shape[1] == 3 + 5 + 5
    assert [(s[0], s[1], s[2]) for s in lay.slots[:3]] == [("lens_mass", 0, "scale_factor"), ("lens_mass", 0, "center_x"),
                                                          ("lens_mass", 0, "center_y")]


def test_abi_and_no_cpu_fallback():
    """The header, the ctypes table and the kind tables agree; without a GPU the entries raise NativeLibraryError like all others."""
    import ctypes
    from gigalens_amd import _native
    from gigalens_amd.profiles.mass import Interpolated
    lib = _native.lib()
    comp = _native.gl_component(14, 0, 0, 0)
    assert _native.GL_INTERPOL_MASS == 14 and lib.gl_kind_num_params(ctypes.byref(comp)) == 3
    assert lib.gl_model_set_lens_maps(None, 0, 1, 1, None, None, 0.1) == -1
    assert lib.gl_interpol_mass_eval(None, 1, 1, None, None, 0.1, None, None, 1, 1, 0, None, None, None, 0, None) == -1
    if torch.cuda.is_available():
        return
    prof = Interpolated(np.ones((2, 3), dtype=np.float32), np.ones((2, 3), dtype=np.float32), 0.1)
    with pytest.raises(_native.NativeLibraryError):
        prof.deriv([0.0], [0.0], scale_factor=1.0, center_x=0.0, center_y=0.0)
    from gigalens_amd.simulator import LensSimulator
    wl, _ = MC.case("I", "7x9")
    with pytest.raises(_native.NativeLibraryError):
        LensSimulator(wl.phys_model, wl.sim_config, bs=3)
