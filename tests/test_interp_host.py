"""The interpolated light (gigalens_amd/csrc/gl_interp.h) without a GPU: its float64 instantiation (tests/hostmath/interp_host.cpp, a
host build of its own) against the float64 restatement of the formula (tests/interp_cases.py), the weights' identities, the
stand-alone host program over huge, negative and non-finite coordinates, and the Python-side validation."""
import math
import subprocess

import numpy as np
import pytest
import torch

from tests import interp_cases as IC

SHAPES = [(1, 1), (2, 3), (5, 4), (16, 16)]


def _points(shape, p, r, order, grad):
    """Sky points whose pixel coordinates cover the inside of the image, its apron, the sky beyond and -- for values -- the nodes
    themselves.  ``grad`` with order 1: nodes are left out and every point keeps 1e-3 px from them (the hat's derivative jumps)."""
    h, w = shape
    u = np.concatenate([r.uniform(0, max(w - 1, 1e-3), 40), r.uniform(-2, 0, 25), r.uniform(w - 1, w + 1, 25), r.uniform(-6, w + 5, 30)])
    v = np.concatenate([r.uniform(0, max(h - 1, 1e-3), 40), r.uniform(-2, h + 1, 50), r.uniform(-6, h + 5, 30)])
    if not (grad and order == 1):
        jj, ii = np.mgrid[-2:h + 2, -2:w + 2]
        u, v = np.concatenate([u, ii.ravel().astype(float)]), np.concatenate([v, jj.ravel().astype(float)])
    else:
        for a in (u, v):
            near = np.abs(a - np.round(a)) < 1e-3
            a[near] += 3e-3
    c, s = math.cos(p[2]), math.sin(p[2])
    ur, vr = (u - 0.5 * (w - 1)) * p[3], (v - 0.5 * (h - 1)) * p[3]
    return p[0] + ur * c - vr * s, p[1] + ur * s + vr * c


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_double_instantiation_matches_the_restatement(shape, order):
    """fwd, vjp (parameter gradient and the cotangent of the evaluation point) and finalize in float64 against torch float64 autograd
    of the dense restatement: both evaluate the same polynomial, 1e-11 of amp max|image| (gradients: of their own largest entry)."""
    r = np.random.default_rng(31 * shape[0] + shape[1] + order)
    img = IC.make_image(*shape, seed=5)
    for trial in range(3):
        p = np.array([r.normal(0, 0.2), r.normal(0, 0.2), r.uniform(-math.pi, math.pi), r.uniform(0.03, 0.3), r.uniform(0.5, 20.0)])
        for grad in (False, True):
            x, y = _points(shape, p, r, order, grad)
            gI = r.normal(size=x.size)
            I, g, gpx, gpy = IC.host_light(order, img, p, x, y, gI)
            pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
            It = IC.interp_light(xt, yt, img, order, pt[0], pt[1], pt[2], pt[3], pt[4])
            scale = p[4] * float(np.abs(img).max())
            assert np.abs(I - It.detach().numpy()).max() <= 1e-11 * scale
            if grad:
                gp, gx, gy = torch.autograd.grad((It * torch.tensor(gI)).sum(), [pt, xt, yt])
                for got, want in ((g, gp.numpy()), (gpx, gx.numpy()), (gpy, gy.numpy())):
                    assert np.abs(got - want).max() <= 1e-11 * max(np.abs(want).max(), scale), (shape, order, trial)


@pytest.mark.parametrize("order", [1, 3])
def test_weights(order):
    """Partition of unity to 1e-15, derivative weights summing to zero, and w(0) = 1, w(+-1) = w(+-2) = 0 (host and restatement)."""
    for t in np.concatenate([[0.0, 0.5, 1.0 - 1e-12], np.random.default_rng(order).random(200)]):
        w, dw = IC.host_weights(order, t)
        assert abs(w.sum() - 1.0) <= 1e-15
        assert abs(dw.sum()) <= 1e-14
        want = IC.weight(torch.tensor([t + 1.0, t, t - 1.0, t - 2.0], dtype=torch.float64), order).numpy()
        assert np.abs(w - want).max() <= 1e-15
    w0, _ = IC.host_weights(order, 0.0)
    assert list(w0) == [0.0, 1.0, 0.0, 0.0]
    nodes = IC.weight(torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64), order).numpy()
    assert list(nodes) == [1.0, 0.0, 0.0, 0.0, 0.0]


def test_out_of_range_is_exactly_zero_with_zero_gradient():
    img = IC.make_image(5, 4)
    p = np.array([0.1, -0.2, 0.3, 0.1, 3.0])
    x = np.array([50.0, -50.0, 1e30, -1e300, np.inf, -np.inf, np.nan, 0.1])
    y = np.array([0.0, 50.0, 0.0, 1e300, 0.0, np.nan, 0.0, np.nan])
    I, g, gpx, gpy = IC.host_light(3, img, p, x, y, np.ones_like(x))
    assert not I.any() and not g.any() and not gpx.any() and not gpy.any()


def test_stand_alone_host_program():
    """The same source as a program of its own (the form a sanitizer build of the host code takes): every shape, both orders,
    coordinates from -1e300 to +1e300, infinities and NaN; it exits non-zero on a non-zero value outside the range."""
    out = subprocess.run([IC.interp_host_program()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 bad" in out.stdout


def test_python_validation():
    from gigalens_amd.profiles.light import Interpolated
    good = np.ones((3, 4), dtype=np.float32)
    p = Interpolated(good)
    assert p.name == "INTERPOL" and p.params == ["center_x", "center_y", "phi", "scale", "amp"] and p.order == 3
    assert p._native_params() == ["center_x", "center_y", "phi", "scale", "amp"] and p._component() == (21, 0, 0)
    q = Interpolated(good, order=1, use_lstsq=True)
    assert q.params == ["center_x", "center_y", "phi", "scale"] and q._native_params()[-1] == "amp" and q._component() == (21, 0, 1)
    for bad in (np.ones(4), np.ones((2, 3, 4)), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            Interpolated(bad)
    for v in (np.nan, np.inf):
        b = good.copy()
        b[1, 2] = v
        with pytest.raises(ValueError):
            Interpolated(b)
    for order in (0, 2, 4, "3"):
        with pytest.raises(ValueError):
            Interpolated(good, order=order)
    with pytest.raises(ValueError):
        Interpolated(np.ones((1, 2049), dtype=np.float32))


def test_abi_and_no_cpu_fallback():
    """The header, the ctypes table and the kind tables agree; without a GPU the entries raise NativeLibraryError like all others."""
    import ctypes
    from gigalens_amd import _native
    from gigalens_amd.profiles.light import Interpolated
    lib = _native.lib()
    comp = _native.gl_component(21, 0, 0, 0)
    assert lib.gl_kind_num_params(ctypes.byref(comp)) == 5
    assert lib.gl_model_set_light_image(None, 0, 1, 1, None) == -1
    assert lib.gl_interpol_eval(None, 1, 1, None, None, None, 1, 1, 0, None, None, 0, None) == -1
    if torch.cuda.is_available():
        return
    prof = Interpolated(np.ones((2, 3), dtype=np.float32))
    with pytest.raises(_native.NativeLibraryError):
        prof.light([0.0], [0.0], center_x=0.0, center_y=0.0, phi=0.0, scale=0.1, amp=1.0)
    from gigalens_amd.simulator import LensSimulator
    wl, _ = IC.case("A", "7x9")
    with pytest.raises(_native.NativeLibraryError):
        LensSimulator(wl.phys_model, wl.sim_config, bs=3)
