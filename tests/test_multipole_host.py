"""The multipole (gigalens_amd/csrc/gl_multipole.h) without a GPU: its float64 and Dual<double, 2> instantiations
(tests/hostmath/multipole_host.cpp, a host build of its own) against the float64 restatement of the formula
(tests/multipole_cases.py, which uses atan2 / cos / sin and so shares nothing with the kernels' recurrence), the identities of the
profile, the hand-written VJP against autograd, the exact zeros at the centre, the stand-alone host program (a sanitizer build), the
Python-side validation, the packing and the ABI."""
import subprocess

import numpy as np
import pytest
import torch

from tests import multipole_cases as MC

ORDERS = [2, 3, 4, 8]
GATE = 1e-11  # of the case's scale: both sides evaluate the same closed form in float64 (the gate of tests/test_interpmass_host.py)
# (a_m, phi_m): either sign of a_m, a_m = 0, |phi_m| > pi
PARAMS = [(0.04, 0.3), (-0.03, -2.1), (0.0, 1.0), (0.05, 4.4), (-0.02, -5.9)]


def _case(m, trial):
    r = np.random.default_rng(17 * m + trial)
    a, ph = PARAMS[trial % len(PARAMS)]
    p = np.array([a, ph, r.normal(0, 0.2), r.normal(0, 0.2)])
    rad = np.concatenate([r.uniform(0.05, 3.0, 150), 10.0 ** r.uniform(-6, 3, 50)])
    ang = r.uniform(-np.pi, np.pi, rad.size)
    return r, p, p[2] + rad * np.cos(ang), p[3] + rad * np.sin(ang)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("m", ORDERS)
def test_double_instantiation_matches_the_restatement(m):
    """fwd and pot in float64 against the restatement: 1e-11 of |a_m| (the deflection) and of |a_m| max r (the potential)."""
    for trial in range(len(PARAMS)):
        r, p, x, y = _case(m, trial)
        ax, ay, psi, _, _, _ = MC.host_eval(m, p, x, y, np.zeros_like(x), np.zeros_like(x))
        tx, ty = MC.deflection(_t(x), _t(y), m, *p)
        tp = MC.potential(_t(x), _t(y), m, *p)
        scale = abs(p[0])
        assert np.abs(ax - tx.numpy()).max() <= GATE * scale and np.abs(ay - ty.numpy()).max() <= GATE * scale, (m, trial)
        assert np.abs(psi - tp.numpy()).max() <= GATE * scale * np.hypot(x - p[2], y - p[3]).max(), (m, trial)


@pytest.mark.parametrize("m", ORDERS)
def test_dual_derivatives_and_identities(m):
    """Dual<double, 2> through multipole_fwd is the closed-form Hessian and autograd's; the gradient of multipole_pot is
    multipole_fwd; x . alpha = psi at 1e-12; the trace of the Hessian is a_m C / r."""
    for trial in range(len(PARAMS)):
        r, p, x, y = _case(m, trial)
        jet = MC.host_jet(m, p, x, y)
        xt, yt = _t(x, True), _t(y, True)
        tx, ty = MC.deflection(xt, yt, m, *p)
        fxx, fxy = torch.autograd.grad(tx.sum(), [xt, yt], retain_graph=True)
        fyx, fyy = torch.autograd.grad(ty.sum(), [xt, yt])
        closed = MC.hessian_closed(_t(x), _t(y), m, *p)
        rad = np.hypot(x - p[2], y - p[3])
        a = abs(p[0])
        for k, (auto, cl) in enumerate(zip((fxx, fxy, fyx, fyy), closed)):
            # a second derivative carries 1 / r
            assert (np.abs(jet[2 + k] - auto.numpy()) * rad).max() <= GATE * max(a, 1e-300) * m, (m, trial, k)
            assert (np.abs(jet[2 + k] - cl.numpy()) * rad).max() <= GATE * max(a, 1e-300) * m, (m, trial, k)
        assert np.abs(jet[7] - jet[0]).max() <= GATE * a and np.abs(jet[8] - jet[1]).max() <= GATE * a  # grad psi = alpha
        euler = (x - p[2]) * jet[0] + (y - p[3]) * jet[1] - jet[6]
        assert (np.abs(euler) / rad).max() <= 1e-12 * a, (m, trial)
        phi = np.arctan2(y - p[3], x - p[2])
        assert (np.abs(jet[2] + jet[5] - p[0] * np.cos(m * (phi - p[1])) / rad) * rad).max() <= GATE * a * m
        assert np.abs(jet[3] - jet[4]).max() == 0.0 or (np.abs(jet[3] - jet[4]) * rad).max() <= GATE * a  # symmetric


@pytest.mark.parametrize("m", ORDERS)
def test_symmetries_of_the_field(m):
    """phi_m -> phi_m + 2 pi / m leaves the field unchanged; (a_m, phi_m) -> (-a_m, phi_m + pi / m) gives the same field."""
    r, p, x, y = _case(m, 0)
    z = np.zeros_like(x)
    base = MC.host_eval(m, p, x, y, z, z)[:3]
    for q in (np.array([p[0], p[1] + 2 * np.pi / m, p[2], p[3]]), np.array([-p[0], p[1] + np.pi / m, p[2], p[3]])):
        other = MC.host_eval(m, q, x, y, z, z)[:3]
        rad = np.hypot(x - p[2], y - p[3])
        assert np.abs(other[0] - base[0]).max() <= GATE * abs(p[0]) and np.abs(other[1] - base[1]).max() <= GATE * abs(p[0])
        assert (np.abs(other[2] - base[2]) / rad).max() <= GATE * abs(p[0])


@pytest.mark.parametrize("m", ORDERS)
def test_vjp_and_finalize_match_autograd(m):
    """multipole_vjp followed by multipole_finalize against autograd of the restatement for random cotangents: the four parameter
    gradients and the cotangent of every point -- a_m = 0, a_m < 0 and |phi_m| > pi among the rows."""
    for trial in range(len(PARAMS)):
        r, p, x, y = _case(m, trial)
        keep = np.hypot(x - p[2], y - p[3]) > 1e-3  # (the point cotangent carries 1 / r: gated where float64 holds 1e-11 of it)
        x, y = x[keep], y[keep]
        gx, gy = r.normal(size=x.size), r.normal(size=x.size)
        _, _, _, g, gpx, gpy = MC.host_eval(m, p, x, y, gx, gy)
        pt, xt, yt = _t(p, True), _t(x, True), _t(y, True)
        tx, ty = MC.deflection(xt, yt, m, pt[0], pt[1], pt[2], pt[3])
        gp, dx, dy = torch.autograd.grad((tx * _t(gx) + ty * _t(gy)).sum(), [pt, xt, yt])
        assert np.isfinite(g).all()
        for got, want in ((g, gp.numpy()), (gpx, dx.numpy()), (gpy, dy.numpy())):
            assert np.abs(got - want).max() <= GATE * max(np.abs(want).max(), 1.0), (m, trial)
        if p[0] == 0.0:  # d / d a_m stays the field of unit amplitude
            assert abs(g[0]) > 1e-3 and g[1] == 0.0 and g[2] == 0.0 and g[3] == 0.0


@pytest.mark.parametrize("m", ORDERS)
def test_the_centre_gives_exact_zeros(m):
    p = np.array([0.04, 0.7, 0.125, -0.25])
    x, y = np.array([p[2]]), np.array([p[3]])
    ax, ay, psi, g, gpx, gpy = MC.host_eval(m, p, x, y, np.array([1.3]), np.array([-0.7]))
    for v in (ax, ay, psi, g, gpx, gpy):
        assert not v.any()
    assert not MC.host_jet(m, p, x, y).any()
    tx, ty = MC.deflection(_t(x), _t(y), m, *p)
    assert not tx.numpy().any() and not ty.numpy().any() and not MC.potential(_t(x), _t(y), m, *p).numpy().any()


def test_stand_alone_host_program_under_the_sanitizers():
    """The same source as a program of its own, built with -fsanitize=address,undefined: every order on float, Dual<float, 2>, the
    nested dual and the wide dual, from the centre to 3e18; it exits non-zero on a sanitizer report, a non-zero value at the centre, a
    value that is not finite elsewhere or a breach of x . alpha = psi."""
    out = subprocess.run([MC.host_program()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 bad" in out.stdout


def test_python_validation():
    from gigalens_amd.profiles.mass import Multipole
    p = Multipole()
    assert p.m == 4 and p.name == "MULTIPOLE" and p.params == ["a_m", "phi_m", "center_x", "center_y"]
    assert p._component() == (15, 4, 0) and Multipole(m=3)._component() == (15, 3, 0)
    for m in (2, 8, np.int64(5)):
        assert Multipole(m).m == int(m)
    for bad in (1, 0, 9, 2.5, -4, "4", None, True):
        with pytest.raises(ValueError):
            Multipole(bad)


def test_packing_has_four_columns_in_params_order():
    wl, rows = MC.case("ESM", "16x16")
    lay = wl.phys_model._packing()
    assert lay.P == rows.shape[1] == 6 + 2 + 4 + 7
    assert [(s[0], s[1], s[2]) for s in lay.slots[8:12]] == [("lens_mass", 2, n) for n in ("a_m", "phi_m", "center_x", "center_y")]


def test_abi_and_no_cpu_fallback():
    """The header, the ctypes table and the kind tables agree; an order outside 2..8 is an error of the library as well; without a
    GPU the entries raise NativeLibraryError like all others."""
    import ctypes
    from gigalens_amd import _native
    from gigalens_amd.profiles.mass import Multipole
    lib = _native.lib()
    assert _native.GL_MULTIPOLE == 15
    assert lib.gl_kind_num_params(ctypes.byref(_native.gl_component(15, 4, 0, 0))) == 4
    for m in (2, 3, 8):
        assert lib.gl_kind_num_params(ctypes.byref(_native.gl_component(15, m, 0, 0))) == 4
    for m in (1, 0, 9, -3):
        assert lib.gl_kind_num_params(ctypes.byref(_native.gl_component(15, m, 0, 0))) < 0
    if torch.cuda.is_available():
        return
    with pytest.raises(_native.NativeLibraryError):
        Multipole().deriv([0.3], [0.2], a_m=0.02, phi_m=0.1, center_x=0.0, center_y=0.0)
    from gigalens_amd.simulator import LensSimulator
    wl, _ = MC.case("ESM", "16x16")
    with pytest.raises(_native.NativeLibraryError):
        LensSimulator(wl.phys_model, wl.sim_config, bs=3)


@pytest.mark.parametrize("name", list(MC.PIXEL_CASES) + ["node"])
def test_float32_restatement_meets_the_gpu_gates(name):
    """The inputs of tests/test_gpu_multipole.py, checked without a GPU: the restatement run in float32 passes the gradient gate
    those tests apply to the kernels, with no more than COND_CAP of a case's elements excused by the conditioning bound."""
    from tests import helpers as H
    from tests.multilens_grad_cases import GRAD_RTOL_COL
    c = MC.pixel_data(name)
    fns = {"g": lambda sh: MC.loglike_and_grad(c["wl"], c["packed"], c["obs"], psf=c["psf"], grid_shift=sh, mask=c["mask"])[2],
           "g_img": lambda sh: MC.image_vjp(c["wl"], c["packed"], c["cot"], psf=c["psf"], grid_shift=sh)[1]}
    for key, fn in fns.items():
        ok, rep = H.grad_gate(c[key + "32"], c[key], GRAD_RTOL_COL, lambda S: MC.conditioning_bound(c["wl"], fn, c[key], S))
        print(name, key, rep)
        assert ok and rep["conditioned"] <= MC.COND_CAP * c[key].size, (name, key, rep)
