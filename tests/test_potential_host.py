"""Lensing potential templates (*_pot of gl_profiles.h, gl_dpie.h, gl_extra.h), instantiated in float64 on the host by
tests/hostmath/potential_host.cpp, against the float64 oracle: for every built-in kind the gradient of psi is the oracle's
deflection, the Laplacian is twice the oracle's convergence where it has one, and the closed forms hold.  Pure CPU."""
import numpy as np
import pytest
import torch

from oracle import ref_torch as ref
from tests.potential_cases import (KINDS, gauss_legendre_delta, host_psi, host_psi_scaled, oracle_alpha, points_away,
                                   row_to_kwargs)


def _centre(name, p):
    kw = row_to_kwargs(name, p)
    return (kw.get("center_x", 0.0), kw.get("center_y", 0.0))


def _grad5(f, x, y, h):
    gx = (-f(x + 2 * h, y) + 8 * f(x + h, y) - 8 * f(x - h, y) + f(x - 2 * h, y)) / (12 * h)
    gy = (-f(x, y + 2 * h) + 8 * f(x, y + h) - 8 * f(x, y - h) + f(x, y - 2 * h)) / (12 * h)
    return gx, gy


def _lap5(f, x, y, h):
    f0 = f(x, y)
    dxx = (-f(x + 2 * h, y) + 16 * f(x + h, y) - 30 * f0 + 16 * f(x - h, y) - f(x - 2 * h, y)) / (12 * h * h)
    dyy = (-f(x, y + 2 * h) + 16 * f(x, y + h) - 30 * f0 + 16 * f(x, y - h) - f(x, y - 2 * h)) / (12 * h * h)
    return dxx + dyy


@pytest.mark.parametrize("name", list(KINDS))
def test_gradient_of_psi_is_the_oracle_deflection(name):
    """Fourth-order central differences of psi (step h) against the oracle's float64 mass_deriv, random parameters within and
    well beyond the priors, points at least r_min from the centre.  Error budget: h^4 psi^(5) / 30 plus the rounding of psi over
    h.  TNFW: its g(X) cancels from O(ln X) to O(X^2 ln X) near the centre, so psi carries float64 noise ~1e-9 relative there
    that a small step amplifies; a larger step and r_min keep both terms near 1e-7."""
    kind, _, sample = KINDS[name]
    h, r_min, tol = (1e-2, 0.3, 5e-7) if name == "TNFW" else (1e-3, 0.2, 1e-7)
    r = np.random.default_rng(100 + kind)
    for _ in range(25):
        p = sample(r)
        x, y = points_away(r, 40, _centre(name, p), r_min)
        gx, gy = _grad5(lambda u, v: host_psi(kind, p, u, v), x, y, h)
        ax, ay = oracle_alpha(name, p, x, y)
        a = np.hypot(ax, ay)
        err = np.hypot(gx - ax, gy - ay) / np.maximum(a, 1e-3 * a.max())
        assert err.max() < tol, (name, p, float(err.max()))


@pytest.mark.parametrize("name", list(KINDS))
def test_psi_differences_are_line_integrals_of_the_oracle_deflection(name):
    """psi(B) - psi(A) equals the float64 Gauss-Legendre line integral of the oracle's deflection along A -> B (no step to
    amplify rounding: this pins the constant-free part of psi to ~1e-10 of the lens's |psi|; TNFW to 1e-8, the float64 noise of
    its g(X) near the centre, in the oracle's deflection and in psi alike)."""
    kind, _, sample = KINDS[name]
    tol = 1e-8 if name == "TNFW" else 1e-9
    r = np.random.default_rng(200 + kind)
    for _ in range(10):
        p = sample(r)
        c = _centre(name, p)
        xa, ya = points_away(r, 20, c, 0.3)
        xb, yb = points_away(r, 20, c, 0.3)
        # keep segments clear of the centre (the SIS / SIE / EPL / dPIS deflections are singular or NaN there)
        d = np.abs((xb - xa) * (ya - c[1]) - (yb - ya) * (xa - c[0])) / np.hypot(xb - xa, yb - ya)
        keep = d > 0.1
        xa, ya, xb, yb = xa[keep], ya[keep], xb[keep], yb[keep]
        want = gauss_legendre_delta(lambda u, v: oracle_alpha(name, p, u, v), xa, ya, xb, yb)
        pa, pb = host_psi(kind, p, xa, ya), host_psi(kind, p, xb, yb)
        scale = np.abs(pa) + np.abs(pb) + np.abs(want) + 1e-12
        assert np.all(np.abs((pb - pa) - want) < tol * scale), (name, p)


def test_laplacian_is_twice_the_oracle_convergence():
    """dPIE: Laplacian of psi = 2 kappa (piemd.py:140-149).  dPIS: the reference's convergence carries a factor (rc + rt) / rt
    that its deflection does not have (piemd.py:85-94, dpis_kappa_excess); psi follows the deflection, so its Laplacian is
    2 kappa rt / (rc + rt) with the sorted radii."""
    r = np.random.default_rng(7)
    for name in ("dPIE", "dPIS"):
        kind, _, sample = KINDS[name]
        for _ in range(15):
            p = sample(r)
            kw = row_to_kwargs(name, p)
            x, y = points_away(r, 30, _centre(name, p), 0.3)
            lap = _lap5(lambda u, v: host_psi(kind, p, u, v), x, y, 1e-2)
            xt, yt = torch.as_tensor(x), torch.as_tensor(y)
            if name == "dPIE":
                want = 2 * ref.dpie_convergence(xt, yt, **kw).numpy()
            else:
                rc, rt = ref._sort_ra_rs(torch.tensor(kw["r_core"], dtype=torch.float64), torch.tensor(kw["r_cut"], dtype=torch.float64))
                want = 2 * ref.dpis_convergence(xt, yt, **kw).numpy() * float(rt / (rc + rt))
            assert np.allclose(lap, want, rtol=1e-6, atol=1e-7 * np.abs(want).max()), (name, p)


def test_catalogue_psi_is_the_member_sum():
    """A DPIESubhalo catalogue (the fused K_SCALED lens): grad psi = the oracle's scaled_deriv."""
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    from gigalens_amd.profiles.mass.piep import DPIEP
    from gigalens_amd.profiles.mass.scaling_relation import ScalingRelation
    r = np.random.default_rng(3)
    G = 9
    cat = {"lum": r.uniform(0.2, 3.0, G), "center_x": r.uniform(-4, 4, G), "center_y": r.uniform(-4, 4, G),
           "e1": r.uniform(-0.3, 0.3, G), "e2": r.uniform(-0.3, 0.3, G)}
    profs = [DPIESubhalo(lum_star=1.0, galaxy_catalogue=cat),
             ScalingRelation(DPIEP(), ["theta_E", "Rs"], 1.0, {"theta_E": 0.5, "Rs": 0.5},
                             dict(cat, Ra=r.uniform(0.01, 0.2, G)))]
    for prof, scales in zip(profs, ([1.2, 0.05, 8.0], [0.9, 6.0])):
        base_kind, cols, table = prof._catalogue()
        x, y = r.uniform(-5, 5, 400), r.uniform(-5, 5, 400)
        dmin = np.min(np.hypot(x[:, None] - cat["center_x"][None], y[:, None] - cat["center_y"][None]), axis=1)
        x, y = x[dmin > 0.2], y[dmin > 0.2]
        gx, gy = _grad5(lambda u, v: host_psi_scaled(base_kind, cols, table, scales, u, v), x, y, 1e-3)
        kw = dict(zip(prof.params, scales))
        ax, ay = ref.scaled_deriv(prof, torch.as_tensor(x), torch.as_tensor(y), **kw)
        ax, ay = ax.numpy(), ay.numpy()
        a = np.hypot(ax, ay)
        assert np.all(np.hypot(gx - ax, gy - ay) < 1e-7 * np.maximum(a, 1e-3 * a.max())), prof.name


def test_closed_forms_sis_and_shear():
    r = np.random.default_rng(11)
    x, y = r.uniform(-5, 5, 200), r.uniform(-5, 5, 200)
    te, cx, cy = 1.37, 0.21, -0.4
    assert np.array_equal(host_psi(5, [te, cx, cy], x, y), te * np.sqrt((x - cx) ** 2 + (y - cy) ** 2))
    g1, g2 = 0.07, -0.031
    assert np.allclose(host_psi(4, [g1, g2], x, y), 0.5 * g1 * (x * x - y * y) + g2 * x * y, rtol=1e-15, atol=1e-15)


def test_time_delay_unit_constant():
    """D_dt / c * arcsec^2 in days per Mpc, derived in float64 from the IAU astronomical unit and the exact c."""
    from gigalens_amd.simulator import LensSimulator
    pc = 648000.0 / np.pi * 149597870700.0
    want = pc * 1e6 / 299792458.0 * (np.pi / 180 / 3600) ** 2 / 86400.0
    assert LensSimulator.DAYS_PER_MPC_ARCSEC2 == pytest.approx(want, rel=1e-15)
    assert LensSimulator.DAYS_PER_MPC_ARCSEC2 == pytest.approx(0.0280005030, rel=1e-9)
