"""Lens-equation solver (LensSimulator.image_positions, gl_image_positions): the images of a source for every sample, against the
closed form of the SIS and the float64 Newton solver of tests/images_cases.py on the oracle's deflections (Hessians from
torch.autograd), plus the family-level diagnostics of ForwardProbModel (predicted_positions, image_plane_rms) and the refusals."""
import warnings

import numpy as np
import pytest
import torch

from tests import helpers as H
# the float64 Newton reference lives in tests/images_cases.py (shared with tests/test_gpu_images_edges.py)
from tests.images_cases import _check_against_f64, _default_tol, _deriv64, _lens_rows, _residual64, _solve64  # noqa: F401

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS32 = float(np.finfo(np.float32).eps)


def _sim(lenses, num_pix, delta_pix, bs, constants=None):
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.simulator import LensSimulator, SimulatorConfig
    phys = PhysicalModel(lenses, [], [Sersic()], lenses_constants=constants)
    return LensSimulator(phys, SimulatorConfig(delta_pix=delta_pix, num_pix=num_pix), bs=bs)


def _rows(sim, lens_cols):
    """Packed [B, P] rows from the lens columns; the source columns (unused by the solver) get a valid Sersic."""
    B = lens_cols.shape[0]
    src = np.tile(np.array([[0.2, 2.0, 0.0, 0.0, 1.0]], np.float32), (B, 1))
    return torch.tensor(np.concatenate([np.asarray(lens_cols, np.float32), src], 1), device=sim.device)


def test_sis_closed_form():
    from gigalens_amd.profiles.mass.sis import SIS
    B = 256
    sim = _sim([SIS()], 64, 0.08, B)
    g = np.random.default_rng(3)
    theta_E = g.uniform(0.6, 1.2, B)
    cx, cy = g.uniform(-0.3, 0.3, B), g.uniform(-0.3, 0.3, B)
    # inside the Einstein radius (two images) and outside it (one), away from |beta| ~ theta_E where the inner image
    # approaches the singular centre closer than a few cells
    inner = np.arange(B) % 2 == 0
    frac = np.where(inner, g.uniform(0.05, 0.8, B), g.uniform(1.1, 1.5, B))
    phi = g.uniform(0, 2 * np.pi, B)
    bx, by = frac * theta_E * np.cos(phi), frac * theta_E * np.sin(phi)
    packed = _rows(sim, np.stack([theta_E, cx, cy], 1))
    f32 = lambda a: torch.tensor(a.astype(np.float32), device=sim.device)
    src_x, src_y = f32(cx + bx), f32(cy + by)
    window = (-4.0, 4.0, -4.0, 4.0)
    x, y, mu, n = sim.image_positions(packed, src_x, src_y, window=window, num_cells=256, strict=True)
    assert x.shape == (B, 1, 8) and n.shape == (B, 1)
    x, y, mu, n = (t[:, 0].cpu().numpy().astype(np.float64) for t in (x, y, mu, n))
    # closed form from the float32 inputs the kernel saw
    te, cx, cy = (packed[:, k].double().cpu().numpy() for k in range(3))
    rx, ry = src_x.double().cpu().numpy() - cx, src_y.double().cpu().numpy() - cy
    r = np.hypot(rx, ry)
    for b in range(B):
        want = [(1.0, +1.0)] + ([(-1.0, -1.0)] if r[b] < te[b] else [])
        assert n[b] == len(want), (b, n[b], r[b], te[b])
        exp = []
        for sgn, _ in want:  # theta = beta + sgn theta_E beta_hat
            t = r[b] + sgn * te[b]
            exp.append((cx[b] + t * rx[b] / r[b], cy[b] + t * ry[b] / r[b], 1.0 / (1.0 - te[b] / abs(t))))
        exp = np.array(sorted(exp))
        got = np.stack([x[b, :len(want)], y[b, :len(want)], mu[b, :len(want)]], 1)
        assert np.max(np.hypot(got[:, 0] - exp[:, 0], got[:, 1] - exp[:, 1])) <= 2e-5, (b, got, exp)
        np.testing.assert_allclose(got[:, 2], exp[:, 2], rtol=1e-4)
        assert np.all(np.isnan(x[b, len(want):]))


@pytest.mark.parametrize("config", ["C1", "C2"])
def test_sie_and_epl_shear_vs_f64(config):
    from gigalens_amd import workloads
    from gigalens_amd.simulator import LensSimulator
    B, S = 10, 3
    wl = workloads.make(config, num_pix=64, batch=B)
    sim = LensSimulator(wl.phys_model, wl.sim_config, bs=B)
    packed = H.sample_packed(wl, sim, seed=21)
    if config == "C2":  # gamma >= 2: a shallower profile has a demagnified central image within a cell or two of its cusp,
        packed[:, 1] = 2.0 + (packed[:, 1] - 2.0).abs()  # which the solver does not promise to resolve
    g = np.random.default_rng(5)
    theta_E = packed[:, 0].double().cpu().numpy()
    ccx, ccy = packed[:, 3 if config == "C1" else 4].cpu().numpy(), packed[:, 4 if config == "C1" else 5].cpu().numpy()
    # sources around the lens centre: small offsets (inside the astroid: quads) and larger ones (between the caustics: doubles)
    frac = np.concatenate([g.uniform(0.0, 0.08, (B, 1)), g.uniform(0.15, 0.6, (B, S - 1))], axis=1)
    phi = g.uniform(0, 2 * np.pi, (B, S))
    srcx = torch.tensor((ccx[:, None] + frac * theta_E[:, None] * np.cos(phi)).astype(np.float32), device=sim.device)
    srcy = torch.tensor((ccy[:, None] + frac * theta_E[:, None] * np.sin(phi)).astype(np.float32), device=sim.device)
    compared, counts = _check_against_f64(sim, packed, srcx, srcy, (-4.0, 4.0, -4.0, 4.0), 256)
    assert compared >= B * S // 2
    assert 4 in counts and 2 in counts, counts


def test_cluster_nfw_and_catalogue_vs_f64():
    from gigalens_amd import workloads
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    from gigalens_amd.profiles.mass.nfw import NFW
    B, S = 3, 3
    cat = workloads.galaxy_catalogue(24, half_width=3.0, seed=4)
    lenses = [NFW(), NFW(), NFW(), DPIESubhalo(lum_star=1.0, galaxy_catalogue=cat)]
    sim = _sim(lenses, 128, 0.125, B)
    g = np.random.default_rng(9)
    cols = []
    for _ in range(3):  # Rs, alpha_Rs, center_x, center_y of three halos near the middle (C4-like, more concentrated)
        cols += [g.uniform(4.0, 6.0, B), g.uniform(2.2, 2.8, B), g.uniform(-1.0, 1.0, B), g.uniform(-1.0, 1.0, B)]
    cols += [g.uniform(0.2, 0.35, B), g.uniform(0.15, 0.25, B), g.uniform(1.5, 2.5, B)]  # member scales (resolved cores)
    names = [n for p in lenses for n in p._native_params()]
    assert len(names) == len(cols), names
    packed = _rows(sim, np.stack(cols, 1))
    srcx = torch.tensor(g.uniform(-1.0, 1.0, (B, S)).astype(np.float32), device=sim.device)
    srcy = torch.tensor(g.uniform(-1.0, 1.0, (B, S)).astype(np.float32), device=sim.device)
    compared, counts = _check_against_f64(sim, packed, srcx, srcy, (-8.0, 8.0, -8.0, 8.0), 256)
    assert compared >= B * S // 2
    assert max(counts) >= 3, counts


def test_user_written_lens_matches_builtin():
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.profiles.mass.sis import SIS
    from tests.test_user_profile_compile import SIS_BODY

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    B = 16
    g = np.random.default_rng(8)
    rows = np.stack([g.uniform(0.7, 1.2, B), g.uniform(-0.2, 0.2, B), g.uniform(-0.2, 0.2, B)], 1).astype(np.float32)
    frac = np.where(np.arange(B) % 2 == 0, g.uniform(0.1, 0.7, B), g.uniform(1.2, 1.6, B))
    phi = g.uniform(0, 2 * np.pi, B)
    out = []
    for lens in (SIS(), UserSIS()):
        sim = _sim([lens], 48, 0.1, B)
        packed = _rows(sim, rows)
        sx = torch.tensor((rows[:, 1] + frac * rows[:, 0] * np.cos(phi)).astype(np.float32), device=sim.device)
        sy = torch.tensor((rows[:, 2] + frac * rows[:, 0] * np.sin(phi)).astype(np.float32), device=sim.device)
        out.append([t.cpu().numpy() for t in sim.image_positions(packed, sx, sy, window=(-4.0, 4.0, -4.0, 4.0), num_cells=256,
                                                                  strict=True)])
    (x0, y0, m0, n0), (x1, y1, m1, n1) = out
    np.testing.assert_array_equal(n0, n1)
    assert set(n0.ravel().tolist()) == {1, 2}
    np.testing.assert_allclose(x1, x0, atol=1e-5, equal_nan=True)
    np.testing.assert_allclose(y1, y0, atol=1e-5, equal_nan=True)
    np.testing.assert_allclose(m1, m0, rtol=1e-4, equal_nan=True)


def _c2_truth():
    from gigalens_amd import workloads
    from gigalens_amd.simulator import LensSimulator
    wl = workloads.make("C2", num_pix=64, batch=1)
    sim = LensSimulator(wl.phys_model, wl.sim_config, bs=1)
    truth = {"lens_mass": [dict(theta_E=1.1, gamma=2.05, e1=0.08, e2=-0.05, center_x=0.02, center_y=-0.03),
                           dict(gamma1=0.03, gamma2=-0.02)],
             "source_light": [dict(R_sersic=0.25, n_sersic=2.0, center_x=0.0, center_y=0.0, Ie=100.0)]}
    truth = {g: [{k: torch.tensor([v], device=sim.device) for k, v in d.items()} for d in lst] for g, lst in truth.items()}
    return wl, sim, truth


def test_round_trip_with_positions_likelihood():
    from gigalens_amd.model import ForwardProbModel
    wl, sim, truth = _c2_truth()
    packed = sim.pack(truth)
    # two families: a quad (source near the centre) and a double
    x, y, mu, n = sim.image_positions(packed, torch.tensor([[0.03, 0.45]], device=sim.device),
                                      torch.tensor([[-0.02, -0.3]], device=sim.device), strict=True)
    n = n[0].tolist()
    assert n == [4, 2], n
    fx = [x[0, f, :n[f]].cpu().numpy() for f in range(2)]
    fy = [y[0, f, :n[f]].cpu().numpy() for f in range(2)]
    ones = [np.ones_like(v) for v in fx]
    pm = ForwardProbModel(wl.prior, include_pixels=False, centroids_x=fx, centroids_y=fy, centroids_errors_x=ones,
                          centroids_errors_y=ones)
    rep = pm.image_plane_rms(sim, truth)
    assert rep["rms"].shape == (1, 2)
    assert bool(rep["counts_match"].all()), rep
    assert float(rep["rms"].max()) <= 1e-4, rep
    _, red_chi2 = pm.stats_positions(sim, truth)
    assert float(red_chi2[0]) * pm.n_position <= 1e-6
    fams = pm.predicted_positions(sim, truth)
    assert [int(f[3][0]) for f in fams] == [4, 2]
    # a perturbed sample predicts the observed images less well
    pert = {g: [dict(d) for d in lst] for g, lst in truth.items()}
    pert["lens_mass"][0]["theta_E"] = pert["lens_mass"][0]["theta_E"] * 1.01
    rep2 = pm.image_plane_rms(sim, pert)
    assert float(rep2["rms"][0].max()) > float(rep["rms"][0].max())
    assert torch.isfinite(rep2["rms"]).all()


def test_deterministic_and_batch_independent():
    from gigalens_amd import workloads
    from gigalens_amd.simulator import LensSimulator
    wl = workloads.make("C2", num_pix=64, batch=64)
    sim = LensSimulator(wl.phys_model, wl.sim_config, bs=64)
    packed = H.sample_packed(wl, sim, seed=31)
    g = torch.Generator().manual_seed(2)
    sx = (0.5 * torch.rand(64, 4, generator=g) - 0.25).to(sim.device)
    sy = (0.5 * torch.rand(64, 4, generator=g) - 0.25).to(sim.device)
    bits = lambda ts: [t.contiguous().view(torch.int32) for t in ts]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = bits(sim.image_positions(packed, sx, sy))
        b = bits(sim.image_positions(packed, sx, sy))
        rows = torch.tensor([5, 17, 40], device=sim.device)
        c = bits(sim.image_positions(packed[rows].contiguous(), sx[rows], sy[rows]))
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v)
        assert torch.equal(u[rows], w)
    assert int(a[3].view(torch.int32).max()) >= 4  # quads among them


def test_refusals_and_reporting():
    from gigalens_amd import _native, workloads
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import LensSimulator
    # series-expansion lens: typed refusal
    wl = workloads.make("C6S", num_pix=32, batch=2, n_galaxies=8, n_sources=1)
    sim_s = LensSimulator(wl.phys_model, wl.sim_config, bs=2)
    with pytest.raises(_native.NativeLibraryError, match="series"):
        sim_s.image_positions(H.sample_packed(wl, sim_s, seed=1), 0.1, 0.1)
    # a quad with room for one image: reported, never silently truncated
    _, sim, truth = _c2_truth()
    packed = sim.pack(truth)
    with pytest.warns(RuntimeWarning, match="not returned"):
        x, y, mu, n = sim.image_positions(packed, 0.03, -0.02, max_images=1)
    assert int(n[0, 0]) == 1 and x.shape == (1, 1, 1)
    with pytest.raises(RuntimeError, match="not returned"):
        sim.image_positions(packed, 0.03, -0.02, max_images=1, strict=True)
    # a source far outside the caustics has one image
    x, y, mu, n = sim.image_positions(packed, 1.2, -0.9, window=(-4.0, 4.0, -4.0, 4.0), strict=True)
    assert int(n[0, 0]) == 1 and float(mu[0, 0, 0]) > 0
    # argument errors
    for kw in (dict(max_images=0), dict(num_cells=0), dict(window=(1.0, 1.0, -1.0, 1.0)), dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(_native.NativeLibraryError):
            sim.image_positions(packed, 0.05, 0.03, **kw)
    # a singular lens centre exactly on a grid vertex: flagged, no crash, no NaN image
    sim2 = _sim([SIS()], 40, 0.1, 1)
    p2 = _rows(sim2, np.array([[1.0, 0.0, 0.0]]))
    x, y, mu, n = sim2.image_positions(p2, 0.3, 0.1, window=(-2.0, 2.0, -2.0, 2.0), num_cells=64, strict=True)
    k = int(n[0, 0])
    assert k == 2
    assert torch.isfinite(x[0, 0, :k]).all() and torch.isfinite(y[0, 0, :k]).all() and torch.isfinite(mu[0, 0, :k]).all()
