"""GPU parity tests: the HIP path, called through the product API (ctypes -> C ABI), against the oracle.

Tolerances (fp32 kernels vs the float64 restatement of the reference, BASELINE.json north_star):
  * image pixels        rtol 2e-5 of the image maximum
  * chi^2 / log-like    rtol 1e-5
  * parameter gradients: every element within GRAD_RTOL_COL of the scale of its own parameter COLUMN (max over the batch of
    the oracle's |d/d theta_k|) at the reduced sizes, GRAD_RTOL_COL_FULL at the full BASELINE sizes.  Measured worst cases
    (tools/dev/grad_accuracy_scan.py, profiles/README.md): 2.2e-4 over the reduced cases; full size C2 6e-5, C3 1.4e-4,
    C3D 9e-4, C4 1e-3 -- where the reference's own algorithm evaluated in float32 (the oracle at dtype float32) sits at
    2e-4, 1e-4, 2.5e-4 and 1.5 (sic: NFW scale-radius columns) of the same scale.  Round 2 held gradients to 2e-3 of the
    ROW maximum, which let a small column be wrong by its own size.
"""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

IMG_RTOL = 2e-5
LL_RTOL = 1e-5
GRAD_RTOL = 2e-3          # per element, relative to max(|g|, 1e-2 column scale): the dPIE / extra-profile suites
GRAD_RTOL_COL = 3e-4      # per element, relative to its column's scale: reduced-size cases
GRAD_RTOL_COL_FULL = 7e-4  # the same at the full BASELINE sizes (65 536-term sums with cancellation); elements beyond it must lie
                           # within 4 x the float32 conditioning bound of the oracle's own gradient (helpers.grad_gate)


@pytest.fixture(scope="module")
def gl():
    import __graft_entry__ as ge
    from gigalens_amd import _native
    if not __import__("os").path.exists(_native.lib_path()):
        ge.build()
    _native.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gigalens_amd import workloads
    from gigalens_amd.model import ForwardProbModel
    from gigalens_amd.simulator import LensSimulator

    class NS:
        pass
    ns = NS()
    ns.workloads, ns.ForwardProbModel, ns.LensSimulator = workloads, ForwardProbModel, LensSimulator
    return ns


# ---------------------------------------------------------------------------------------------------
# plugin level: the reference's own test recipes (tests/test_profiles.py), through MassProfile.deriv /
# LightProfile.light on the GPU, against the published closed forms and the oracle
# ---------------------------------------------------------------------------------------------------
def _pts(n, seed=0):
    r = np.random.default_rng(seed)
    return r.normal(size=n).astype(np.float32), r.normal(size=n).astype(np.float32)


def test_sersic_ellipse_known_answer(gl):
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from oracle import ref_torch as ref
    se = SersicEllipse(use_lstsq=False)
    lp = dict(R_sersic=1.0, n_sersic=2.0, center_x=0.0, center_y=0.0, e1=0.0, e2=0.0, Ie=5.0)
    a = se.light(x=0.0, y=1.0, **lp)
    assert math.isclose(float(a), 5.0, rel_tol=1e-6)  # tests/test_profiles.py:25-26
    x, y = _pts(1000)
    a = se.light(x=x, y=y, **lp).cpu().numpy()
    b = ref.sersic_light(torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64),
                         1.0, 2.0, 0.0, 0.0, 5.0, 0.0, 0.0).numpy()
    assert np.allclose(a, b, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kw", [dict(theta_E=1.0, gamma=2.0, e1=0.0, e2=0.0, center_x=0.0, center_y=0.0),
                                dict(theta_E=1.2, gamma=2.2, e1=-0.1, e2=0.1, center_x=0.0, center_y=0.0)])
def test_epl_recipe(gl, kw):
    from gigalens_amd.profiles.mass.epl import EPL
    from oracle import published as pub
    x, y = _pts(10000)
    fx, fy = EPL(100).deriv(x=x, y=y, **kw)
    px, py = pub.epl_deriv_2f1(x, y, kw["theta_E"], kw["gamma"], kw["e1"], kw["e2"])
    assert np.allclose(fx.cpu().numpy(), px, rtol=1e-5, atol=1e-4)  # tests/test_profiles.py:57-58
    assert np.allclose(fy.cpu().numpy(), py, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("kw", [dict(theta_E=1.0, center_x=0.0, center_y=0.0, e1=1e-3, e2=1e-3),
                                dict(theta_E=1.2, center_x=0.0, center_y=0.0, e1=0.1, e2=-0.1)])
def test_sie_recipe(gl, kw):
    from gigalens_amd.profiles.mass.sie import SIE
    from oracle import published as pub
    x, y = _pts(10000, 1)
    fx, fy = SIE().deriv(x=x, y=y, **kw)
    px, py = pub.epl_deriv_2f1(x, y, kw["theta_E"], 2.0, kw["e1"], kw["e2"])
    assert np.allclose(fx.cpu().numpy(), px, rtol=1e-5, atol=1e-4)
    assert np.allclose(fy.cpu().numpy(), py, rtol=1e-5, atol=1e-4)


def test_sis_shear_nfw_recipes(gl):
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    from oracle import published as pub
    from oracle import ref_torch as ref
    x, y = _pts(10000, 2)
    for te in (1.0, 1.2):
        fx, fy = SIS().deriv(x=x, y=y, theta_E=te, center_x=0.0, center_y=0.0)
        px, py = pub.sis_deriv(x, y, te)
        assert np.allclose(fx.cpu().numpy(), px, rtol=1e-5, atol=1e-6) and np.allclose(fy.cpu().numpy(), py, rtol=1e-5, atol=1e-6)
    for g1, g2 in ((0.0, 0.0), (0.1, 0.1)):
        fx, fy = Shear().deriv(x=x, y=y, gamma1=g1, gamma2=g2)
        px, py = pub.shear_deriv(x, y, g1, g2)
        assert np.allclose(fx.cpu().numpy(), px, atol=1e-6) and np.allclose(fy.cpu().numpy(), py, atol=1e-6)
    fx, fy = NFW().deriv(x=x * 3, y=y * 3, Rs=1.7, alpha_Rs=0.9, center_x=0.1, center_y=-0.2)
    ox, oy = ref.nfw_deriv(torch.as_tensor(x * 3, dtype=torch.float64), torch.as_tensor(y * 3, dtype=torch.float64),
                           1.7, 0.9, 0.1, -0.2)
    assert np.allclose(fx.cpu().numpy(), ox.numpy(), rtol=2e-5, atol=2e-6)
    assert np.allclose(fy.cpu().numpy(), oy.numpy(), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("n_max", [5, 14])  # 14: above the register-resident orders, the runtime-order point kernels
@pytest.mark.parametrize("interpolate", [True, False])
def test_shapelets_recipe(gl, interpolate, n_max):
    from gigalens_amd.profiles.light.shapelets import Shapelets
    from oracle import published as pub
    shp = Shapelets(n_max=n_max, use_lstsq=False, interpolate=interpolate)
    r = np.random.default_rng(3)
    amplitudes = r.normal(size=(shp.n_layers, 1)).astype(np.float32)
    amp = {n: a for n, a in zip(shp._amp_names, amplitudes)}
    x, y = r.normal(size=(5, 5, 1)).astype(np.float32), r.normal(size=(5, 5, 1)).astype(np.float32)
    a = shp.light(x=x, y=y, center_x=0, center_y=0, beta=1, **amp).cpu().numpy()
    b = pub.shapelet_set(x.ravel(), y.ravel(), amplitudes.ravel().astype(np.float64), n_max, 1.0)
    assert a.shape == (5, 5, 1)
    assert np.allclose(a.ravel(), b, rtol=1e-5, atol=1e-4)  # tests/test_profiles.py:47


# ---------------------------------------------------------------------------------------------------
# simulator + likelihood level vs the oracle at sizes the oracle finishes in seconds
# ---------------------------------------------------------------------------------------------------
CASES = [
    ("C1", dict(num_pix=64, batch=1)),
    ("C1", dict(num_pix=24, batch=5)),
    ("C2", dict(num_pix=32, batch=8)),
    ("C2", dict(num_pix=47, batch=3)),   # ragged: 2209 pixels, not a multiple of the tile
    ("C3", dict(num_pix=32, batch=4, interpolate=False)),
    ("C3", dict(num_pix=32, batch=4, interpolate=True)),
    ("C3", dict(num_pix=20, batch=3, interpolate=True, n_max=4)),
    ("C4", dict(num_pix=40, batch=4, n_halos=3, n_sources=4)),
    ("C4", dict(num_pix=32, batch=2)),
    ("C3D", dict(num_pix=30, batch=3, interpolate=True, n_max=8)),   # shapelets-demo.ipynb model
    ("C3D", dict(num_pix=30, batch=3, interpolate=False, n_max=5)),
    ("C3", dict(num_pix=24, batch=3, interpolate=True, n_max=12)),    # above n_max = 10: the runtime-order interpreter variant
    ("C3", dict(num_pix=20, batch=2, interpolate=False, n_max=16)),
    ("C3D", dict(num_pix=22, batch=2, interpolate=True, n_max=20)),   # 231 amplitudes beside a lens light
]


@pytest.mark.parametrize("name,kw", CASES)
def test_simulate_loglike_grad_vs_oracle(gl, name, kw):
    wl = gl.workloads.make(name, **kw)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=11)
    obs_np = obs.cpu().numpy()
    err_np = None if err is None else err.cpu().numpy()
    ll_o, red_o, g_o, img_o = H.oracle_loglike_and_grad(wl, packed.cpu().double(), obs_np, err_np, wl.batch)

    img = sim.simulate(packed).cpu().numpy().reshape(img_o.shape)
    assert np.abs(img - img_o).max() <= IMG_RTOL * np.abs(img_o).max() + 1e-7

    pm = gl.ForwardProbModel(wl.prior, obs_np, wl.background_rms, wl.exp_time, error_map=err_np, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, red = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    assert np.allclose(ll.detach().cpu().numpy(), ll_o, rtol=LL_RTOL)
    assert np.allclose(red.detach().cpu().numpy(), red_o, rtol=LL_RTOL)
    g = p.grad.cpu().numpy()
    # every element against the scale of its own parameter column (H.grad_col_err)
    bad = H.grad_col_err(g, g_o) > GRAD_RTOL_COL
    assert not bad.any(), (np.argwhere(bad)[:5], g[bad][:5], g_o[bad][:5], H.grad_col_err(g, g_o).max())

    # forward-only entry (grad_params == NULL, a different kernel instantiation) agrees to rounding
    ll2, _ = pm._pixel_stats_packed(sim, packed)
    assert torch.allclose(ll2, ll.detach(), rtol=LL_RTOL)

    # image-boundary pair (gl_simulate_fwd / gl_simulate_bwd): same gradient through the materialised image
    p2 = packed.clone().requires_grad_(True)
    im = sim.simulate(p2).reshape(wl.batch, wl.sim_config.num_pix, wl.sim_config.num_pix)
    if err is None:
        sig2 = wl.background_rms ** 2 + im / wl.exp_time
    else:
        sig2 = (err ** 2).expand_as(im)
    ll3 = -0.5 * (((im - obs) ** 2 / sig2).sum((-2, -1)) + torch.log(2 * math.pi * sig2).sum((-2, -1)))
    ll3.sum().backward()
    g3 = p2.grad.cpu().numpy()
    bad = H.grad_col_err(g3, g_o) > GRAD_RTOL_COL
    assert not bad.any(), (np.argwhere(bad)[:5], g3[bad][:5], g_o[bad][:5], H.grad_col_err(g3, g_o).max())
    assert np.allclose(ll3.detach().cpu().numpy(), ll_o, rtol=5e-5)


def test_log_prob_layout_and_prior(gl):
    """z column k == k-th leaf in tf.nest.flatten order; log_prob = log_like + prior + log|J| (tf/model.py:148-167)."""
    wl = gl.workloads.make("C2", num_pix=24, batch=6)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    x = wl.prior.sample(wl.batch, seed=3)
    z = pm.bij.inverse(x)
    assert z.shape == (wl.batch, 13)
    # App. B of SURVEY.md: center_x center_y e1 e2 gamma theta_E | gamma1 gamma2 | Ie R_sersic center_x center_y n_sersic
    assert torch.allclose(z[:, 5].cpu(), torch.log(x["lens_mass"][0]["theta_E"]).cpu(), atol=1e-6)
    assert torch.allclose(z[:, 6].cpu(), x["lens_mass"][1]["gamma1"].cpu())
    assert torch.allclose(z[:, 8].cpu(), torch.log(x["source_light"][0]["Ie"]).cpu(), atol=1e-6)
    back = pm.bij.forward(z)
    for a, b in zip(__import__("gigalens_amd.prior", fromlist=["x"]).nest_flatten(back),
                    __import__("gigalens_amd.prior", fromlist=["x"]).nest_flatten(x)):
        assert torch.allclose(a.cpu(), b.cpu(), rtol=2e-5, atol=1e-6)
    z = z.to("cuda").requires_grad_(True)
    lp, red = pm.log_prob(sim, z)
    ll = pm.log_like(sim, z.detach())
    lpr = pm.log_prior(z.detach())
    assert torch.allclose(lp.detach(), ll + lpr, rtol=LL_RTOL, atol=1e-3)
    ll_s, red_s = pm.stats_pixels(sim, x)
    # stats_pixels takes x itself, log_prob takes forward(inverse(x)): equal up to the fp32 bijector round trip
    assert torch.allclose(ll_s, ll, rtol=1e-4) and torch.allclose(red_s, red.detach(), rtol=1e-4)
    lp.sum().backward()
    assert torch.isfinite(z.grad).all() and (z.grad.abs().sum(0) > 0).all()
    # finite-difference check of d log_prob / dz through bijector + kernels (float32: loose)
    k, eps = 5, 1e-3
    zp, zm = z.detach().clone(), z.detach().clone()
    zp[:, k] += eps
    zm[:, k] -= eps
    fd = (pm.log_prob(sim, zp)[0] - pm.log_prob(sim, zm)[0]) / (2 * eps)
    assert torch.allclose(fd, z.grad[:, k], rtol=5e-2, atol=5e-2 * float(z.grad[:, k].abs().max()))


@pytest.mark.parametrize("name,kw", [("C2", dict(num_pix=40, batch=33)), ("C4", dict(num_pix=32, batch=5, n_halos=2, n_sources=3)),
                                     ("C3", dict(num_pix=24, batch=6, interpolate=False, n_max=6))])
def test_fused_log_prob_matches_unfused(gl, name, kw):
    """gl_logprob_fwd_bwd (bijector + prior inside the native launch sequence) == torch bijector/prior around
    gl_loglike_fwd_bwd, value and gradient w.r.t. z."""
    wl = gl.workloads.make(name, **kw)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time,
                             error_map=None if err is None else err.cpu().numpy(), include_positions=False)
    z0 = pm.bij.inverse(wl.prior.sample(wl.batch, seed=21)).to("cuda")
    za, zb = z0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
    lpa, reda = pm.log_prob(sim, za)
    lpb, redb = pm.log_prob_unfused(sim, zb)
    lpa.sum().backward()
    lpb.sum().backward()
    assert torch.allclose(lpa, lpb, rtol=2e-6, atol=1e-3)
    assert torch.allclose(reda, redb, rtol=2e-6)
    scale = zb.grad.abs().max(dim=1, keepdim=True).values
    assert ((za.grad - zb.grad).abs() <= 2e-4 * scale + 1e-4).all(), ((za.grad - zb.grad).abs() / scale).max()
    lp_nograd, _ = pm.log_prob(sim, z0)  # forward-only entry
    assert torch.allclose(lp_nograd, lpa.detach(), rtol=LL_RTOL, atol=1e-3)
    lp2, red2, g2 = pm.log_prob_and_grad(sim, z0)  # no autograd graph: bitwise the same numbers
    assert torch.equal(lp2, lpa.detach()) and torch.equal(red2, reda.detach()) and torch.equal(g2, za.grad)


@pytest.mark.parametrize("lens", ["SIE", "EPL"])  # thread-per-component front end (gl_prep_kernel) / wavefront-per-sample (gl_prep_wave_kernel)
def test_front_end_from_z_equals_front_end_from_packed_rows(gl, lens):
    """One front-end kernel takes `z` or the packed rows.  Under a prior of Normal columns every bijector is the identity, so the
    packed rows ARE z, bit for bit: gl_logprob_fwd_bwd and gl_loglike_fwd_bwd then run the same main kernel in the same mode on
    derived rows that must be the same bits, and nothing may round differently -- loglike and chi2 are compared bitwise.
    B = 45 samples of three components: 135 threads cross the 128-thread workgroup of gl_prep_kernel, and the last workgroup
    of gl_prep_wave_kernel (four samples each) is partly empty."""
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    J, S, N = tfd.JointDistributionNamed, tfd.JointDistributionSequential, tfd.Normal
    main = dict(theta_E=N(0.4, 0.02), e1=N(0.1, 0.02), e2=N(-0.05, 0.02), center_x=N(0, 0.02), center_y=N(0, 0.02))
    if lens == "EPL":
        main["gamma"] = N(2.0, 0.05)
    prior = J(dict(lens_mass=S([J(main), J(dict(gamma1=N(0, 0.02), gamma2=N(0, 0.02)))]),
                   source_light=S([J(dict(R_sersic=N(0.25, 0.01), n_sersic=N(2.0, 0.1), center_x=N(0, 0.03), center_y=N(0, 0.03),
                                          Ie=N(50.0, 2.0)))])))
    phys = PhysicalModel([EPL() if lens == "EPL" else SIE(), Shear()], [], [Sersic()])
    B = 45
    wl = gl.workloads.Workload("PREP", phys, prior, SimulatorConfig(delta_pix=0.07, num_pix=16), B)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(phys, wl.sim_config, bs=B)
    pm = gl.ForwardProbModel(prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    z = pm.bij.inverse(prior.sample(B, seed=5)).to("cuda").contiguous()
    packed = sim.pack(pm.bij.forward(z)).contiguous()
    assert sorted(packed[7].tolist()) == sorted(z[7].tolist())  # identity bijectors: the same numbers in the packed order
    model = pm._bind_prior(sim)
    args = (pm.observed_image, pm.error_map, pm._mask(sim), wl.background_rms, wl.exp_time, True)
    _, ll_z, chi2_z, grad_z = model.logprob(z, *args)
    ll_p, chi2_p, grad_p = model.loglike(packed, *args)
    assert torch.isfinite(ll_z).all() and torch.isfinite(grad_z).all() and torch.isfinite(grad_p).all()
    assert torch.equal(ll_z, ll_p) and torch.equal(chi2_z, chi2_p)


@pytest.mark.parametrize("name,kw", [("C1", dict(num_pix=40, batch=9)), ("C2", dict(num_pix=50, batch=17)),
                                     ("C3", dict(num_pix=32, batch=5, interpolate=False)),
                                     ("C3", dict(num_pix=32, batch=5, interpolate=True, n_max=7)),
                                     ("C3D", dict(num_pix=28, batch=4, interpolate=True, n_max=8)), ("DEMO", dict())])
@pytest.mark.parametrize("tile", ["1", "2", "4", "pair"])
def test_specialised_kernels_match_interpreter(gl, name, kw, tile, monkeypatch):
    """The compile-time-specialised kernels (gl_static.hip.h) and the generic interpreter kernel evaluate the
    same maths: image, log-likelihood and gradient agree to rounding for every supported composition."""
    if name == "DEMO":  # the reference's default model (tests/conftest.py:76-80): EPL+Shear / SersicEllipse / SersicEllipse
        from gigalens_amd.model import PhysicalModel
        from gigalens_amd.profiles.light.sersic import SersicEllipse
        from gigalens_amd.profiles.mass.epl import EPL
        from gigalens_amd.profiles.mass.shear import Shear
        from gigalens_amd.simulator import SimulatorConfig
        from tests.test_prior_host import default_prior
        wl = gl.workloads.Workload("DEMO", PhysicalModel([EPL(), Shear()], [SersicEllipse()], [SersicEllipse()]),
                                   default_prior(), SimulatorConfig(delta_pix=0.065, num_pix=44), 7)
    else:
        wl = gl.workloads.make(name, **kw)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    res = {}
    for static in ("1", "0"):
        monkeypatch.setenv("GIGALENS_HIP_STATIC", static)
        monkeypatch.setenv("GIGALENS_HIP_PAIR", "1" if tile == "pair" else "0")  # pixel-pair (packed fp32) kernels
        monkeypatch.setenv("GIGALENS_HIP_TILE", "2" if tile == "pair" else tile)
        sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
        packed = H.sample_packed(wl, sim, seed=13)
        pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time,
                                 error_map=None if err is None else err.cpu().numpy(), include_positions=False)
        p = packed.clone().requires_grad_(True)
        ll, red = pm._pixel_stats_packed(sim, p)
        ll.sum().backward()
        p2 = packed.clone().requires_grad_(True)
        img = sim.simulate(p2)
        (img * obs).sum().backward()
        res[static] = (ll.detach(), p.grad.clone(), img.detach(), p2.grad.clone(), pm._pixel_stats_packed(sim, packed)[0])
    a, b = res["1"], res["0"]
    assert torch.allclose(a[0], b[0], rtol=LL_RTOL) and torch.allclose(a[4], b[4], rtol=LL_RTOL)
    # shapelet images are sums of +-500-amplitude terms: evaluation order moves pixels by ~1e-5 of the maximum
    assert torch.allclose(a[2], b[2], rtol=1e-5, atol=IMG_RTOL * float(b[2].abs().max()))
    for ga, gb in ((a[1], b[1]), (a[3], b[3])):
        scale = gb.abs().max(dim=1, keepdim=True).values
        assert ((ga - gb).abs() <= 3e-4 * scale + 1e-6).all(), ((ga - gb).abs() / scale).max()


def test_pix_region_and_constants(gl):
    """pix_region masks pixels out of the render and the likelihood (tf/simulator.py:34-44, tf/model.py:97-100);
    fixed parameters arrive through *_constants (model.py:29-44)."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    from oracle import ref_torch as ref
    n = 28
    yy, xx = np.mgrid[:n, :n]
    mask = (((xx - 13.5) ** 2 + (yy - 13.5) ** 2) < 11 ** 2).astype(np.float32)
    phys = PhysicalModel([EPL(), Shear()], [SersicEllipse()], [SersicEllipse()],
                         lenses_constants=[{"center_x": 0.01, "center_y": -0.02}, {}],
                         lens_light_constants=[{"n_sersic": 3.0}], source_light_constants=[{}])
    cfg = SimulatorConfig(delta_pix=0.08, num_pix=n, pix_region=mask)
    B = 4
    sim = gl.LensSimulator(phys, cfg, bs=B)
    r = np.random.default_rng(0)
    f = lambda lo, hi: torch.tensor(r.uniform(lo, hi, size=B).astype(np.float32))
    params = {
        "lens_mass": [dict(theta_E=f(0.8, 1.2), gamma=f(1.8, 2.3), e1=f(-0.2, 0.2), e2=f(-0.2, 0.2)),
                      dict(gamma1=f(-0.05, 0.05), gamma2=f(-0.05, 0.05))],
        "lens_light": [dict(R_sersic=f(0.5, 1.0), e1=f(-0.1, 0.1), e2=f(-0.1, 0.1), center_x=f(-0.05, 0.05),
                            center_y=f(-0.05, 0.05), Ie=f(10, 30))],
        "source_light": [dict(R_sersic=f(0.1, 0.3), n_sersic=f(1, 3), e1=f(-0.3, 0.3), e2=f(-0.3, 0.3),
                              center_x=f(-0.2, 0.2), center_y=f(-0.2, 0.2), Ie=f(50, 150))],
    }
    img = sim.simulate(params).cpu().numpy()
    rs = ref.RefSimulator(phys, cfg, B, dtype=torch.float64)
    img_o = rs.simulate({k: [{n: v.double() for n, v in d.items()} for d in lst] for k, lst in params.items()}).numpy()
    assert np.abs(img - img_o).max() <= IMG_RTOL * np.abs(img_o).max()
    assert np.all(img[:, mask == 0] == 0)
    obs = img_o[0] + 0.05 * r.normal(size=(n, n))
    pm = gl.ForwardProbModel(_dummy_prior(), obs, 0.2, 100.0, include_positions=False)
    ll, red = pm.stats_pixels(sim, params)
    ll_o, red_o = ref.stats_pixels(rs, {k: [{n: v.double() for n, v in d.items()} for d in lst] for k, lst in params.items()},
                                   obs, 0.2, 100.0)
    assert np.allclose(ll.cpu().numpy(), ll_o.numpy(), rtol=LL_RTOL)
    assert np.allclose(red.cpu().numpy(), red_o.numpy(), rtol=LL_RTOL)


def _dummy_prior():
    from gigalens_amd import prior as tfd
    return tfd.JointDistributionNamed(dict(lens_mass=tfd.JointDistributionSequential(
        [tfd.JointDistributionNamed(dict(theta_E=tfd.Normal(0, 1)))])))


def test_nan_semantics_sie_circular(gl):
    """SIE with e == 0 is 0/0 in the reference (sie.py:31-40 with s == 0): the image pixel becomes 0
    (tf/simulator.py:140) and chi^2 is computed on that zero image."""
    wl = gl.workloads.make("C1", num_pix=16, batch=2)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=2)
    packed = H.sample_packed(wl, sim, seed=1)
    packed[0, 1] = 0.0
    packed[0, 2] = 0.0  # e1 = e2 = 0 for sample 0
    img = sim.simulate(packed).cpu().numpy()
    assert np.all(img[0] == 0) and np.all(np.isfinite(img)) and img[1].max() > 0


def test_negative_variance_is_nan_in_value_and_gradient(gl):
    """sigma^2 = bg^2 + model / t below zero somewhere: the reference's sqrt makes the sample's log-likelihood NaN and, through
    the square root's derivative, every entry of its gradient row (tf/model.py:96-99); the other samples are untouched."""
    wl = gl.workloads.make("C2", num_pix=24, batch=4)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=4)
    packed[1, -1] = -packed[1, -1].abs()  # a source of negative amplitude: the model dips below -bg^2 t at its peak
    ll_o, _, g_o, _ = H.oracle_loglike_and_grad(wl, packed.cpu().double(), obs.cpu().numpy(), None, wl.batch)
    assert np.isnan(ll_o[1]) and np.isnan(g_o[1]).all() and np.isfinite(ll_o[[0, 2, 3]]).all()
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, _ = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    g = p.grad.cpu().numpy()
    assert np.array_equal(np.isnan(ll.detach().cpu().numpy()), np.isnan(ll_o))
    assert np.array_equal(np.isnan(g), np.isnan(g_o))
    keep = [0, 2, 3]
    assert np.allclose(ll.detach().cpu().numpy()[keep], ll_o[keep], rtol=LL_RTOL)
    assert H.grad_col_err(g[keep], g_o[keep]).max() <= GRAD_RTOL_COL


def test_error_conventions(gl):
    from gigalens_amd import _native
    wl = gl.workloads.make("C2", num_pix=16, batch=2)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=2)
    with pytest.raises(_native.NativeLibraryError):
        sim._model.simulate_fwd(torch.zeros((2, 5), device="cuda"))  # wrong P
    with pytest.raises(_native.NativeLibraryError):
        sim._model.simulate_fwd(torch.zeros((2, sim._model.P)))  # CPU tensor: no CPU path
    with pytest.raises(KeyError):
        sim.simulate({"lens_mass": [{}, {}], "source_light": [{}]})


# ---------------------------------------------------------------------------------------------------
# full BASELINE sizes: size-independent properties (the oracle would take minutes here)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("C2", {}), ("C4", {}), ("C5", {}), ("C3", dict(interpolate=True)), ("C3", dict(interpolate=False)),
                                     ("C4", dict(batch=64)), ("C3", dict(batch=128, interpolate=False))])
def test_full_size_properties(gl, name, kw):
    """Every BASELINE config at its FULL size and in its default mode (C2 128^2 x 1024; C3 table and direct shapelets
    128^2 x 1024; C4 256^2 x 512; C5's per-rank shard 256^2 x 256), plus two reduced batches."""
    wl = gl.workloads.make(name, **kw)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=5)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time,
                             error_map=None if err is None else err.cpu().numpy(), include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, red = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    # (1) fused log-likelihood == likelihood of the materialised image (independent kernels + torch reductions, f64)
    im = sim.simulate(packed).double()
    o = obs.double()
    sig2 = (wl.background_rms ** 2 + im / wl.exp_time) if err is None else (err.double() ** 2).expand_as(im)
    ll_img = -0.5 * (((im - o) ** 2 / sig2).sum((-2, -1)) + torch.log(2 * math.pi * sig2).sum((-2, -1)))
    assert torch.allclose(ll.detach().double(), ll_img, rtol=LL_RTOL)
    # (1b) the float64 oracle on the first rows at the config's FULL pixel grid (the whole batch would take minutes): the
    # reduced-size oracle cases cannot see errors that only matter on 65 536-pixel sums of large residuals
    n_o = 4
    wl_o = gl.workloads.make(name, **{**kw, "batch": n_o})
    ll_o, _, g_o, _ = H.oracle_loglike_and_grad(wl_o, packed[:n_o].double().cpu(), obs.cpu().numpy(),
                                                None if err is None else err.cpu().numpy(), n_o)
    assert np.allclose(ll.detach()[:n_o].cpu().numpy(), ll_o, rtol=LL_RTOL)
    assert np.allclose(ll_img[:n_o].cpu().numpy(), ll_o, rtol=LL_RTOL)
    # every element of the checked rows against the scale of its own parameter column, taken from the ORACLE rows (until round
    # 4: from the product's own batch-wide maximum -- an inflated product column would have loosened its own bound); elements
    # beyond the tolerance must be explained by the float32 conditioning of the oracle's own gradient (helpers.grad_gate)
    g_all = p.grad.cpu().numpy()
    err_np = None if err is None else err.cpu().numpy()
    p64c = packed[:n_o].double().cpu()
    ok, rep = H.grad_gate(g_all[:n_o], g_o, GRAD_RTOL_COL_FULL,
                          lambda S: H.float32_conditioning_bound(wl_o, p64c, obs.cpu().numpy(), err_np, n_o, g_o, S))
    print(f"{name} {kw}: gradient gate {rep}")
    assert ok, rep
    # (2) batch independence: a sub-batch gives the same rows (another batch size means another pixel chunking, i.e. another
    # fixed summation order of the fp32 partial sums: a few ulps of the 65 536-term sum)
    sim_small = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=7)
    ll_small, _ = pm._pixel_stats_packed(sim_small, packed[:7].clone())
    assert torch.allclose(ll_small, ll.detach()[:7], rtol=3e-6)
    ll_again, _ = pm._pixel_stats_packed(sim, packed)          # forward-only kernel instantiation
    assert torch.allclose(ll_again, ll.detach(), rtol=LL_RTOL)
    p_again = packed.clone().requires_grad_(True)
    ll_rep, _ = pm._pixel_stats_packed(sim, p_again)             # same instantiation twice: bitwise reproducible
    ll_rep.sum().backward()
    assert torch.equal(ll_rep.detach(), ll.detach()) and torch.equal(p_again.grad, p.grad)
    # (3) linearity of the render in the source amplitudes
    scaled = packed.clone()
    last = wl.phys_model.source_light[-1]
    if last.name.startswith("SERSIC"):
        scaled[:, -1] *= 2.0
        only = packed.clone()
        delta = (sim.simulate(scaled) - sim.simulate(packed))
        other = packed.clone()
        other[:, -1] *= 3.0
        delta2 = (sim.simulate(other) - sim.simulate(packed))
        assert torch.allclose(2 * delta, delta2, rtol=1e-4, atol=1e-5 * float(delta2.abs().max()))
    assert torch.isfinite(p.grad).all()


@pytest.mark.parametrize("name,kw,n_check", [("C2", {}, 128), ("C3", dict(interpolate=True), 48), ("C3", dict(interpolate=False), 48),
                                             ("C4", {}, 32)])
def test_full_size_loglike_many_samples_vs_oracle(gl, name, kw, n_check):
    """The fused log-likelihood of the BASELINE configs at FULL size against the float64 oracle over many samples (the
    oracle forward-only, in chunks): chi^2 / log-like within rtol 1e-5 on EVERY sample checked, not only on the reduced-size
    cases.  (Measured worst case over 256 / 128 / 128 / 64 samples: 1.1e-6, 0.9e-6, 1.2e-6, 3.3e-6 --
    tools/dev/ll_accuracy_scan.py; this scan is what exposed the NFW closed form's loss of 2e-6 in 0.6 < X < 0.95, 3.4e-5 on the
    log-likelihood of one C4 sample in 512, before the h(X) table.)"""
    wl = gl.workloads.make(name, **kw)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=5)
    err_np = None if err is None else err.cpu().numpy()
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, error_map=err_np, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, _ = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    ll_o = H.oracle_loglike_chunked(wl, packed.double().cpu(), obs.cpu().numpy(), err_np, n_check)
    rel = np.abs(ll.detach().double().cpu().numpy()[:n_check] - ll_o) / np.abs(ll_o)
    assert rel.max() <= LL_RTOL, (int(rel.argmax()), float(rel.max()))
    ll_f, _ = pm._pixel_stats_packed(sim, packed)  # forward-only instantiation
    rel_f = np.abs(ll_f.double().cpu().numpy()[:n_check] - ll_o) / np.abs(ll_o)
    assert rel_f.max() <= LL_RTOL, (int(rel_f.argmax()), float(rel_f.max()))


@pytest.mark.parametrize("n_halos,n_sources,ellipse,num_pix,batch", [(8, 20, False, 48, 5), (3, 5, False, 40, 4), (8, 20, True, 40, 3),
                                                                     (2, 7, True, 33, 2), (5, 9, False, 64, 2)])
def test_cluster_kernel_matches_interpreter(gl, n_halos, n_sources, ellipse, num_pix, batch, monkeypatch):
    """gl_cluster_kernel (forward state in registers, in-register transpose-reduction of the gradient sums, spherical fast
    path) against the interpreter kernel on the same NFW + Sersic models: log-likelihood, its gradient and the VJP of
    ``simulate`` agree to rounding -- both capacities (4 + 8 and 8 + 20), spherical and elliptical sources, ragged tiles
    (33 x 33 px), odd source counts (the spherical path packs sources in pairs)."""
    import math
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.simulator import SimulatorConfig
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    halo = lambda: J(dict(Rs=tfd.LogNormal(math.log(2.0), 0.3), alpha_Rs=tfd.LogNormal(math.log(0.5), 0.3),
                          center_x=tfd.Uniform(-1.5, 1.5), center_y=tfd.Uniform(-1.5, 1.5)))
    src = dict(R_sersic=tfd.LogNormal(math.log(0.25), 0.15), n_sersic=tfd.Uniform(0.5, 4), center_x=tfd.Uniform(-1, 1),
               center_y=tfd.Uniform(-1, 1), Ie=tfd.LogNormal(math.log(150.0), 0.5))
    if ellipse:
        src.update(e1=tfd.Normal(0, 0.15), e2=tfd.Normal(0, 0.15))
    phys = PhysicalModel([NFW() for _ in range(n_halos)], [], [(SersicEllipse if ellipse else Sersic)() for _ in range(n_sources)])
    prior = J(dict(lens_mass=S([halo() for _ in range(n_halos)]), source_light=S([J(dict(src)) for _ in range(n_sources)])))
    wl = gl.workloads.Workload("CL", phys, prior, SimulatorConfig(delta_pix=0.065, num_pix=num_pix), batch)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    res = {}
    for flag in ("2", "1", "0"):
        monkeypatch.setenv("GIGALENS_HIP_CLUSTER", flag)
        sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
        packed = H.sample_packed(wl, sim, seed=3)
        pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
        p = packed.clone().requires_grad_(True)
        ll, _ = pm._pixel_stats_packed(sim, p)
        ll.sum().backward()
        kern = sim._model.last_main_kernel()
        p2 = packed.clone().requires_grad_(True)
        (sim.simulate(p2) * obs).sum().backward()
        res[flag] = (ll.detach(), p.grad.clone(), p2.grad.clone(), kern)
    assert "gl_cluster_kernel" in res["1"][3] and "gl_clusterw_kernel" in res["2"][3] and "gl_main_kernel" in res["0"][3]
    for flag in ("1", "2"):
        # (the component-per-wave kernel adds the deflections and the source images in another order and reads the NFW function
        # from its own table: a rounding-level change of beta moves the log-likelihood of these steep, badly fitting models by a
        # few 1e-6 -- it is held to the oracle tolerance here and against the oracle itself in the tests below)
        assert torch.allclose(res[flag][0], res["0"][0], rtol=2e-6 if flag == "1" else LL_RTOL)
        for k in (1, 2):
            a, b = res[flag][k], res["0"][k]
            scale = b.abs().amax(dim=1, keepdim=True).clamp_min(1e-6 * float(b.abs().max()))
            assert float(((a - b).abs() / scale).max()) < 2e-4, (flag, k)
            assert float((a - b).abs().max()) > 0.0 or n_sources == 0  # two different kernels ran


@pytest.mark.parametrize("case", ["psf", "c2"])
def test_gradient_error_distribution_vs_float32_reference(gl, case):
    """Is the HIP gradient systematically further from the float64 truth than the reference's OWN algorithm evaluated in float32
    (the oracle at dtype float32, torch.autograd through the restated TF graph)?  A single ill-conditioned row cannot tell (see
    helpers.float32_conditioning_bound); 128 samples can: per row e = max over columns of |g - g_f64| / column scale, and the
    quantiles of the two error distributions are compared.  Measured over 256 samples (tools/dev/grad_error_distribution.py,
    profiles/r4_grad_error_distribution.jsonl): ratio HIP / float32-reference of p50 0.52 / 0.70, p90 0.86 / 1.40, max
    0.83 / 1.18 (PSF geometry / C2 model); the cluster model: 6e-4 (the float32 reference's NFW closed form cancels).
    Ref: src/gigalens/tf/model.py:89-101, tf/inference.py:33-39."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    from oracle import ref_torch as ref
    from tests.test_prior_host import default_prior
    n = 128
    if case == "psf":
        phys, prior = PhysicalModel([EPL(), Shear()], [SersicEllipse()], [SersicEllipse()]), default_prior()
        cfg, psf = SimulatorConfig(delta_pix=0.08, num_pix=60, supersample=1), _gauss_psf(13, 1.2)
    else:
        w2 = gl.workloads.make("C2", num_pix=64, batch=n)
        phys, prior, cfg, psf = w2.phys_model, w2.prior, w2.sim_config, None
    wl = gl.workloads.Workload("DIST", phys, prior, cfg, n)
    sim = gl.LensSimulator(phys, cfg, bs=n, supersampled_kernel=psf)
    packed = H.sample_packed(wl, sim, seed=4)
    rs1 = ref.RefSimulator(phys, cfg, 1, dtype=torch.float64, supersampled_kernel=psf)
    img0 = rs1.simulate(H.struct_from_packed(phys, packed[:1].cpu().double())).detach().numpy().reshape(cfg.num_pix, cfg.num_pix)
    obs = (img0 + 0.3 * np.random.default_rng(1).normal(size=img0.shape)).astype(np.float32)
    pm = gl.ForwardProbModel(prior, obs, 0.2, 100.0, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, _ = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    g = p.grad.double().cpu().numpy()

    def oracle(dt):
        out = []
        for i0 in range(0, n, 32):
            q = packed[i0:i0 + 32].cpu().to(dt).requires_grad_(True)
            rs = ref.RefSimulator(phys, cfg, q.shape[0], dtype=dt, supersampled_kernel=psf)
            l, _ = ref.stats_pixels(rs, H.struct_from_packed(phys, q), obs, 0.2, 100.0)
            out.append(torch.autograd.grad(l.sum(), q)[0].double().numpy())
        return np.concatenate(out)
    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    ok = np.isfinite(g64).all(axis=1) & np.isfinite(g32).all(axis=1)
    assert ok.sum() >= n - 4 and np.isfinite(g[ok]).all()
    S = np.abs(g64[ok]).max(axis=0, keepdims=True)
    e_h, e_3 = (np.abs(g[ok] - g64[ok]) / S).max(axis=1), (np.abs(g32[ok] - g64[ok]) / S).max(axis=1)
    q = lambda a, f: float(np.quantile(a, f))
    rep = dict(hip=(q(e_h, .5), q(e_h, .9), float(e_h.max())), f32_reference=(q(e_3, .5), q(e_3, .9), float(e_3.max())))
    assert q(e_h, 0.5) <= 1.5 * q(e_3, 0.5) and q(e_h, 0.9) <= 2.0 * q(e_3, 0.9) and e_h.max() <= 4.0 * e_3.max(), rep
    assert q(e_h, 0.5) <= 2e-6, rep


@pytest.mark.parametrize("cluster", ["2", "1", "0"])
def test_nfw_table_ranges_vs_oracle(gl, cluster, monkeypatch):
    """The main kernels read h(X) = g(X)/X^2 of the NFW deflection (nfw.py:26-52) from an LDS table on [2^-6, 2^6) and take
    the closed form outside it and at X == 1 (gl_vec.hip.h::nfw_h_pair).  Halos whose scale radius puts the image's pixels
    below the table (Rs = 40: X down to 3e-4), above it (Rs = 0.01: X up to 300), across X = 1 (Rs = 1) and with a pixel 1e-5
    from the halo centre against the float64 oracle: image, log-likelihood, gradient -- through the cluster kernel and
    through the interpreter.  (The g(1) = 1 point itself: tests/test_hostmath_vjp.py::test_nfw_through_x_equal_one.)"""
    import math
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.nfw import NFW
    from gigalens_amd.simulator import SimulatorConfig
    monkeypatch.setenv("GIGALENS_HIP_CLUSTER", cluster)
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    phys = PhysicalModel([NFW()], [], [Sersic()])
    prior = J(dict(lens_mass=S([J(dict(Rs=tfd.LogNormal(0.0, 1.0), alpha_Rs=tfd.LogNormal(0.0, 0.3), center_x=tfd.Normal(0, 1),
                                       center_y=tfd.Normal(0, 1)))]),
                   source_light=S([J(dict(R_sersic=tfd.LogNormal(math.log(0.3), 0.1), n_sersic=tfd.Uniform(1, 3),
                                          center_x=tfd.Normal(0, 0.1), center_y=tfd.Normal(0, 0.1), Ie=tfd.LogNormal(math.log(100.0), 0.3)))])))
    cfg = SimulatorConfig(delta_pix=0.065, num_pix=48)
    rows = [  # Rs, alpha_Rs, cx, cy | R_sersic, n, cx, cy, Ie
        [40.0, 30.0, 0.03, -0.01, 0.3, 1.5, 0.05, 0.02, 100.0],
        [0.01, 0.02, 0.4, 0.3, 0.3, 2.0, 0.05, 0.02, 100.0],
        [1.0, 1.0, 0.2, -0.1, 0.25, 1.0, -0.05, 0.1, 120.0],
        [0.13, 0.5, 0.03249, 0.03251, 0.3, 2.5, 0.0, 0.0, 80.0],   # centre 1e-5 off a pixel (exactly ON it the reference's gradient is NaN: d sqrt at 0)
        [5.0, 2.0, 3.0, -0.1, 0.3, 1.5, 0.05, 0.02, 100.0],
    ]
    B = len(rows)
    wl = gl.workloads.Workload("NFWT", phys, prior, cfg, B)
    sim = gl.LensSimulator(phys, cfg, bs=B)
    packed = torch.tensor(rows, dtype=torch.float32, device="cuda")
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    obs_np = obs.cpu().numpy()
    ll_o, red_o, g_o, img_o = H.oracle_loglike_and_grad(wl, packed.cpu().double(), obs_np, None, B)
    img = sim.simulate(packed).cpu().numpy().reshape(img_o.shape)
    assert np.abs(img - img_o).max() <= IMG_RTOL * np.abs(img_o).max() + 1e-7
    pm = gl.ForwardProbModel(prior, obs_np, wl.background_rms, wl.exp_time, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, _ = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    assert {"2": "gl_clusterw_kernel", "1": "gl_cluster_kernel", "0": "gl_main_kernel"}[cluster] in sim._model.last_main_kernel()
    assert np.allclose(ll.detach().cpu().numpy(), ll_o, rtol=LL_RTOL)
    g = p.grad.cpu().numpy()
    bad = ~(H.grad_col_err(g, g_o) <= GRAD_RTOL_COL)
    assert not bad.any(), (np.argwhere(bad)[:8], g[bad][:8], g_o[bad][:8], H.grad_col_err(g, g_o).max())


def test_dispatched_kernels_do_not_spill(gl):
    """Ask the library which kernel each BASELINE config really launched (gl_model_last_main_kernel) for simulate(), its VJP,
    the log-likelihood and the fused forward+gradient, and check that instantiation's code-object metadata: no VGPR
    spills.  The names must be the ones tests/test_kernel_resources.py lists (the CPU half of this check)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_flops as isa
    from tests.test_kernel_resources import DISPATCHED
    meta = isa.kernel_metadata(isa.code_object())
    by_symbol = {v["symbol"]: (k, v) for k, v in meta.items()}
    table = {"C1": "C1 SIE | Sersic", "C2": "C2 EPL+Shear | Sersic", "C3": "C3 EPL+Shear | Shapelets", "C4": "C4 / C5 8 NFW | 20 Sersic",
             "C5": "C4 / C5 8 NFW | 20 Sersic"}
    for name in ("C1", "C2", "C3", "C4", "C5"):
        wl = gl.workloads.make(name, num_pix=32, batch=4)
        obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
        sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
        packed = H.sample_packed(wl, sim, seed=1)
        m = sim._model
        seen = []
        img = m.simulate_fwd(packed)
        seen.append(m.last_main_kernel())
        m.simulate_bwd(packed, torch.ones_like(img))
        seen.append(m.last_main_kernel())
        m.loglike(packed, obs, err, None, wl.background_rms, wl.exp_time, False)
        seen.append(m.last_main_kernel())
        m.loglike(packed, obs, err, None, wl.background_rms, wl.exp_time, True)
        seen.append(m.last_main_kernel())
        for sym, want in zip(seen, DISPATCHED[table[name]]):
            dem, md = by_symbol[sym]
            assert want in dem, (name, dem, want)
            assert md["vgpr_spill_count"] == 0, (name, dem, md)


# ---------------------------------------------------------------------------------------------------
# PSF convolution + supersampling (tf/simulator.py:60-70,142-156) -- the image-materialising path
# ---------------------------------------------------------------------------------------------------
def _gauss_psf(n, sigma, seed=0):
    r = np.random.default_rng(seed)
    ax = np.arange(n) - (n - 1) / 2
    k = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * sigma ** 2)) * (1 + 0.1 * r.uniform(size=(n, n)))  # asymmetric
    return (k / k.sum()).astype(np.float32)


@pytest.mark.parametrize("ss,ksize,n,B", [(1, 7, 22, 3), (2, 0, 22, 3), (2, 9, 22, 3), (3, 5, 22, 3), (2, 8, 22, 3),
                                          (2, 13, 60, 5),   # the reference's demo geometry: 27-tap effective kernel, several tiles, odd batch
                                          (1, 13, 60, 4),
                                          (2, 33, 36, 2)])  # wider than the register-blocked kernel serves: the tap-by-tap kernels
def test_psf_supersample_vs_oracle(gl, ss, ksize, n, B, monkeypatch):
    """simulate(), the pixel likelihood and their gradients with a PSF and / or supersampling against the float64 oracle --
    through the register-blocked sample-pair correlation (gl_corr_pair_kernel: supersample <= 2, effective kernel <= 32 taps
    wide; forward = stride-ss correlation, transpose = ss^2 decimated flipped sub-kernels) and through the tap-by-tap
    kernels that serve everything else."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    from oracle import ref_torch as ref
    from tests.test_prior_host import default_prior
    if (ss, ksize, n) == (1, 13, 60):  # batches beyond the launch's grid.z go out in slices: forced here to one pair per slice
        monkeypatch.setenv("GIGALENS_HIP_CORR_MAXPAIRS", "1")
    phys = PhysicalModel([EPL(), Shear()], [SersicEllipse()], [SersicEllipse()])
    prior = default_prior()
    psf = _gauss_psf(ksize, 1.2 * ss) if ksize else None
    cfg = SimulatorConfig(delta_pix=0.08, num_pix=n, supersample=ss)
    sim = gl.LensSimulator(phys, cfg, bs=B, supersampled_kernel=psf)
    wl = gl.workloads.Workload("PSF", phys, prior, cfg, B)
    packed = H.sample_packed(wl, sim, seed=4)
    rs = ref.RefSimulator(phys, cfg, B, dtype=torch.float64, supersampled_kernel=psf)
    p64 = packed.cpu().double().requires_grad_(True)
    img_o = rs.simulate(H.struct_from_packed(phys, p64))
    r = np.random.default_rng(1)
    obs = (img_o[0].detach().numpy() + 0.3 * r.normal(size=(n, n))).astype(np.float32)
    ll_o, red_o = ref.stats_pixels(rs, H.struct_from_packed(phys, p64), obs, 0.2, 100.0)
    (g_o,) = torch.autograd.grad(ll_o.sum(), p64)
    img = sim.simulate(packed)
    assert img.shape == (B, n, n)
    assert np.abs(img.cpu().numpy() - img_o.detach().numpy()).max() <= IMG_RTOL * float(img_o.abs().max())
    pm = gl.ForwardProbModel(prior, obs, 0.2, 100.0, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, red = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    assert np.allclose(ll.detach().cpu().numpy(), ll_o.detach().numpy(), rtol=LL_RTOL)
    assert np.allclose(red.detach().cpu().numpy(), red_o.detach().numpy(), rtol=LL_RTOL)
    g, go = p.grad.cpu().numpy(), g_o.numpy()
    # The gate: every element within GRAD_RTOL_COL of its column's scale (oracle rows), or -- a sample whose source centre maps
    # next to a pixel has gradients with a condition number of 1e3-1e4 in the rounding of beta = x - alpha, whatever the
    # formulation (seed 4, row 1 of the 60 x 60 cases: HIP 3.8e-3, the reference's algorithm in float32 3.4e-4, every other row
    # 3e-7) -- within 4 x what one float32 rounding of beta does to that element of the ORACLE's gradient
    # (helpers.float32_conditioning_bound).  That HIP draws from the same error distribution as the reference's algorithm in
    # float32 over hundreds of samples is test_gradient_error_distribution_vs_float32_reference below.
    p64c = packed.cpu().double()
    ok, rep = H.grad_gate(g, go, GRAD_RTOL_COL, lambda S: H.float32_conditioning_bound(
        wl, p64c, obs, None, B, go, S, bg=(0.2, 100.0), supersampled_kernel=psf))
    assert ok, rep
    # image-boundary pair through autograd (gl_simulate_bwd with the transposed PSF / pooling)
    p2 = packed.clone().requires_grad_(True)
    w = torch.as_tensor(r.normal(size=(B, n, n)).astype(np.float32), device=p2.device)
    (sim.simulate(p2) * w).sum().backward()
    (g2_o,) = torch.autograd.grad((rs.simulate(H.struct_from_packed(phys, p64)) * w.cpu().double()).sum(), p64)

    def bound2(S):  # the same yardstick for the linear functional sum(w * image)
        out = np.zeros_like(g2_o.numpy())
        d = float(np.spacing(np.float32(float(rs.img_X.abs().max()))))
        for sx, sy in ((d, d), (d, -d)):
            rs_p = ref.RefSimulator(phys, cfg, B, dtype=torch.float64, supersampled_kernel=psf)
            rs_p.img_X, rs_p.img_Y = rs_p.img_X + sx, rs_p.img_Y + sy
            pp = packed.cpu().double().requires_grad_(True)
            (gp,) = torch.autograd.grad((rs_p.simulate(H.struct_from_packed(phys, pp)) * w.cpu().double()).sum(), pp)
            out = np.maximum(out, np.abs(gp.numpy() - g2_o.numpy()) / S)
        return out
    ok2, rep2 = H.grad_gate(p2.grad.cpu().numpy(), g2_o.numpy(), GRAD_RTOL_COL, bound2)
    assert ok2, rep2
    # the z-space entry uses the same path
    z = pm.bij.inverse(prior.sample(B, seed=9)).to("cuda")
    lp, red2, gz = pm.log_prob_and_grad(sim, z)
    zz = z.clone().requires_grad_(True)
    lpu, _ = pm.log_prob_unfused(sim, zz)
    lpu.sum().backward()
    assert torch.allclose(lp, lpu.detach(), rtol=LL_RTOL, atol=1e-3)
    sc = zz.grad.abs().max(dim=1, keepdim=True).values
    assert ((gz - zz.grad).abs() <= 5e-4 * sc + 1e-4).all()


# ---------------------------------------------------------------------------------------------------
# edge cases: degenerate compositions, truncated series, exact-zero ellipticity, large / tiny batches
# ---------------------------------------------------------------------------------------------------
def _edge_case(gl, phys, prior, n, B, seed=3):
    from gigalens_amd.simulator import SimulatorConfig
    wl = gl.workloads.Workload("EDGE", phys, prior, SimulatorConfig(delta_pix=0.07, num_pix=n), B)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(phys, wl.sim_config, bs=B)
    packed = H.sample_packed(wl, sim, seed=seed)
    ll_o, red_o, g_o, img_o = H.oracle_loglike_and_grad(wl, packed.cpu().double(), obs.cpu().numpy(), None, B)
    img = sim.simulate(packed).cpu().numpy().reshape(img_o.shape)
    assert np.abs(img - img_o).max() <= IMG_RTOL * np.abs(img_o).max() + 1e-7
    pm = gl.ForwardProbModel(prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, red = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    assert np.allclose(ll.detach().cpu().numpy().reshape(-1), ll_o.reshape(-1), rtol=LL_RTOL)
    g = p.grad.cpu().numpy()
    bad = H.grad_col_err(g, g_o) > GRAD_RTOL_COL
    assert not bad.any(), (np.argwhere(bad)[:5], g[bad][:5], g_o[bad][:5], H.grad_col_err(g, g_o).max())


def test_edge_compositions(gl):
    import math
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.sis import SIS
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    ser = lambda: J(dict(R_sersic=tfd.LogNormal(math.log(0.3), 0.1), n_sersic=tfd.Uniform(1, 3), center_x=tfd.Normal(0, 0.1),
                         center_y=tfd.Normal(0, 0.1), Ie=tfd.LogNormal(math.log(50.0), 0.3)))
    # lens light only -- no lens, no source (no deflection at all)
    _edge_case(gl, PhysicalModel([], [Sersic()], []), J(dict(lens_light=S([ser()]))), 18, 3)
    # source only, seen without a lens
    _edge_case(gl, PhysicalModel([], [], [Sersic()]), J(dict(source_light=S([ser()]))), 18, 2)
    # SIS lens (interpreter kernel), one-sample batch: bs == 1 squeezes the outputs like tf.squeeze
    sis = J(dict(theta_E=tfd.LogNormal(math.log(0.5), 0.1), center_x=tfd.Normal(0, 0.02), center_y=tfd.Normal(0, 0.02)))
    _edge_case(gl, PhysicalModel([SIS()], [], [Sersic()]), J(dict(lens_mass=S([sis]), source_light=S([ser()]))), 21, 1)
    # EPL whose series is cut by a small `niter` cap (epl.py:15,51): truncation must match the reference's
    epl = J(dict(theta_E=tfd.LogNormal(math.log(0.5), 0.1), gamma=tfd.TruncatedNormal(2, 0.25, 1, 3), e1=tfd.Normal(0.3, 0.05),
                 e2=tfd.Normal(-0.2, 0.05), center_x=tfd.Normal(0, 0.02), center_y=tfd.Normal(0, 0.02)))
    _edge_case(gl, PhysicalModel([EPL(niter=6)], [SersicEllipse()], [Sersic()]),
               J(dict(lens_mass=S([epl]), lens_light=S([J(dict(R_sersic=tfd.LogNormal(0, 0.1), n_sersic=tfd.Uniform(2, 4),
                 e1=tfd.Normal(0, 0.1), e2=tfd.Normal(0, 0.1), center_x=tfd.Normal(0, 0.02), center_y=tfd.Normal(0, 0.02),
                 Ie=tfd.LogNormal(math.log(20.0), 0.2)))]), source_light=S([ser()]))), 20, 4)


def test_epl_circular_and_large_batch(gl):
    """e1 = e2 = 0 exactly: f = 0, the series has a single term (epl.py:37: log(1e-12)/log(0) + 2 = 2); and a batch
    larger than one grid row of workgroups, with fewer pixels than one tile."""
    wl = gl.workloads.make("C2", num_pix=12, batch=2500)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=2)
    packed[:7, 2] = 0.0
    packed[:7, 3] = 0.0
    sub = torch.cat([packed[:12], packed[-5:]])
    ll_o, red_o, g_o, img_o = H.oracle_loglike_and_grad(gl.workloads.make("C2", num_pix=12, batch=17), sub.cpu().double(),
                                                        np.ones((12, 12), np.float32), None, 17)
    pm = gl.ForwardProbModel(wl.prior, np.ones((12, 12), np.float32), wl.background_rms, wl.exp_time, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, _ = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    got = torch.cat([ll.detach()[:12], ll.detach()[-5:]]).cpu().numpy()
    assert np.allclose(got, ll_o, rtol=LL_RTOL)
    g = torch.cat([p.grad[:12], p.grad[-5:]]).cpu().numpy()
    # d/de at e == 0 is undefined in the reference (sqrt'(0) * 0 = NaN in TF / torch); here it is defined as 0
    assert np.all(np.isnan(g_o[:7, 2:4])) and np.all(g[:7, 2:4] == 0)
    keep = np.ones_like(g, dtype=bool)
    keep[:7, 2:4] = False
    assert H.grad_col_err(np.where(keep, g, 0.0), np.where(keep, g_o, 0.0)).max() <= GRAD_RTOL_COL
    with pytest.raises(__import__("gigalens_amd._native", fromlist=["x"]).NativeLibraryError):
        sim._model.simulate_fwd(torch.zeros((70000, sim._model.P), device="cuda"))  # B > 65535: refused, not truncated


def test_hip_graph_capture(gl):
    """No per-call allocation / synchronisation inside the library: a whole forward+gradient call sequence can be
    captured into a HIP graph and replayed (tf.function-style reuse for the HMC leapfrog loop)."""
    wl = gl.workloads.make("C2", num_pix=32, batch=16)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    z = pm.bij.inverse(wl.prior.sample(wl.batch, seed=4)).to("cuda").contiguous()
    lp0, red0, g0 = pm.log_prob_and_grad(sim, z)  # warm-up: binds the prior, sizes the workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lp, red, g = pm.log_prob_and_grad(sim, z)
    z.add_(0.01)
    graph.replay()
    torch.cuda.synchronize()
    lp1, red1, g1 = pm.log_prob_and_grad(sim, z)
    assert torch.equal(lp, lp1) and torch.equal(g, g1) and not torch.equal(lp, lp0)


def test_partial_renders(gl):
    """simulate(no_deflection=True), simulate_source, simulate_lens_light, simulate_images (tf/simulator.py:125-126,242-328)."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    from oracle import ref_torch as ref
    from tests.test_prior_host import default_prior
    phys = PhysicalModel([EPL(), Shear()], [SersicEllipse()], [SersicEllipse()])
    cfg = SimulatorConfig(delta_pix=0.07, num_pix=26)
    B = 3
    sim = gl.LensSimulator(phys, cfg, bs=B)
    x = default_prior().sample(B, seed=8)
    full, nodefl = sim.simulate(x), sim.simulate(x, no_deflection=True)
    src, ll, arcs = sim.simulate_source(x), sim.simulate_lens_light(x), sim.simulate_images(x)
    tol = dict(rtol=1e-5, atol=1e-5 * float(full.abs().max()))
    assert torch.allclose(full, ll + arcs, **tol) and torch.allclose(nodefl, ll + src, **tol)
    assert not torch.allclose(arcs, src, **tol)
    rs = ref.RefSimulator(phys, cfg, B, dtype=torch.float64)
    x64 = {k: [{n: v.double().cpu() for n, v in d.items()} for d in lst] for k, lst in x.items()}
    o = rs.simulate(x64, no_deflection=True).numpy()
    assert np.abs(nodefl.cpu().numpy() - o).max() <= IMG_RTOL * np.abs(o).max()
    # the helpers accept only the group they need, like the reference's
    only_src = sim.simulate_source({"source_light": x["source_light"]})
    assert torch.equal(only_src, src)


def test_pair_correlation_matches_tap_kernels_on_random_shapes(gl, monkeypatch):
    """The register-blocked sample-pair correlation (gl_corr_pair_kernel) against the tap-by-tap PSF / pooling kernels on random
    geometries: image sizes off the tile grid, even and odd PSF sizes down to 1 x 1, rectangular PSFs, supersample 1 and 2,
    odd batches and a batch of one -- simulate() and its VJP agree to rounding."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    r = np.random.default_rng(7)
    phys = PhysicalModel([SIE()], [], [Sersic()])
    wl0 = gl.workloads.make("C1")
    for trial in range(24):
        ss = int(r.integers(1, 3))
        n = int(r.integers(5, 71))
        kh, kw = (int(r.integers(1, 17)), int(r.integers(1, 17))) if trial % 3 else (int(r.integers(1, 17)),) * 2
        B = int(r.choice([1, 2, 3, 5, 8]))
        psf = r.uniform(0.1, 1.0, size=(kh, kw)).astype(np.float32)
        psf /= psf.sum()
        if trial == 5:
            psf = None
            ss = 2
        cfg = SimulatorConfig(delta_pix=0.08, num_pix=n, supersample=ss)
        wl = gl.workloads.Workload("F", phys, wl0.prior, cfg, B)
        res = {}
        for flag in ("1", "0"):
            monkeypatch.setenv("GIGALENS_HIP_CORR_PAIR", flag)
            sim = gl.LensSimulator(phys, cfg, bs=B, supersampled_kernel=psf)
            packed = H.sample_packed(wl, sim, seed=trial)
            p = packed.clone().requires_grad_(True)
            img = sim.simulate(p)
            w = torch.as_tensor(np.random.default_rng(trial).normal(size=tuple(img.shape)).astype(np.float32), device=img.device)
            (img * w).sum().backward()
            res[flag] = (img.detach(), p.grad.clone())
        a, b = res["1"], res["0"]
        assert torch.allclose(a[0], b[0], rtol=2e-5, atol=2e-6 * float(b[0].abs().max())), (trial, ss, n, kh, kw, B)
        sc = b[1].abs().amax(dim=1, keepdim=True).clamp_min(1e-20)
        assert float(((a[1] - b[1]).abs() / sc).max()) < 2e-4, (trial, ss, n, kh, kw, B)


def test_log_prob_and_grad_from_a_hip_graph_equals_stream_launches(gl):
    """BASELINE configs[0] (one 64 x 64 sample) is host-issue bound; ``log_prob_and_grad(..., graph=True)`` replays the launch
    sequence from a HIP graph.  Same bits as the stream launches, for a new ``z`` (copied in) and for the graph's own input
    updated in place; the outputs are static (overwritten by the next replay), as documented."""
    wl = gl.workloads.make("C1", batch=3)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    z1 = pm.bij.inverse(wl.prior.sample(wl.batch, seed=1)).to("cuda").contiguous()
    z2 = pm.bij.inverse(wl.prior.sample(wl.batch, seed=2)).to("cuda").contiguous()
    a1 = [t.clone() for t in pm.log_prob_and_grad(sim, z1)]
    a2 = [t.clone() for t in pm.log_prob_and_grad(sim, z2)]
    g1 = pm.log_prob_and_grad(sim, z1, graph=True)
    assert all(torch.equal(x, y) for x, y in zip(a1, g1))
    g2 = pm.log_prob_and_grad(sim, z2, graph=True)
    assert all(torch.equal(x, y) for x, y in zip(a2, g2))
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(g1, g2))  # static outputs
    zs = pm.graph_input(sim, z1)
    g3 = pm.log_prob_and_grad(sim, zs, graph=True)
    assert all(torch.equal(x, y) for x, y in zip(a1, g3))
    zs.copy_(z2)
    g4 = pm.log_prob_and_grad(sim, zs, graph=True)
    assert all(torch.equal(x, y) for x, y in zip(a2, g4))


def test_shapelet_cull_changes_no_bit(gl, monkeypatch):
    """Table-mode shapelet kernel: wave-tiles provably outside the table skip the lens (csrc/gl_shp.hip.h shp_cull_setup).  Nothing
    of such a tile's lens evaluation reaches an output, so log-likelihood and gradient with the test on equal those with it off
    bit for bit -- and the test does fire on this geometry (the kernel's own count of tiles that ran the lens)."""
    wl = gl.workloads.make("C3", batch=6)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("GIGALENS_HIP_SHP_CULL", flag)
        sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
        packed = H.sample_packed(wl, sim, seed=3)
        ll, chi, g = sim._model.loglike(packed, obs, err, None, wl.background_rms, wl.exp_time, True)
        rows = sim._model.partial_rows(wl.batch)
        pk = rows[:, :, 3].double()
        out[flag] = (ll.clone(), chi.clone(), g.clone(), float(torch.remainder(pk, 4096.0).sum()), float(torch.floor(pk / 4096.0).sum()))
    assert torch.equal(out["1"][0], out["0"][0]) and torch.equal(out["1"][1], out["0"][1]) and torch.equal(out["1"][2], out["0"][2])
    assert out["0"][4] == out["0"][3]                     # test off: every wave-tile ran the lens
    assert out["1"][3] == out["0"][3] and out["1"][4] < 0.9 * out["1"][3]  # test on: at least a tenth of them did not
