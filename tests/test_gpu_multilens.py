"""Multi-plane ray tracing (csrc/gl_multiplane.hip.h) on the GPU against the float64 restatement of tests/multilens_cases.py.

Lens maps: K = 2 and K = 3, EPL + Shear | SIE, NFW | dPIE | SIS (the target between planes 2 and 3, and behind all three), two lenses
sharing a plane, dPIS | SIE (the convergence excess of the dPIS Hessian, reference: the explicit Jacobian recursion); B = 1 and 3; 70 points (one full wave and a tail) and 1 point, replicated per sample (xy_batched) and shared.  beta
and all four entries of A are checked at every point.  Renders: 16 x 16 without PSF, 12 x 12 at supersample 2 with a 5 x 5 PSF, a
13 x 13 ``pix_region``, 11 x 11 with a CoreSersic lens light; a source between the planes, one behind both, a lens light.

Gates (nothing invented): the yardstick of a quantity of a case is the worst deviation of the same restatement run in float32 on the
CPU from its float64 result, and the kernel must stay within 4 x it (the factor of tests/pixsrc_cases.py).  A lens-map case is a lens
set with its target; its yardstick is taken on its 70 points x 3 samples, of which the smaller shapes (1 point, 1 sample) are
subsets -- one point's float32 error is a single draw of the distribution those 210 sample.  Every figure is printed before it is
asserted."""
import ctypes

import numpy as np
import pytest
import torch

from tests import multilens_cases as MC
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
_SIMS = {}


def _t(params):
    return {g: [{k: torch.as_tensor(v) for k, v in d.items()} for d in lst] for g, lst in params.items()}


def _map_sim(gl, name, B):
    """One simulator per (lens set, batch size), shared by the tests (the grid is irrelevant to the lens maps)."""
    from gigalens_amd.simulator import SimulatorConfig
    if (name, B) not in _SIMS:
        _SIMS[name, B] = gl.LensSimulator(MC.map_case(name)["phys_mp"], SimulatorConfig(delta_pix=0.1, num_pix=8), bs=B)
    return _SIMS[name, B]


def _lens_t(lens_params, B):
    return [{k: torch.as_tensor(v) for k, v in d.items()} for d in MC.sample_rows(lens_params, B)]


# ---- lens maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("n_pts", [70, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", MC.MAP_CASES)
def test_maps_against_float64(gl, name, B, n_pts, batched):
    c, x, y, ref, _ = MC.map_data(name, n_pts, B)
    _, _, _, ref_case, yard = MC.map_data(name, 70, 3)
    sim = _map_sim(gl, name, B)
    lp = _lens_t(c["lens_params"], B)
    if batched:  # the public calls: points replicated per sample on the device
        xt, yt = torch.as_tensor(x).reshape(-1, 1), torch.as_tensor(y).reshape(-1, 1)
        bx, by = sim.beta(xt, yt, lp, deflection_scale=c["target"])
        fxx, fxy, fyx, fyy = sim._hessian(xt, yt, lp, c["target"])
        native = torch.stack([bx, by, fxx, fxy, fyx, fyy])
        kap, (g1, g2), mu, rot = (sim.convergence(xt, yt, lp, c["target"]), sim.shear(xt, yt, lp, c["target"]),
                                  sim.magnification(xt, yt, lp, c["target"]), sim.rotation(xt, yt, lp, c["target"]))
        # the same definitions the single-plane calls apply to I - H, bit for bit on the maps above
        assert torch.equal(kap, 0.5 * (fxx + fyy)) and torch.equal(g1, 0.5 * (fxx - fyy)) and torch.equal(g2, fxy)
        assert torch.equal(mu, 1.0 / ((1 - fxx) * (1 - fyy) - fxy * fyx)) and torch.equal(rot, 0.5 * (fyx - fxy))
    else:        # [n] points every sample shares
        native = sim._model.multiplane_maps(sim._pack_partial({"lens_mass": lp}), x, y, c["target"], shared_points=True)
    assert tuple(native.shape) == (6, n_pts, B)
    got = MC.as_jacobian(native.cpu().numpy())
    assert np.isfinite(got).all()
    e = MC.map_errors(got, ref, *MC.points(70), a_scale=np.abs(ref_case[2:]).max())  # the scales of the case, whatever the subset
    for k in MC.MAP_KEYS:
        print(f"{name} B={B} n={n_pts} batched={batched} {k}: kernel error {e[k]:.3e}, yardstick {yard[k]:.3e}, gate {4 * yard[k]:.3e}")
    for k in MC.MAP_KEYS:
        assert e[k] <= 4 * yard[k], (name, B, n_pts, batched, k, e[k], yard[k])


def test_source_index_selects_the_source_plane(gl):
    """``deflection_scale=s`` (an int) is the plane of source s: the couplings ``source_scales[:, s]``."""
    c = MC.render_case("plain16")
    sim = _render_sim(gl, "plain16")
    x, y = (torch.as_tensor(v).reshape(-1, 1) for v in MC.points(70))
    lp = _t(c["params"])["lens_mass"]
    for s in (0, 1):
        a = sim.beta(x, y, lp, deflection_scale=s)
        b = sim.beta(x, y, lp, deflection_scale=c["mp"].source_scales[:, s])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(sim.beta(x, y, lp, deflection_scale=0)[0], sim.beta(x, y, lp, deflection_scale=1)[0])
    for bad in (1.0, 2, -1, [0.5], [0.5, float("nan")], True):
        with pytest.raises(ValueError):
            sim.beta(x, y, lp, deflection_scale=bad)


def test_two_shear_planes_closed_form(gl):
    from gigalens_amd.simulator import SimulatorConfig
    phys, phys_mp, mp, lp, T, A = MC.two_shear_case()
    x, y = MC.points(70)
    ref = MC.maps(phys, mp, lp, x, y, T)
    yard = MC.map_errors(MC.maps(phys, mp, lp, x, y, T, MC.F32), ref, x, y)
    sim = gl.LensSimulator(phys_mp, SimulatorConfig(delta_pix=0.1, num_pix=8), bs=1)
    lt = _lens_t(lp, 1)
    xt, yt = torch.as_tensor(x).reshape(-1, 1), torch.as_tensor(y).reshape(-1, 1)
    native = sim._model.multiplane_maps(sim._pack_partial({"lens_mass": lt}), xt, yt, T).cpu().numpy()
    closed = np.empty_like(ref)
    closed[:2] = (A @ np.stack([x, y]).astype(np.float64))[:, :, None]
    closed[2:] = A.reshape(4, 1, 1)
    assert max(MC.map_errors(ref, closed, x, y).values()) <= 1e-14  # the restatement IS the closed form
    e = MC.map_errors(MC.as_jacobian(native), closed, x, y)
    yb, yA = MC.closed_form_yardstick(yard, MC.MAP_KEYS[:2]), MC.closed_form_yardstick(yard, MC.MAP_KEYS[2:])
    for k in MC.MAP_KEYS:
        gate = 4 * (yb if k.startswith("beta") else yA)
        print(f"two Shear planes {k}: kernel error {e[k]:.3e}, float32 restatement {yard[k]:.3e}, gate {gate:.3e}")
        assert e[k] <= gate, (k, e[k], gate)
    # the rotation: sign and value, C_2t C_12 g1 g2 > 0 (its scale is A's, as for the entries it is made of)
    rot = sim.rotation(xt, yt, lt, T).cpu().numpy().astype(np.float64)
    want = 0.5 * (A[0, 1] - A[1, 0])
    assert want > 1e-3 and (rot > 0).all()
    s_A = np.abs(A).max()
    err = np.abs(rot - want).max() / s_A
    print(f"two Shear planes rotation: kernel error {err:.3e}, gate {4 * yA:.3e}")
    assert err <= 4 * yA


def test_two_coaxial_sis_planes_closed_form(gl):
    from gigalens_amd.simulator import SimulatorConfig
    phys, phys_mp, mp, lp, T, x, y, th2, beta = MC.two_sis_case()
    ref = MC.maps(phys, mp, lp, x, y, T)
    yard = MC.map_errors(MC.maps(phys, mp, lp, x, y, T, MC.F32), ref, x, y)
    sim = gl.LensSimulator(phys_mp, SimulatorConfig(delta_pix=0.1, num_pix=8), bs=1)
    lt = _lens_t(lp, 1)
    xt, yt = torch.as_tensor(x).reshape(-1, 1), torch.as_tensor(y).reshape(-1, 1)
    bx, by = (v.cpu().numpy().astype(np.float64)[:, 0] for v in sim.beta(xt, yt, lt, deflection_scale=T))
    t2 = sim.beta(xt, yt, lt, deflection_scale=[mp.lens_scales[0, 1], 0.0])[0].cpu().numpy().astype(np.float64)[:, 0]
    s = float(np.abs(x).max())
    for what, got, want in (("beta_x", bx, beta), ("beta_y", by, 0 * beta), ("theta_2", t2, th2)):
        err = np.abs(got - want).max() / s
        gate = 4 * MC.closed_form_yardstick(yard, MC.MAP_KEYS[:2])
        print(f"two SIS planes {what}: kernel error {err:.3e}, gate {gate:.3e}")
        assert err <= gate, (what, err, gate)
    assert (np.sign(t2) == np.sign(th2)).all()


def test_empty_second_plane_equals_the_scaled_single_plane(gl):
    """K = 2 with a zero-strength lens alone on the second plane: the maps of the existing single-plane kernels with
    ``deflection_scale = C_1t``, to the gate of the lens set."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import SimulatorConfig
    base = MC.map_case("shared")["lens_params"]
    lp = [base[0], base[2], {"theta_E": MC._f32(0.0, 0.0, 0.0), "center_x": base[1]["center_x"], "center_y": base[1]["center_y"]}]
    lenses = [SIE(), Shear(), SIS()]
    mp = MC._mp([0.4, 0.4, 0.9])
    T = mp.target_scales(1.8)
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    sim2 = gl.LensSimulator(PhysicalModel(lenses, [], [], multiplane=mp), cfg, bs=3)
    sim1 = gl.LensSimulator(PhysicalModel(lenses, [], []), cfg, bs=3)
    x, y = MC.points(70)
    xt, yt = (torch.as_tensor(v, device=sim1.device).reshape(-1, 1) for v in (x, y))
    lt = [{k: v.to(sim1.device) for k, v in d.items()} for d in _lens_t(lp, 3)]  # (the plugin-level calls of the single-plane beta take device tensors)
    c1 = float(np.float32(T[0]))
    one = torch.stack([*sim1.beta(xt, yt, lt, deflection_scale=c1), *sim1._hessian(xt, yt, lt, c1)]).cpu().numpy()
    two = torch.stack([*sim2.beta(xt, yt, lt, deflection_scale=T), *sim2._hessian(xt, yt, lt, T)]).cpu().numpy()
    ref = MC.maps(PhysicalModel(lenses, [], []), mp, lp, x, y, T)
    yard = MC.map_errors(MC.maps(PhysicalModel(lenses, [], []), mp, lp, x, y, T, MC.F32), ref, x, y)
    e = MC.map_errors(MC.as_jacobian(two), MC.as_jacobian(one), x, y)
    for k in MC.MAP_KEYS:
        print(f"empty second plane {k}: multi-plane vs single-plane kernels {e[k]:.3e}, gate {4 * yard[k]:.3e}")
        assert e[k] <= 4 * yard[k], (k, e[k], yard[k])
    assert sim1._model.n_planes == 1 and sim2._model.n_planes == 2


# ---- renders -----------------------------------------------------------------------------------------------------------
def _render_sim(gl, name):
    if name not in _SIMS:
        c = MC.render_case(name)
        _SIMS[name] = gl.LensSimulator(c["phys_mp"], c["cfg"], bs=c["B"], supersampled_kernel=c["psf"])
    return _SIMS[name]


def _prior_of(params):
    """A prior with the structure of ``params`` (only its structure is used: ``stats_pixels`` takes constrained parameters)."""
    from gigalens_amd import prior as tfd
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    return J({g: S([J({k: tfd.Normal(float(v[0]), 0.1) for k, v in d.items()}) for d in lst]) for g, lst in params.items()})


@pytest.mark.parametrize("name", MC.RENDER_CASES)
def test_render_and_pixel_statistics_against_float64(gl, name):
    c, obs, ref, yard = MC.render_data(name)
    sim = _render_sim(gl, name)
    p = _t(c["params"])
    img = sim.simulate(p)
    assert tuple(img.shape) == ref["image"].shape and bool(torch.isfinite(img).all())
    assert torch.equal(img, sim.simulate(p)), "two calls must give identical bits"
    if c["cfg"].pix_region is not None:  # pixels outside the region are exact zeros
        assert bool((img[:, torch.as_tensor(c["cfg"].pix_region == 0, device=img.device)] == 0).all())
    pm = gl.ForwardProbModel(_prior_of(c["params"]), obs, MC.BG, MC.TEXP, include_positions=False)
    ll, red = pm.stats_pixels(sim, p)
    ll2, red2 = pm.stats_pixels(sim, p)
    assert torch.equal(ll, ll2) and torch.equal(red, red2)
    got = dict(image=img.cpu().numpy(), log_like=ll.cpu().numpy(), red_chi2=red.cpu().numpy())
    e = {k: MC.rel_err(got[k], ref[k]) for k in yard}
    for k in yard:
        print(f"{name} {k}: kernel error {e[k]:.3e}, yardstick {yard[k]:.3e}, gate {4 * yard[k]:.3e}")
    for k in yard:
        assert e[k] <= 4 * yard[k], (name, k, e[k], yard[k])


@pytest.mark.parametrize("method,parts", [("simulate_source", 4), ("simulate_lens_light", 2), ("simulate_images", 1 | 4)])
def test_partial_renders(gl, method, parts):
    """The partial renders follow the same rules (12 x 12 at supersample 2 with the PSF): the gate is the case's image gate, on the
    scale of the full image."""
    c, _, ref, yard = MC.render_data("psf12ss2")
    sim = _render_sim(gl, "psf12ss2")
    want, _ = MC.image(c["phys"], c["cfg"], c["psf"], c["mp"], c["params"], c["B"], MC.F64, parts=parts)
    got = getattr(sim, method)(_t(c["params"])).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want.numpy()).max() / np.abs(ref["image"]).max())
    print(f"{method}: kernel error {err:.3e}, gate {4 * yard['image']:.3e}")
    assert err <= 4 * yard["image"]
    if parts == 1 | 4:  # = the full image minus the lens light, to the same gate
        full = sim.simulate(_t(c["params"])).cpu().numpy() - sim.simulate_lens_light(_t(c["params"])).cpu().numpy()
        assert np.abs(got - full).max() / np.abs(ref["image"]).max() <= 4 * yard["image"]


def test_one_plane_runs_the_existing_kernels(gl):
    """``multiplane`` with K = 1 is ``source_light_scales``: the same kernel, the same bits."""
    from gigalens_amd.cosmology import MultiPlane, deflection_scale
    from gigalens_amd.model import PhysicalModel
    c = MC.render_case("plain16")
    ph = c["phys"]
    mp1 = MultiPlane([0.5, 0.5, 0.5], [0.8, 2.0], MC.Z_REF)
    a = gl.LensSimulator(PhysicalModel(ph.lenses, ph.lens_light, ph.source_light, multiplane=mp1), c["cfg"], bs=c["B"])
    b = gl.LensSimulator(PhysicalModel(ph.lenses, ph.lens_light, ph.source_light,
                                       source_light_scales=deflection_scale(0.5, [0.8, 2.0], MC.Z_REF)), c["cfg"], bs=c["B"])
    ia, ib = a.simulate(_t(c["params"])), b.simulate(_t(c["params"]))
    assert torch.equal(ia, ib) and a._model.last_main_kernel() == b._model.last_main_kernel()
    assert a._mp is None and a._model.n_planes == 1 and "gl_mp_" not in a._model.last_main_kernel()


# ---- refusals and state ------------------------------------------------------------------------------------------------
def test_refused_entries(gl):
    from gigalens_amd import _native
    c, obs, _, _ = MC.render_data("plain16")
    sim = _render_sim(gl, "plain16")
    p = _t(c["params"])
    packed = sim.pack(p)
    lens = p["lens_mass"]
    U = _native.UnsupportedLensError
    one = [np.array([0.5, -0.5], np.float32)]
    pm = gl.ForwardProbModel(_prior_of(c["params"]), obs, MC.BG, MC.TEXP, centroids_x=one, centroids_y=one, centroids_errors_x=one,
                             centroids_errors_y=one)
    z = pm.bij.inverse(pm.prior.sample(c["B"], seed=1)).to(sim.device)
    refused = {
        "simulate_bwd": lambda: sim._model.simulate_bwd(packed, torch.ones(3, 16, 16, device=sim.device)),
        "loglike with gradient": lambda: sim._model.loglike(packed, pm.observed_image, None, None, MC.BG, MC.TEXP, True),
        "log_prob (fused)": lambda: pm.log_prob(sim, z),
        "log_prob_and_grad": lambda: pm.log_prob_and_grad(sim, z),
        "term_log_prob_and_grad": lambda: pm.term_log_prob_and_grad(sim, z, "pixels"),
        "lstsq_simulate": lambda: sim.lstsq_simulate(p, obs, np.ones_like(obs)),
        "image_positions": lambda: sim.image_positions(lens, 0.1, 0.1),
        "critical_curves": lambda: sim.critical_curves(lens),
        "einstein_radius": lambda: sim.einstein_radius(lens),
        "potential": lambda: sim.potential(0.3, 0.2, lens),
        "fermat_potential": lambda: sim.fermat_potential(0.3, 0.2, 0.0, 0.0, lens),
        "time_delays": lambda: sim.time_delays(lens, 0.1, 0.1),
        "reconstruct_source": lambda: sim.reconstruct_source(p, obs, np.ones_like(obs), n_src=(4, 4), pitch=0.2),
        "stats_positions": lambda: pm.stats_positions(sim, p),
        "single-plane lens maps": lambda: sim._model.lens_maps(packed, 0.3, 0.2),
        "single-plane render": lambda: sim._model.simulate_fwd(packed),
    }
    for what, call in refused.items():
        with pytest.raises(U):
            call()
        print("refused:", what)
    # forward only: input that requires a gradient
    g = packed.clone().requires_grad_(True)
    for call in (lambda: sim.simulate(g), lambda: sim.simulate_images(g), lambda: sim.beta(0.3, 0.2, g, deflection_scale=0),
                 lambda: sim.magnification(0.3, 0.2, g, deflection_scale=0), lambda: pm._pixel_stats_packed(sim, g),
                 lambda: sim.rotation(torch.tensor([0.3], requires_grad=True), 0.2, lens, deflection_scale=0)):
        with pytest.raises(NotImplementedError):
            call()
    # the library refuses on its own, whatever the Python layer checks
    L = _native.lib()
    img = torch.empty((3, 16, 16), dtype=torch.float32, device=sim.device)
    ws = sim._model._workspace(3)
    rc = L.gl_simulate_fwd(sim._model._h, ctypes.c_void_p(packed.data_ptr()), 3, ctypes.c_void_p(img.data_ptr()),
                           ctypes.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert rc == _native.GL_EUNSUPPORTED and b"lens planes" in L.gl_last_error()
    out = torch.empty((6, 1, 3), dtype=torch.float32, device=sim.device)
    xy = torch.zeros(1, device=sim.device) + 0.3
    rc = L.gl_lens_maps(sim._model._h, ctypes.c_void_p(packed.data_ptr()), 3, ctypes.c_void_p(xy.data_ptr()),
                        ctypes.c_void_p(xy.data_ptr()), 1, 0, ctypes.c_void_p(out.data_ptr()), None)
    assert rc == _native.GL_EUNSUPPORTED


def test_refused_models(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.dpie_series import DPIESeries
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import SimulatorConfig
    from tests.test_user_profile_compile import SIS_BODY

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    mp = MC._mp([0.4, 0.9], [2.0])
    for second in (DPIESeries(2), UserSIS()):  # the field of a series lives on theta, not theta_j; user-written bodies
        with pytest.raises(_native.UnsupportedLensError):
            gl.LensSimulator(PhysicalModel([SIS(), second], [], [Sersic()], multiplane=mp), cfg, bs=1)
    # lights beyond the Sersic family (refused by the library when the planes are attached) and galaxy populations
    from gigalens_amd.profiles.light.shapelets import Shapelets
    from gigalens_amd.profiles.mass.scaling_relation import ScalingRelation
    with pytest.raises(_native.UnsupportedLensError):
        gl.LensSimulator(PhysicalModel([SIS(), SIS()], [], [Shapelets(4, interpolate=False)], multiplane=mp), cfg, bs=1)
    cat = dict(lum=np.array([1.0, 0.5], np.float32), center_x=np.array([0.3, -0.4], np.float32), center_y=np.array([0.1, 0.2], np.float32))
    pop = ScalingRelation(SIS(), ["theta_E"], 1.0, {"theta_E": 0.5}, cat)
    with pytest.raises(_native.UnsupportedLensError):
        gl.LensSimulator(PhysicalModel([SIS(), pop], [], [Sersic()], multiplane=mp), cfg, bs=1)


def test_native_set_lens_planes_refusals_and_reset(gl):
    from gigalens_amd import _native
    c = MC.render_case("plain16")
    fresh = gl.LensSimulator(c["phys"], c["cfg"], bs=c["B"])  # gl_model_create: a new model has no planes
    m = fresh._model
    packed = fresh.pack(_t(c["params"]))
    assert m.n_planes == 1
    with pytest.raises(_native.NativeLibraryError, match="gl_model_set_lens_planes has not been called"):
        m.multiplane_maps(packed, 0.3, 0.2, [0.5, 0.5])
    with pytest.raises(_native.NativeLibraryError, match="gl_model_set_lens_planes has not been called"):
        m.multiplane_simulate(packed)
    single = m.simulate_fwd(packed)
    mp = c["mp"]
    with pytest.raises(_native.UnsupportedLensError):  # more than 4 planes
        m.set_lens_planes([0, 1, 4], np.triu(np.ones((5, 5)), 1), np.ones((5, 2)))
    with pytest.raises(_native.NativeLibraryError, match="source"):  # couplings of 3 sources for 2 source lights
        m.set_lens_planes(mp.plane_of_lens, mp.lens_scales, np.ones((2, 3)))
    for bad in (dict(plane_of_lens=[0, 0]), dict(plane_of_lens=[0, 0, 2]), dict(plane_of_lens=[0, 0, 0]),
                dict(lens_scales=mp.lens_scales.T), dict(lens_scales=np.array([[0.0, float("nan")], [0.0, 0.0]])),
                dict(source_scales=np.array([[0.0, 1.0], [0.0, 0.5]])), dict(source_scales=np.array([[1.0, 1.0], [-0.5, 0.5]]))):
        kw = dict(plane_of_lens=mp.plane_of_lens, lens_scales=mp.lens_scales, source_scales=mp.source_scales)
        kw.update(bad)
        with pytest.raises(_native.NativeLibraryError):
            m.set_lens_planes(**kw)
    assert m.n_planes == 1 and torch.equal(m.simulate_fwd(packed), single)  # refused calls leave the model as it was
    m.set_lens_planes(mp.plane_of_lens, mp.lens_scales, mp.source_scales)
    assert m.n_planes == 2 and torch.equal(m.multiplane_simulate(packed), _render_sim(gl, "plain16")._model.multiplane_simulate(packed))
    with pytest.raises(_native.UnsupportedLensError):
        m.simulate_fwd(packed)
    again = gl.LensSimulator(c["phys"], c["cfg"], bs=c["B"])  # ... and the next model created starts without planes
    assert again._model.n_planes == 1 and torch.equal(again._model.simulate_fwd(packed), single)
