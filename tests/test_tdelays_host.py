"""The time-delay likelihood without a GPU: the float64 restatement of tests/tdelay_cases.py against the float64 host build of the
``*_pot`` templates, the envelope property the kernels' gradient rests on, the constructor's validation, the C ABI, the binding to
the native model (with the recording library of tests/test_model_binding_host.py) and the float32 yardsticks of the GPU test."""
import os
import re
import types

import numpy as np
import pytest
import torch

from gigalens_amd import _native
from tests import mp_positions_cases as PC
from tests import tdelay_cases as TC
from tests.test_model_binding_host import B, N_PIX, _RecordingModel, _z, library  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.CASES)
def test_paths_keep_their_distance_from_every_centre(name):
    d = TC.min_centre(TC.case(name))
    print(f"{name}: the paths keep {d:.3f} arcsec from every profile centre")
    assert d >= TC.MIN_CENTRE


@pytest.mark.parametrize("name", ("quad",) + TC.KIND_CASES)
def test_line_integral_equals_the_host_potential_differences(name):
    """psi(theta_j) - psi(anchor) of the line integral of the oracle's deflection against the float64 ``*_pot`` templates: 1e-9 of
    the largest difference, for every kind."""
    c = TC.case(name)
    p, lp = PC.leaf(c)
    rows = p.detach().numpy()
    for fam in c["fams"]:
        got = TC.psi_delta(c["phys"], lp, fam["x"], fam["y"], c["B"]).detach().numpy()
        ref = TC.host_psi_model(c, rows, fam["x"], fam["y"]) - TC.host_psi_model(c, rows, [TC.R_ANCHOR], [0.0])
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{name}: psi differences, line integral vs host templates {err:.2e} (largest difference {np.abs(ref).max():.3f})")
        assert err <= 1e-9


@pytest.mark.parametrize("name", ("quad", "quad_given", "quad_nan", "tnfw"))
def test_envelope_property(name):
    """autograd through the profiled lambda_f and T_f equals the partial derivative at fixed (lambda_f, T_f): the kernels' formula."""
    c = TC.case(name)
    ll, chi2, g, lam, T, model = TC.loglike_grad(c)
    ll_f, chi2_f, g_f, lam_f, T_f, _ = TC.loglike_grad(c, fixed=True)
    err = np.abs(g - g_f).max() / np.abs(g).max()
    print(f"{name}: total vs fixed-amplitude gradient {err:.2e}")
    assert np.array_equal(ll, ll_f) and np.array_equal(lam, lam_f) and np.array_equal(T, T_f)
    assert np.abs(g).max() > 0 and err <= 1e-10


def test_the_fixed_amplitude_formula_in_closed_form():
    """a_j = lambda w r_j, sum_M a_j = 0 (T minimises) and, lambda profiled, sum_M a_j phi_j = 0 (lambda minimises)."""
    c = TC.case("quad")
    p, lp = PC.leaf(c)
    fam = c["fams"][0]
    phi = TC.fermat(c, p, lp, fam).detach().requires_grad_(True)
    ll, chi2, lam, T, _ = TC.family_term(phi, fam["delay"], fam["delay_err"], fam["scale"], fixed=True)
    (a,) = torch.autograd.grad(ll.sum(), phi)
    w = torch.as_tensor(1.0 / fam["delay_err"].astype(np.float64) ** 2)[:, None]
    r = torch.as_tensor(fam["delay"].astype(np.float64))[:, None] - lam[None, :] * phi - T[None, :]
    assert torch.allclose(a, lam[None, :] * w * r, rtol=1e-12, atol=1e-12)
    scale = float(a.abs().max())
    assert float(a.sum(dim=0).abs().max()) <= 1e-10 * scale and float((a * phi.detach()).sum(dim=0).abs().max()) <= 1e-9 * scale


def test_a_shift_of_the_clock_or_of_the_potential_changes_nothing_but_the_offset():
    c = TC.case("quad")
    p, lp = PC.leaf(c)
    fam = c["fams"][0]
    phi = TC.fermat(c, p, lp, fam).detach()
    ll, chi2, lam, T, model = TC.family_term(phi, fam["delay"], fam["delay_err"], np.nan)
    ll2, chi22, lam2, T2, model2 = TC.family_term(phi + 3.0, fam["delay"].astype(np.float64) + 1000.0, fam["delay_err"], np.nan)
    assert torch.allclose(ll, ll2, rtol=1e-9) and torch.allclose(lam, lam2, rtol=1e-9)
    assert torch.allclose(model2, model + 1000.0, rtol=1e-9) and torch.allclose(T2, T + 1000.0 - 3.0 * lam, rtol=1e-9)


def test_a_family_without_delays_is_exactly_zero():
    c = TC.case("two_fams")
    _, ref, _ = TC.data("two_fams")
    _, ref1, _ = TC.data("quad")
    assert np.array_equal(ref["log_like"], ref1["log_like"]) and np.array_equal(ref["grad"], ref1["grad"])
    assert np.isnan(ref["scale"][:, 1]).all() and np.isnan(ref["offset"][:, 1]).all() and np.isnan(ref["model"][:, 4:]).all()
    assert TC.n_delay(c) == 4 and TC.n_delay(TC.case("quad_nan")) == 3 and TC.n_delay(TC.case("b65")) == 7


@pytest.mark.parametrize("name", TC.CASES)
def test_float32_yardsticks_stay_under_their_ceiling(name):
    _, ref, yard = TC.data(name)
    print(f"{name}: float32 yardsticks " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    assert np.isfinite(ref["log_like"]).all() and np.isfinite(ref["grad"]).all() and np.abs(ref["grad"]).max() > 0
    for k, v in yard.items():
        assert v <= TC.YARD_CEILING[k], (k, v)


# ---- the constructor -------------------------------------------------------------------------------------------------
def _pm(**kw):
    from gigalens_amd.model import ForwardProbModel
    from gigalens_amd import prior as tfd
    c = TC.case("two_fams")
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), 0.01) for k, v in d.items()}) for d in c["params"]["lens_mass"]])))
    args = dict(TC.centroids(c), include_pixels=False)
    args.update(kw)
    return ForwardProbModel(prior, **args)


def test_constructor_takes_the_delays():
    pm = _pm()
    assert pm.n_delay == 4.0 and pm.n_position == 14.0 and pm.n_flux == 0.0
    assert np.isnan(pm.centroids_time_delays[1]).all() and np.isnan(pm.time_delay_distances).all()
    t = [np.asarray([1.0, 5.0, np.nan, 3.0], np.float32), np.asarray([0.0, 2.0, 9.0], np.float32)]
    pm = _pm(centroids_time_delays=t, centroids_time_delays_errors=[0.5, np.asarray([0.1, 0.2, 0.3])], time_delay_distances=[3000.0, None])
    assert pm.n_delay == 6.0 and pm.centroids_time_delays_errors[0].tolist() == [0.5] * 4
    assert pm.time_delay_distances[0] == 3000.0 and np.isnan(pm.time_delay_distances[1])
    plain = _pm(centroids_time_delays=None, centroids_time_delays_errors=None, time_delay_distances=None)
    assert plain.n_delay == 0.0 and plain.centroids_time_delays is None
    with pytest.raises(ValueError, match="needs a model built with centroids_time_delays"):
        plain.stats_time_delays(None, None)
    with pytest.raises(ValueError, match="needs a model built with centroids_time_delays"):
        plain.fitted_time_delays(None, None)


def test_constructor_refusals():
    t4, t3 = np.asarray([1.0, 5.0, 2.0, 3.0], np.float32), np.asarray([0.0, 2.0, 9.0], np.float32)
    nan = np.float32(np.nan)
    bad = [
        (dict(centroids_time_delays_errors=None), "come together"),
        (dict(centroids_time_delays=None), "come together"),
        (dict(centroids_time_delays=None, centroids_time_delays_errors=None, time_delay_distances=[1.0, 2.0]), "time_delay_distances needs"),
        (dict(centroids_time_delays=[t4]), "one entry per image family"),
        (dict(centroids_time_delays=[t3, t3]), "has shape"),
        (dict(centroids_time_delays_errors=[None, 1.0]), "without centroids_time_delays_errors"),
        (dict(centroids_time_delays_errors=[np.ones(3), 1.0]), "does not broadcast"),
        (dict(centroids_time_delays=[np.asarray([1.0, np.inf, 2.0, 3.0], np.float32), None]), "must be finite"),
        (dict(centroids_time_delays_errors=[np.asarray([1.0, np.inf, 1.0, 1.0]), 1.0]), "must be finite"),
        (dict(centroids_time_delays_errors=[np.asarray([1.0, 0.0, 1.0, 1.0]), 1.0]), "must be > 0"),
        (dict(centroids_time_delays_errors=[np.asarray([1.0, -1.0, 1.0, 1.0]), 1.0]), "must be > 0"),
        (dict(centroids_time_delays=[np.asarray([1.0, nan, nan, nan], np.float32), None]), "one measured arrival time"),
        (dict(centroids_time_delays=[np.asarray([1.0, 4.0, nan, nan], np.float32), None]), "two measured arrival times with a profiled"),
        (dict(time_delay_distances=3000.0), "one float"),
        (dict(time_delay_distances=[3000.0]), "one entry per image family"),
        (dict(time_delay_distances=[np.inf, None]), "must be finite"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            _pm(**kw)
    # two measured times are a constraint once the distance is given; an unmeasured image's error is not looked at
    pm = _pm(centroids_time_delays=[np.asarray([1.0, 4.0, nan, nan], np.float32), None], time_delay_distances=[3000.0, None],
             centroids_time_delays_errors=[np.asarray([1.0, 1.0, -1.0, np.nan]), None])
    assert pm.n_delay == 2.0
    from gigalens_amd.model import ForwardProbModel
    with pytest.raises(ValueError, match="needs centroids_x"):
        ForwardProbModel(pm.prior, np.zeros((4, 4), np.float32), 0.1, 100.0, include_positions=False, centroids_time_delays=[t4],
                         centroids_time_delays_errors=[1.0])


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "gigalens_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("gl_model_set_position_delays", 6), ("gl_position_delays_fwd_bwd", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_native.SYMBOLS[name][1])
    assert "gl_tdelays.hip.h" in open(os.path.join(ROOT, "gigalens_amd", "csrc", "gl_api_points.hip")).read()


# ---- the binding -----------------------------------------------------------------------------------------------------
def _simulator(phys):
    region = torch.ones(N_PIX, N_PIX)
    return types.SimpleNamespace(_model=_RecordingModel(), _layout=phys._packing(), phys_model=phys, img_region=region,
                                 sim_config=types.SimpleNamespace(pix_region=None), _mp=phys.multiplane, _n_eff=None,
                                 _linear_cols_dev=None, _lp_graphs={}, _lp_captures=0)


def test_delays_are_handed_over_after_the_positions(library):
    c = TC.case("two_fams")
    sim, pm = _simulator(c["phys"]), _pm()
    pm.log_prob_and_grad(sim, _z(pm))
    calls = [n for n in library.calls if n.startswith("gl_model_set_pos")]
    assert calls == ["gl_model_set_positions", "gl_model_set_position_delays"]
    pm.log_prob_and_grad(sim, _z(pm))
    pm.term_log_prob_and_grad(sim, _z(pm), "positions")
    assert library.calls.count("gl_model_set_position_delays") == 1 and sim._model.positions_owner is pm
    # a second owner re-binds: new positions, which clear the delays, and its own delays after them
    other = _pm(time_delay_distances=[3000.0, None])
    other.log_prob_and_grad(sim, _z(other))
    assert [n for n in library.calls if n.startswith("gl_model_set_pos")] == ["gl_model_set_positions", "gl_model_set_position_delays"] * 2
    plain = _pm(centroids_time_delays=None, centroids_time_delays_errors=None, time_delay_distances=None)
    plain.log_prob_and_grad(sim, _z(plain))
    assert library.calls.count("gl_model_set_positions") == 3 and library.calls.count("gl_model_set_position_delays") == 2
    # with fluxes and scales of 1: positions, scales, fluxes, delays
    fl = _pm(centroids_fluxes=[np.ones(4, np.float32), None], centroids_fluxes_errors=[0.1, None], centroids_scales=[1.0, 1.0])
    del library.calls[:]
    fl.log_prob_and_grad(sim, _z(fl))
    assert [n for n in library.calls if n.startswith("gl_model_set_pos")] == [
        "gl_model_set_positions", "gl_model_set_position_scales", "gl_model_set_position_fluxes", "gl_model_set_position_delays"]


def test_the_setter_moves_the_generation_and_keeps_the_workspace(library):
    model = _RecordingModel()
    model.n_images, model.n_families = 4, 1
    ws, gen = model._workspace(2), model.generation
    model.prior_owner, model.positions_owner = "p", "q"
    model.set_position_delays([1.0, 2.0, 3.0, np.nan], [1.0] * 4, [np.nan])
    assert model.generation == gen + 1 and model._workspace(2) is ws and (model.prior_owner, model.positions_owner) == ("p", "q")
    model.set_position_delays(None, None, None)
    assert model.generation == gen + 2 and model._workspace(2) is ws
    assert library.calls.count("gl_model_set_position_delays") == 2


def test_binding_refusals_leave_the_native_model_alone(library):
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profile import MassProfile
    from tests.test_user_profile_compile import SIS_BODY
    c = TC.case("two_fams")
    # a family with delays on a scaled plane: predicted_time_delays' NotImplementedError; the scale of a delay-less family is fine
    sim = _simulator(c["phys"])
    scaled = _pm(centroids_scales=[0.9, 1.0])
    with pytest.raises(NotImplementedError, match="scaled source plane"):
        scaled.log_prob_and_grad(sim, _z(scaled))
    assert not [n for n in library.calls if n.startswith("gl_model_set_pos")] and sim._model.positions_owner is None
    ok = _pm(centroids_scales=[1.0, 0.9])
    ok.log_prob_and_grad(sim, _z(ok))
    assert library.calls.count("gl_model_set_position_delays") == 1
    # lens planes
    k2 = PC.case("k2")
    sim_mp = _simulator(k2["phys_mp"])
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import ForwardProbModel
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), 0.01) for k, v in d.items()}) for d in k2["params"]["lens_mass"]])))
    kw = PC.centroids(k2)
    pm_mp = ForwardProbModel(prior, include_pixels=False, **kw, centroids_time_delays=[np.asarray([1.0, 2.0, 4.0], np.float32), None],
                             centroids_time_delays_errors=[1.0, None])
    del library.calls[:]
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        pm_mp.log_prob_and_grad(sim_mp, _z(pm_mp))
    assert not [n for n in library.calls if n.startswith("gl_model_set_pos")]

    # a lens without a potential
    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    sim_u = _simulator(PhysicalModel([UserSIS()], [], []))
    prior_u = J(dict(lens_mass=S([J(dict(theta_E=tfd.Normal(1.0, 0.01), center_x=tfd.Normal(0.0, 0.01), center_y=tfd.Normal(0.0, 0.01)))])))
    pm_u = ForwardProbModel(prior_u, include_pixels=False, **TC.centroids(c))
    with pytest.raises(_native.UnsupportedLensError, match="user-written"):
        pm_u.log_prob_and_grad(sim_u, _z(pm_u))
    assert not [n for n in library.calls if n.startswith("gl_model_set_pos")]
