"""The time-delay likelihood on lens planes without a GPU: the float64 restatement of tests/mp_tdelay_like_cases.py against
``mp_tdelay_cases.reference_T``, the yardstick of the GPU test (the kernel's double arithmetic compiled with g++) under its ceiling
and under ``2^-24``, the convergence of the central differences the gradient is gated against, the physics pin of the restatement
(an empty second plane: the single-plane term of tests/tdelay_cases.py), the ``time_delay_h0`` keyword, the C ABI and the binding to
the native model (the recording library of tests/test_model_binding_host.py)."""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from gigalens_amd import _native
from tests import mp_positions_cases as PC
from tests import mp_tdelay_like_cases as LC
from tests import multilens_cases as MC
from tests import tdelay_cases as TC
from tests.test_model_binding_host import B, N_PIX, _RecordingModel, _z, library  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement and its yardstick ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.CASES)
def test_composed_sum_is_reference_T(name):
    """``composed_T`` (float64 rows, for the central differences) against ``mp_tdelay_cases.reference_T`` at the rows of the case."""
    c, ref, _ = LC.data(name)
    err = LC.errors(LC.values(c, how="reference"), [ref[k] for k in LC.QUANTITIES])
    print(f"{name}: composed sum against reference_T " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert max(err.values()) <= 1e-13


@pytest.mark.parametrize("name", LC.CASES)
def test_yardsticks_stay_under_their_ceiling_and_under_float32_rounding(name):
    c, ref, yard = LC.data(name)
    print(f"{name}: host-build yardsticks " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    assert np.isfinite(ref["log_like"]).all() and LC.n_delay(c) >= 3
    for k, v in yard.items():
        assert v <= LC.YARD_CEILING[k] and v < LC.EPS32, (k, v)
        assert LC.value_gate(v) == 8 * LC.EPS32  # (the gate of the GPU test is the float32 rounding of the results)


@pytest.mark.parametrize("name", LC.CASES)
def test_central_differences_have_converged(name):
    """``h`` and ``h / 2`` agree to 1e-3 of the gradient gate (``mp_positions_cases.grad_gate``: 5e-4 scale + 1e-6; the cancelled
    columns of ``LC.CANCELLED``: of their gate at the row's scale)."""
    c = LC.case(name)
    g, g2 = LC.grad(name), LC.gradient(c, halve=2.0)
    u, u_row = LC.gate_units(name, c, g2, g)
    print(f"{name}: h against h / 2, worst element {u:.2e} of the gate (cancelled columns {u_row:.2e} of theirs); largest gradient "
          f"element {np.abs(g).max():.3g}")
    assert np.isfinite(g).all() and np.abs(g).max() > 0 and u <= 1e-3 and u_row <= 1e-3
    if not LC.cancelled_columns(name, c).any():
        assert u == PC.grad_gate(g2, g)


def test_the_cancelled_columns_cancel_and_the_smooth_psi_is_the_host_psi():
    """``zoo_b``: in the Shear columns the direct part and the part through the source cancel to 1e-6 of either, element by element, and every other column
    holds a gradient of its own; the line-integral psi of the TNFW gives the values of the host psi to 1e-9, on paths that keep
    ``tdelay_cases.MIN_CENTRE`` from the TNFW's centre."""
    name = "zoo_b"
    c = LC.case(name)
    ex = LC.cancelled_columns(name, c)
    cols = np.flatnonzero(ex)
    g = LC.grad(name)
    direct = LC.gradient(c, cols=cols, direct=True)
    ratio = (np.abs(g[:, ex]) / np.abs(direct[:, ex])).max()
    print(f"{name}: cancelled columns {cols.tolist()}: total {np.abs(g[:, ex]).max():.2e}, direct part {np.abs(direct[:, ex]).min():.3g} "
          f"... {np.abs(direct[:, ex]).max():.3g}, ratio {ratio:.1e}")
    assert ex.sum() == 2 and ratio <= 1e-6 and np.all(np.abs(direct[:, ex]).max(axis=0) <= np.abs(g).max())
    assert np.all(np.abs(g[:, ~ex]).max(axis=0) > 1e-3 * np.abs(g).max(axis=0).min() + 1.0)
    err = LC.errors(LC.values(c, smooth=True), LC.values(c))
    print(f"{name}: line-integral psi of the TNFW against the host psi " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert max(err.values()) <= 1e-9
    d = LC.smooth_min_centre(c)
    print(f"{name}: the TNFW's paths keep {d:.3f} arcsec from its centre")
    assert d >= TC.MIN_CENTRE


def test_case_shapes_and_masks():
    """Every path of the kernels has a case: K_f < K, a column behind a family, an unmeasured image, a delay-less family, B = 65."""
    assert all(np.count_nonzero(fm["T"]) < LC.case("front")["mp"].K for fm in LC.case("front")["fams"])
    for name in ("k2", "k3", "k4", "zoo_a", "zoo_b"):
        c = LC.case(name)
        n_front = [np.count_nonzero(fm["T"]) for fm in c["fams"]]
        assert min(n_front) < c["mp"].K == max(n_front), name
    assert LC.case("k4")["mp"].K == 4 and LC.case("k3")["mp"].K == 3 and LC.case("k2_b65")["B"] == 65
    assert LC.n_delay(LC.case("k2_nan")) == 6 and LC.n_delay(LC.case("k2_two")) == 3 == LC.n_delay(LC.case("k2_one"))
    assert [np.isnan(fm["h0"]) for fm in LC.case("k2_mixed")["fams"]] == [True, False]
    assert not any(np.isnan(fm["h0"]) for fm in LC.case("k2_given")["fams"])
    kinds = {type(lens).__name__ for name in ("zoo_a", "zoo_b") for lens, pl in
             zip(LC.case(name)["phys"].lenses, LC.case(name)["mp"].plane_of_lens) if pl > 0}
    assert kinds == {"EPL", "Shear", "NFW", "DPIS", "DPIE", "SIS", "TNFW", "NFW_ELLIPSE", "DPIEP", "SIE"}, kinds
    # the delay-less family adds exactly nothing, and columns of lenses at or behind every family with delays are exactly zero
    _, two, _ = LC.data("k2_two")
    _, one, _ = LC.data("k2_one")
    assert np.array_equal(two["log_like"], one["log_like"]) and np.array_equal(two["chi2"], one["chi2"])
    assert np.isnan(two["scale"][:, 1]).all() and np.isnan(two["model"][:, 3:]).all()
    g = LC.grad("k2_two")
    behind = LC.behind_columns(LC.case("k2_two"))
    assert behind.any() and np.all(g[:, behind] == 0.0) and np.all(np.abs(g[:, ~behind]).max(axis=0) > 0)
    assert np.array_equal(g, LC.grad("k2_one"))


# ---- the physics pin: an empty second plane is the single-plane term ------------------------------------------------------------
PIN_SOURCE = (0.01, -0.008)  # arcsec off the centre of the SIE (theta_E = 0.4): inside its astroid caustic, four images
PIN_WINDOW, PIN_CELLS = (-3.0, 3.0, -3.0, 3.0), 96
# the two forms agree to first order in beta_j - mean beta and differ at second order; with solved images rounded to float32
# |beta_j - mean beta| is 3e-8 and its square is below double rounding.  Measured on the CPU when the case was fixed: log_like
# 7.5e-16, chi2 1.5e-13, the model delays 5.6e-15 (relative to their largest value), the gradient columns of the plane-1 lenses
# 7.7e-4 of the gate (the single-plane reference is autograd through the line integral of the oracle's deflection, this one central
# differences through the host build of the potential templates); lambda_multi g_1 / lambda_single - 1 = 3.1e-15
PIN_MEASURED = dict(log_like=7.5e-16, chi2=1.5e-13, model=5.6e-15, grad=7.7e-4)


@functools.lru_cache(maxsize=None)
def _pin():
    """``(multi-plane case, single-plane case, g_1)``: SIE + Shear on plane 1, a zero-strength SIS alone on plane 2 (sample 0 of
    ``mp_positions_cases.case('empty')``), one family at ``z_ref`` -- coupling 1 -- whose positions are the float64 images of one source,
    Newton-polished as ``mp_tdelay_cases.polished_images`` does and rounded to float32."""
    from gigalens_amd.cosmology import comoving_distance
    from oracle import ref_torch as ref
    from tests import images_cases as IC
    e = PC.case("empty")
    phys, mp = e["phys"], e["mp"]
    lp0 = [{k: np.asarray(v, np.float32)[:1] for k, v in d.items()} for d in e["params"]["lens_mass"]]
    lp64 = MC._tensors({"lens_mass": lp0}, MC.F64)["lens_mass"]
    consts = MC._consts(phys, MC.F64)

    def deriv(x, y):  # the family's coupling to plane 1 is 1 and plane 2 deflects nothing: alpha of the lenses on plane 1
        ax = ay = 0
        for l, lens in enumerate(phys.lenses):
            if int(mp.plane_of_lens[l]) == 0:
                fx, fy = ref.mass_deriv(lens, x, y, **{k: v[0] for k, v in lp64[l].items()}, **consts[l])
                ax, ay = ax + fx, ay + fy
        return ax, ay
    sx = float(lp0[0]["center_x"][0]) + PIN_SOURCE[0]
    sy = float(lp0[0]["center_y"][0]) + PIN_SOURCE[1]
    img = IC._solve64(deriv, sx, sy, PIN_WINDOW, PIN_CELLS)
    x, y = torch.as_tensor(img[:, 0].copy()), torch.as_tensor(img[:, 1].copy())
    for _ in range(8):
        bx, by, fxx, fxy, fyx, fyy = IC._beta_jac(deriv, x, y)
        rx, ry = sx - bx, sy - by
        if float(torch.hypot(rx, ry).max()) <= 1e-12:
            break
        a00, a01, a10, a11 = 1 - fxx, -fxy, -fyx, 1 - fyy
        det = a00 * a11 - a01 * a10
        x, y = x + (a11 * rx - a01 * ry) / det, y + (a00 * ry - a10 * rx) / det
    assert np.all(IC._residual64(deriv, x.numpy(), y.numpy(), sx, sy) <= 1e-12) and x.numel() == 4
    x32, y32 = x.numpy().astype(np.float32), y.numpy().astype(np.float32)
    fam = dict(z=float(mp.z_ref), T=np.asarray(mp.target_scales(mp.z_ref), dtype=np.float64), x=x32, y=y32,
               ex=np.full(4, 0.01, np.float32), ey=np.full(4, 0.0125, np.float32))
    assert np.all(np.float32(fam["T"]) == 1.0)
    params = dict(e["params"], lens_mass=lp0)
    cm = dict(phys=phys, phys_mp=e["phys_mp"], mp=mp, params=params, B=1, fams=[fam], lens_cols=10)
    cm = dict(cm, fams=LC.with_delays(cm))
    # the single-plane twin: the same lenses on one plane, the same times, lambda_single = lambda_multi g_1
    c1, cs = float(comoving_distance(mp.z_planes[0], mp.omega_m)), float(comoving_distance(mp.z_ref, mp.omega_m))
    g1 = c1 * cs / (cs - c1)
    mp1 = MC._mp([float(mp.z_planes[0])] * len(phys.lenses))
    f1 = dict(fam, T=np.ones(1), delay=cm["fams"][0]["delay"], delay_err=cm["fams"][0]["delay_err"], scale=np.nan)
    cs1 = dict(phys=e["phys_1"], mp=mp1, params=params, B=1, fams=[f1], lens_cols=10, catalogue=None)
    return cm, cs1, g1


def test_empty_second_plane_is_the_single_plane_term():
    cm, c1, g1 = _pin()
    ll, chi2, lam, off, model = LC.values(cm)
    g = LC.gradient(cm)
    ll1, chi21, grad1, lam1, off1, model1 = TC.loglike_grad(c1)
    shared = slice(0, 7)  # the columns of the SIE and the Shear on plane 1
    figures = dict(log_like=MC.rel_err(ll, ll1), chi2=MC.rel_err(chi2, chi21), model=MC.rel_err(model, model1),
                   grad=PC.grad_gate(g[:, shared], grad1[:, shared]))
    lam_err = abs(float(lam[0, 0]) * g1 / float(lam1[0, 0]) - 1.0)
    print("empty second plane against the single-plane term: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items())
          + f"; lambda_multi g_1 / lambda_single - 1 = {lam_err:.2e}; fitted H0 = {LC.h0_of(lam[0, 0]):.3f}")
    for k, v in figures.items():
        assert v <= 10 * PIN_MEASURED[k], (k, v)
    assert lam_err <= 10 * 3.1e-15


# ---- the keyword -------------------------------------------------------------------------------------------------------
def _prior(c):
    from gigalens_amd import prior as tfd
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    return J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), 0.01) for k, v in d.items()}) for d in c["params"]["lens_mass"]])))


def _pm(name="k2", **kw):
    from gigalens_amd.model import ForwardProbModel
    c = LC.case(name)
    args = dict(LC.centroids(c), include_pixels=False)
    args.update(kw)
    return ForwardProbModel(_prior(c), **args)


def test_constructor_takes_time_delay_h0():
    pm = _pm()
    assert pm.n_delay == 7.0 and np.isnan(pm.time_delay_h0).all() and np.isnan(pm.time_delay_distances).all()
    assert _pm(time_delay_h0="profile").time_delay_h0.tolist() != [] and np.isnan(_pm(time_delay_h0="profile").time_delay_h0).all()
    assert _pm(time_delay_h0=70.0).time_delay_h0.tolist() == [70.0, 70.0]
    mixed = _pm(time_delay_h0=[None, 67.0]).time_delay_h0
    assert np.isnan(mixed[0]) and mixed[1] == 67.0
    assert _pm(time_delay_h0=np.asarray([70.0, 71.0])).time_delay_h0.tolist() == [70.0, 71.0]
    # two measured times are a constraint once H0 is given
    nan = np.float32(np.nan)
    t = [np.asarray([1.0, 4.0, nan], np.float32), None]
    assert _pm(centroids_time_delays=t, centroids_time_delays_errors=[1.0, None], time_delay_h0=[70.0, None]).n_delay == 2.0
    # without the keyword the model is what it was
    plain = _pm(time_delay_h0=None)
    assert plain.time_delay_h0 is None and plain.n_delay == 7.0
    with pytest.raises(ValueError, match="needs a model built with time_delay_h0"):
        plain.fitted_h0(None, None)


def test_constructor_refusals():
    nan = np.float32(np.nan)
    two = [np.asarray([1.0, 4.0, nan], np.float32), None]
    bad = [
        (dict(time_delay_distances=[3000.0, None]), "give one"),
        (dict(centroids_time_delays=None, centroids_time_delays_errors=None), "needs centroids_time_delays"),
        (dict(centroids_redshifts=None), "needs centroids_redshifts"),
        (dict(time_delay_h0=[70.0]), "one entry per image family"),
        (dict(time_delay_h0=[70.0, 70.0, 70.0]), "one entry per image family"),
        (dict(time_delay_h0=0.0), "finite and > 0"),
        (dict(time_delay_h0=-70.0), "finite and > 0"),
        (dict(time_delay_h0=[np.inf, None]), "finite and > 0"),
        (dict(time_delay_h0=[np.nan, 70.0]), "finite and > 0"),
        (dict(time_delay_h0="fit"), "'profile'"),
        (dict(centroids_time_delays=two, centroids_time_delays_errors=[1.0, None]), "two measured arrival times with a profiled"),
        (dict(centroids_time_delays=two, centroids_time_delays_errors=[1.0, None], time_delay_h0=[None, 70.0]), "give time_delay_h0"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            _pm(**kw)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "gigalens_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("gl_model_set_position_plane_delays", 9), ("gl_multiplane_position_delays_fwd_bwd", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_native.SYMBOLS[name][1])
    assert "gl_multiplane_tdelays.hip.h" in open(os.path.join(ROOT, "gigalens_amd", "csrc", "gl_api_points.hip")).read()


# ---- the binding -------------------------------------------------------------------------------------------------------
def _simulator(phys):
    region = torch.ones(N_PIX, N_PIX)
    return types.SimpleNamespace(_model=_RecordingModel(), _layout=phys._packing(), phys_model=phys, img_region=region,
                                 sim_config=types.SimpleNamespace(pix_region=None), _mp=phys.multiplane, _n_eff=None,
                                 _linear_cols_dev=None, _lp_graphs={}, _lp_captures=0)


def _set_calls(library):
    return [n for n in library.calls if n.startswith("gl_model_set_pos")]


def test_plane_delays_are_handed_over_last(library):
    c = LC.case("k2")
    sim, pm = _simulator(c["phys_mp"]), _pm()
    pm.log_prob_and_grad(sim, _z(pm))
    assert _set_calls(library) == ["gl_model_set_positions", "gl_model_set_position_targets", "gl_model_set_position_plane_delays"]
    assert sim._model.fused[-1][0] == "multiplane_logprob"
    pm.log_prob_and_grad(sim, _z(pm))
    pm.term_log_prob_and_grad(sim, _z(pm), "positions")
    assert library.calls.count("gl_model_set_position_plane_delays") == 1 and sim._model.positions_owner is pm
    # with fluxes: positions, targets, fluxes, plane delays
    fl = _pm(centroids_fluxes=[np.ones(3, np.float32), None], centroids_fluxes_errors=[0.1, None])
    del library.calls[:]
    fl.log_prob_and_grad(sim, _z(fl))
    assert _set_calls(library) == ["gl_model_set_positions", "gl_model_set_position_targets", "gl_model_set_position_fluxes",
                                   "gl_model_set_position_plane_delays"]
    # a positions-only owner after it: new positions (which clear the delays), nothing else of the delays
    plain = _pm(centroids_time_delays=None, centroids_time_delays_errors=None, time_delay_h0=None)
    del library.calls[:]
    plain.log_prob_and_grad(sim, _z(plain))
    assert _set_calls(library) == ["gl_model_set_positions", "gl_model_set_position_targets"]


def test_the_tables_come_from_delay_weights():
    c = LC.case("k2_mixed")
    pm = _pm("k2_mixed")
    sim = types.SimpleNamespace(_mp=c["mp"], phys_model=c["phys_mp"])
    geom, pot, lam = pm._plane_delay_tables(sim, pm.position_targets(c["mp"]))
    g_ref, v_ref = LC.family_weights(c)
    assert np.array_equal(geom, g_ref) and np.array_equal(pot, v_ref) and lam.dtype == np.float32
    assert np.isnan(lam[0]) and lam[1] == np.float32(LC.lambda_of(67.0))
    assert np.array_equal(geom != 0.0, pm.position_targets(c["mp"]) != 0.0)
    # pot is that of the farthest family WITH delays
    c2, pm2 = LC.case("k2_two"), _pm("k2_two")
    _, pot2, _ = pm2._plane_delay_tables(types.SimpleNamespace(_mp=c2["mp"], phys_model=c2["phys_mp"]), pm2.position_targets(c2["mp"]))
    assert np.array_equal(pot2, c2["mp"].delay_weights(c2["fams"][0]["z"])[1])


def test_the_setter_moves_the_generation_and_drops_the_workspaces(library):
    model = _RecordingModel()
    model.n_images, model.n_families = 4, 1
    ws, gen = model._workspace(2), model.generation
    model.prior_owner, model.positions_owner = "p", "q"
    model.set_position_plane_delays([1.0, 2.0, 3.0, np.nan], [1.0] * 4, np.ones((1, 2)), np.ones(2), [np.nan])
    assert model.generation == gen + 1 and model._workspace(2) is not ws and (model.prior_owner, model.positions_owner) == ("p", "q")
    model.set_position_plane_delays(None, None, None, None, None)
    assert model.generation == gen + 2 and library.calls.count("gl_model_set_position_plane_delays") == 2
    with pytest.raises(_native.NativeLibraryError, match="geom must be"):
        model.set_position_plane_delays([1.0, 2.0, 3.0, np.nan], [1.0] * 4, np.ones((2, 2)), np.ones(2), [np.nan])


def test_binding_refusals_leave_the_native_model_alone(library):
    from gigalens_amd.model import ForwardProbModel, PhysicalModel
    c = LC.case("k2")
    # without time_delay_h0 a model with delays is refused on planes as before (the text existing tests pin), now with a pointer
    old = _pm(time_delay_h0=None)
    sim = _simulator(c["phys_mp"])
    with pytest.raises(_native.UnsupportedLensError, match="lens planes.*time_delay_h0"):
        old.log_prob_and_grad(sim, _z(old))
    assert not _set_calls(library) and sim._model.positions_owner is None
    # time_delay_h0 on a simulator without several planes -- a one-plane MultiPlane included -- points to time_delay_distances
    pm = _pm()
    for phys in (c["phys"], PhysicalModel(c["phys"].lenses, [], [], multiplane=MC._mp([0.5] * len(c["phys"].lenses)))):
        sim1 = _simulator(phys)
        assert sim1._mp is None
        for call in (lambda: pm.log_prob_and_grad(sim1, _z(pm)), lambda: pm.stats_time_delays(sim1, torch.zeros(B, 13)),
                     lambda: pm.fitted_h0(sim1, torch.zeros(B, 13))):
            with pytest.raises(ValueError, match="time_delay_distances"):
                call()
        assert not _set_calls(library) and sim1._model.positions_owner is None
    # a family at or in front of the first plane: the ValueError of the targets, before anything is handed over
    far = _pm(centroids_redshifts=[0.2, 2.0])
    with pytest.raises(ValueError):
        far.log_prob_and_grad(sim, _z(far))
    assert not _set_calls(library)

    # a lens without a potential
    from gigalens_amd.profile import MassProfile
    from tests.test_user_profile_compile import SIS_BODY

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    from gigalens_amd import prior as tfd
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    lenses = [UserSIS(), UserSIS()]
    sim_u = _simulator(PhysicalModel(lenses, [], []))
    sim_u._mp = MC._mp([0.5, 1.0])  # (the refusal under test comes before any plane is looked at by the library)
    sis = lambda: J(dict(theta_E=tfd.Normal(1.0, 0.01), center_x=tfd.Normal(0.0, 0.01), center_y=tfd.Normal(0.0, 0.01)))
    pm_u = ForwardProbModel(J(dict(lens_mass=S([sis(), sis()]))), include_pixels=False, **LC.centroids(c))
    with pytest.raises(_native.UnsupportedLensError, match="user-written"):
        pm_u.log_prob_and_grad(sim_u, _z(pm_u))
    assert not _set_calls(library)
