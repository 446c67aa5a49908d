"""The image-plane position likelihood of image families (csrc/gl_imgplane.hip.h: gl_imgplane_loglike) on the GPU against the float64
restatement of tests/imgplane_cases.py: ``LensSimulator.image_plane_log_like_and_grad`` on the SIS closed form with an explicit
source, on every case (an EPL + shear quad, two families on planes of their own, a dPIS + NFW, a dPIE catalogue), on exact images,
beside the grid-scan solver, with a lost image, at the launch edges, its refusals; ``ImagePlaneProbModel`` alone and joined with a
positions-only ``ForwardProbModel``; one MAP run.

Gates: ``log_like`` / ``chi2`` / ``predicted`` within max(LL_RTOL, 4 x the float32 CPU yardstick) of float64 (``MC.rel_err``); every
gradient element within max(1, 4 x yardstick) units of ``PC.grad_gate``, with 4 x yardstick <= 100 units asserted on the reference
alone (tests/test_imgplane_host.py); two calls bitwise equal.  Every figure is printed before it is asserted.

Measured on an MI355X (in brackets the float32 yardstick): ``epl_shear_quad`` log_like 2.3e-6 (2.1e-5), chi2 1.0e-6 (1.0e-5), predicted
4.6e-7 (6.9e-7), gradient 0.018 gate units (0.031); ``two_planes`` 2.8e-6 (5.5e-6), 2.0e-6 (4.2e-6), 5.4e-7 (4.2e-7), 0.020 (0.021);
``dpis_nfw`` 1.6e-6 (2.3e-6), 2.8e-5 (4.5e-5), 9.3e-7 (1.3e-6), 0.072 (0.149); ``catalogue`` 4.0e-6 (2.2e-5), 1.9e-6 (9.5e-6), 4.9e-7
(1.1e-6), 0.120 (0.107).  Launch edges J B = 63 / 64 / 65 / 129: log_like 1.1e-5 / 8.7e-6 / 1.6e-5 / 8.6e-6 (yardsticks 9.4e-6 / 9.4e-6 /
8.9e-6 / 5.3e-6), gradient 0.034 / 0.029 / 0.034 / 0.031 gate units, grad_source 4.0e-6 at 129.  SIS closed form: predicted 4.6e-8, chi2
1.1e-6, the three gradient elements 1.1e-6, 1.1e-6 and 2.2e-7 of their terms' scale.  Exact images: |predicted - observed| 3.0e-7, chi2
2.2e-10, gradient 0.001 of its bound.  Grid-scan solver: chi2 and J rms^2 differ by 1.3e-7 where the bound is 3.6e-5.  Lost image: chi2
= 302.92 (survivor) + 422.605 (cap) = 725.525 to the last float32 bit, gradient within 6.3e-8 of the survivor's.  MAP: chi2 (5.841,
7.483) -> (0.07005, 0.06645) after 40 steps of 1e-3, the float64 restatement on the CPU (5.841, 7.483) -> (0.07006, 0.06646); the
stated factor is 20."""
import numpy as np
import pytest
import torch

from tests import imgplane_cases as IC
from tests import mp_positions_cases as PC
from tests import multilens_cases as MC
from tests.test_gpu_multilens_grad import _prior_of
from tests.test_gpu_parity import LL_RTOL, gl  # noqa: F401

pytestmark = pytest.mark.gpu
B = IC.B
_SIMS = {}


def _cfg():
    from gigalens_amd.simulator import SimulatorConfig
    return SimulatorConfig(delta_pix=MC.PIX, num_pix=8)  # (the camera plays no part in the position term)


def _sim(gl, phys, bs):
    key = (tuple(type(l).__name__ for l in phys.lenses), bs)
    if key not in _SIMS:
        _SIMS[key] = (gl.LensSimulator(phys, _cfg(), bs=bs), phys)
    sim, held = _SIMS[key]
    assert held is phys  # (the cases are cached: one physical model per lens set)
    return sim


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pred(res):
    """``[2, J, B]`` numpy, the layout of the restatement."""
    return torch.stack([res["predicted_x"].t(), res["predicted_y"].t()]).cpu().numpy()


def _values_against(res, ref, yard, what):
    """Prints and asserts ``log_like``, ``chi2``, ``predicted`` and ``grad`` against the float64 ``ref`` under the yardstick rule."""
    assert res["lost"].cpu().numpy().T.tolist() == ref["lost"].tolist() and res["n_lost"].cpu().tolist() == ref["n_lost"].tolist()
    got = {"log_like": res["log_like"].cpu().numpy(), "chi2": res["chi2"].cpu().numpy(), "predicted": np.nan_to_num(_pred(res))}
    err = {k: MC.rel_err(got[k], np.nan_to_num(ref[k])) for k in got}
    worst = PC.grad_gate(res["grad"].cpu().numpy(), ref["grad"])
    print(f"imgplane {what}: " + ", ".join(f"{k} {err[k]:.2e} (float32 yardstick {yard[k]:.2e})" for k in err) +
          f", gradient worst element {worst:.3f} of the gate (float32 yardstick {yard['grad']:.3f})")
    assert torch.isfinite(res["grad"]).all() and torch.isfinite(res["log_like"]).all()
    for k in err:
        assert err[k] <= max(LL_RTOL, 4 * yard[k]), (what, k, err[k], yard[k])
    assert worst <= max(1.0, 4 * yard["grad"]), (what, worst, yard["grad"])


# ---- 1. the SIS closed form with an explicit source ----------------------------------------------------------------------
def test_sis_closed_form_with_an_explicit_source(gl):
    c = IC.sis_case()
    fams = IC.families(c["fam"])
    sim = _sim(gl, c["phys"], B)
    res = sim.image_plane_log_like_and_grad(torch.as_tensor(c["rows"], device=sim.device), fams, source_x=c["source_x"], source_y=c["source_y"])
    cf = IC.sis_closed_form(fams)
    assert res["n_lost"].tolist() == [0] * B and not res["lost"].any() and res["grad_source_x"].shape == (B, 1)
    for b in range(B):
        pred = _pred(res)[:, :, b]
        e_pred = np.abs(pred - cf["predicted"]).max() / np.abs(cf["predicted"]).max()
        e_chi2 = abs(float(res["chi2"][b]) - cf["chi2"]) / cf["chi2"]
        e_ll = abs(float(res["log_like"][b]) - (-0.5 * cf["chi2"] - fams.norm)) / abs(-0.5 * cf["chi2"] - fams.norm)
        got = np.array([float(res["grad"][b, 0]), float(res["grad_source_x"][b, 0]), float(res["grad_source_y"][b, 0])])
        e_grad = np.abs(got - cf["grad"]) / cf["scale"]
        print(f"SIS sample {b}: predicted {e_pred:.2e}, chi2 {e_chi2:.2e}, log_like {e_ll:.2e}, d/d(theta_E, source_x, source_y) "
              f"{e_grad.tolist()} of the terms' scale ({got.tolist()} against {cf['grad'].tolist()})")
        assert e_pred <= LL_RTOL and e_chi2 <= LL_RTOL and e_ll <= LL_RTOL and np.all(e_grad <= LL_RTOL)


# ---- 2. every case against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IC.CASES)
def test_value_and_gradient_against_float64(gl, name):
    c, fams, ref, yard = IC.data(name)
    sim = _sim(gl, c["phys"], B)
    packed = torch.as_tensor(c["rows"], device=sim.device)
    res = sim.image_plane_log_like_and_grad(packed, fams)
    assert res["log_like"].shape == (B,) and res["chi2"].shape == (B,) and res["n_lost"].shape == (B,)
    assert res["predicted_x"].shape == (B, fams.J) and res["lost"].shape == (B, fams.J) and res["grad"].shape == (B, sim._model.P)
    assert res["grad_source_x"] is None and res["grad_source_y"] is None
    _values_against(res, ref, yard, name)
    again = sim.image_plane_log_like_and_grad(packed, fams)
    for k in ("log_like", "chi2", "n_lost", "predicted_x", "predicted_y", "grad"):
        assert torch.equal(_bits(res[k]), _bits(again[k])), k  # two calls give identical bits
    fwd = sim.image_plane_log_like_and_grad(packed, fams, want_grad=False)
    assert fwd["grad"] is None
    for k in ("log_like", "chi2", "predicted_x", "predicted_y"):
        assert torch.equal(_bits(res[k]), _bits(fwd[k])), k  # the value does not depend on the gradient


# ---- 3. exact images of one source ---------------------------------------------------------------------------------------
def test_exact_images_are_their_own_prediction(gl):
    """The float64 images of the quad's source rounded to float32, at the truth row: predicted == observed to the solver's position gate
    g_j = max(5e-5, 2e-6 |mu_j|) (tests/images_cases.py); chi2 <= sum (g_j/sigma)^2, and every gradient element inside what residuals of
    g_j can make of it -- the float64 gradient's response to a shift of g_j of each observed image along each axis, summed."""
    c = IC.case("epl_shear_quad", B, 0.0)
    fams = IC.families(c["fam"])
    rows = np.repeat(c["truth"][None, :], B, axis=0)
    sim = _sim(gl, c["phys"], B)
    res = sim.image_plane_log_like_and_grad(torch.as_tensor(rows, device=sim.device), fams)
    gate = np.maximum(5e-5, 2e-6 * np.abs(c["truth_images"][0][:, 2]))
    d = np.hypot(_pred(res)[0] - fams.x[:, None], _pred(res)[1] - fams.y[:, None])
    base = IC.loglike_grad(c["phys"], rows[:1], fams, IC.F64)["grad"][0]
    bound = np.abs(base)
    for j in range(fams.J):
        for a in ("x", "y"):
            fam = {k: ([v.copy() for v in val] if k in ("x", "y") else val) for k, val in c["fam"].items()}
            fam[a][0][j] += np.float32(gate[j])
            bound = bound + np.abs(IC.loglike_grad(c["phys"], rows[:1], IC.families(fam), IC.F64)["grad"][0] - base)
    worst = float((np.abs(res["grad"].cpu().numpy()) / bound[None, :]).max())
    print(f"exact images: |predicted - observed| {d.max():.2e} (gate {gate.min():.1e}), chi2 {res['chi2'].tolist()} "
          f"(bound {float(((gate / fams.sigma) ** 2).sum()):.2e}), gradient {worst:.3f} of its bound")
    assert res["n_lost"].tolist() == [0] * B and np.all(d <= gate[:, None])
    assert np.all(res["chi2"].cpu().numpy() <= ((gate / fams.sigma) ** 2).sum()) and worst <= 1.0


# ---- 4. agreement with the grid-scan solver ------------------------------------------------------------------------------
def test_chi2_agrees_with_the_grid_scan_solver(gl):
    """sigma = 1: chi2 = sum |theta_pred - theta_obs|^2 = J rms^2 of ``ForwardProbModel.image_plane_rms`` where the counts match.  Both
    positions lie within g = max(5e-5, 2e-6 |mu|) of the root, so the sums differ by at most sum_j [2 |r_j| 2 g + (2 g)^2]."""
    from gigalens_amd.model import ForwardProbModel
    c, _, ref, _ = IC.data("epl_shear_quad")
    fam = dict(c["fam"], sigma=1.0)
    fams = IC.families(fam)
    sim = _sim(gl, c["phys"], B)
    packed = torch.as_tensor(c["rows"], device=sim.device)
    fpm = ForwardProbModel(_prior_of({"lens_mass": _lens_dicts(c["phys"], c["rows"])}), include_pixels=False, centroids_x=fam["x"], centroids_y=fam["y"],
                           centroids_errors_x=[1.0], centroids_errors_y=[1.0])
    rms = fpm.image_plane_rms(sim, packed, window=(-2.5, 2.5, -2.5, 2.5), num_cells=160)
    res = sim.image_plane_log_like_and_grad(packed, fams, want_grad=False)
    match = rms["counts_match"][:, 0].cpu().numpy()
    want = (fams.J * rms["rms"][:, 0] ** 2).cpu().numpy()
    got = res["chi2"].cpu().numpy()
    g = 5e-5  # (|mu| <= 15 on this quad)
    r = np.hypot(ref["predicted"][0] - fams.x[:, None], ref["predicted"][1] - fams.y[:, None])
    tol = (2 * r * 2 * g + (2 * g) ** 2).sum(axis=0)
    print(f"grid-scan solver: counts match {match.tolist()}, chi2 {got.tolist()} against J rms^2 {want.tolist()} (bound {tol.tolist()})")
    assert match.all() and np.all(np.abs(got - want) <= tol)


# ---- 5. a lost image --------------------------------------------------------------------------------------------------------
def test_lost_image_sits_at_its_cap_and_leaves_the_gradient(gl):
    c = IC.sis_case(b=1.2)  # beyond theta_E: the inner image does not exist
    fams = IC.families(c["fam"])
    sim = _sim(gl, c["phys"], B)
    packed = torch.as_tensor(c["rows"], device=sim.device)
    res = sim.image_plane_log_like_and_grad(packed, fams, source_x=c["source_x"], source_y=c["source_y"])
    ref = IC.loglike_grad(c["phys"], c["rows"], fams, IC.F64, source=IC.sis_source(c))
    assert res["n_lost"].tolist() == [1] * B and res["lost"].tolist() == [[False, True]] * B
    assert torch.isnan(res["predicted_x"][:, 1]).all() and torch.isnan(res["predicted_y"][:, 1]).all()
    assert torch.isfinite(res["predicted_x"][:, 0]).all()
    # chi2 = the survivor's |r|^2/sigma^2 + exactly (cap/sigma)^2 in the kernel's float32 arithmetic, added in float64
    cap, sg = fams.max_shift[1], fams.sigma[1]
    at_cap = np.float32(cap * cap) / np.float32(sg * sg)
    dx = res["predicted_x"][:, 0].cpu().numpy() - fams.x[0]
    dy = res["predicted_y"][:, 0].cpu().numpy() - fams.y[0]
    survivor = np.float32(dx * dx + dy * dy) / np.float32(fams.sigma[0] * fams.sigma[0])
    want = (survivor.astype(np.float64) + np.float64(at_cap)).astype(np.float32)
    print(f"lost image: chi2 {res['chi2'].tolist()}, survivor {survivor.tolist()} + (cap/sigma)^2 {float(at_cap)}")
    assert np.all(np.abs(res["chi2"].cpu().numpy() - want) <= np.spacing(want))  # (the survivor's |r|^2 may contract into an FMA)
    assert torch.isfinite(res["log_like"]).all() and torch.isfinite(res["grad"]).all()
    # the gradient is the survivor's alone
    got = np.concatenate([res["grad"].cpu().numpy(), res["grad_source_x"].cpu().numpy(), res["grad_source_y"].cpu().numpy()], axis=1)
    full = np.concatenate([ref["grad"], ref["grad_source"][0], ref["grad_source"][1]], axis=1)
    e = MC.rel_err(got, full)
    print(f"lost image: chi2 against float64 {MC.rel_err(res['chi2'].cpu().numpy(), ref['chi2']):.2e}, gradient (lens and source) {e:.2e}")
    assert ref["lost"][:, 0].tolist() == [False, True] and MC.rel_err(res["chi2"].cpu().numpy(), ref["chi2"]) <= LL_RTOL and e <= LL_RTOL


# ---- 6. launch edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", IC.EDGES)
def test_launch_edges(gl, cfg):
    d = IC.edge_data(cfg)
    c, fams, ref, yard, source = d["case"], d["fams"], d["ref"], d["yard"], d["source"]
    nb = c["rows"].shape[0]
    sim = _sim(gl, c["phys"], nb)
    packed = torch.as_tensor(c["rows"], device=sim.device)
    kw = {} if source is None else dict(source_x=source[0], source_y=source[1])
    res = sim.image_plane_log_like_and_grad(packed, fams, **kw)
    _values_against(res, ref, yard, f"J B = {cfg} ({fams.F} famil(ies))")
    if source is not None:
        gs = torch.stack([res["grad_source_x"], res["grad_source_y"]]).cpu().numpy()
        e = MC.rel_err(gs, ref["grad_source"])
        print(f"imgplane J B = {cfg}: grad_source {e:.2e} (float32 yardstick {yard['grad_source']:.2e})")
        assert e <= max(LL_RTOL, 4 * yard["grad_source"])
    # a sample's row does not depend on what else is in the batch: the batch reversed gives the same bits, reversed
    flip = sim.image_plane_log_like_and_grad(packed.flip(0).contiguous(), fams, **{k: np.ascontiguousarray(v[::-1]) for k, v in kw.items()})
    keys = ["log_like", "chi2", "n_lost", "predicted_x", "predicted_y", "grad"] + (["grad_source_x", "grad_source_y"] if kw else [])
    for k in keys:
        assert torch.equal(_bits(flip[k].flip(0)), _bits(res[k])), k
    # ... and a sample alone in a batch of one gives the bits it has here
    sim1 = _sim(gl, c["phys"], 1)
    for s in (0, nb - 1):
        one = sim1.image_plane_log_like_and_grad(packed[s:s + 1], fams, **{k: v[s:s + 1] for k, v in kw.items()})
        for k in keys:
            assert torch.equal(_bits(one[k][0]), _bits(res[k][s])), (k, s)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    c, fams, _, _ = IC.data("epl_shear_quad")
    sim = _sim(gl, c["phys"], B)
    packed = torch.as_tensor(c["rows"], device=sim.device)
    with pytest.raises(NotImplementedError, match="no autograd graph"):
        sim.image_plane_log_like_and_grad(packed.clone().requires_grad_(True), fams)
    sx = torch.zeros((B, 1), device=sim.device)
    with pytest.raises(NotImplementedError, match="no autograd graph"):
        sim.image_plane_log_like_and_grad(packed, fams, source_x=sx.clone().requires_grad_(True), source_y=sx)
    with pytest.raises(ValueError, match="both"):
        sim.image_plane_log_like_and_grad(packed, fams, source_x=sx)
    with pytest.raises(ValueError, match="shape"):
        sim.image_plane_log_like_and_grad(packed, fams, source_x=sx[:, :0], source_y=sx[:, :0])
    one = IC.families(dict(x=[c["fam"]["x"][0][:1]], y=[c["fam"]["y"][0][:1]], sigma=0.02, max_shift=0.3))
    with pytest.raises(ValueError, match="no barycentre"):
        sim.image_plane_log_like_and_grad(packed, one)
    sim_p = gl.LensSimulator(PhysicalModel([SIS(), SIS()], [], [], multiplane=MC._mp([0.4, 0.9])), _cfg(), bs=2)
    pp = torch.tensor([[1.0, 0.0, 0.0, 0.5, 0.1, 0.1]] * 2, device=sim_p.device)
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim_p.image_plane_log_like_and_grad(pp, fams)
    with pytest.raises(_native.UnsupportedLensError):  # the native refusal itself
        L = _native.lib()
        tabs = fams.device_tables(sim_p.device)
        out = torch.empty(3 * 2, device=sim_p.device)
        n_lost = torch.empty(2, dtype=torch.int32, device=sim_p.device)
        ws = torch.empty(1 << 16, dtype=torch.uint8, device=sim_p.device)
        _native._check_potential(L.gl_imgplane_loglike(
            sim_p._model._h, pp.data_ptr(), 2, tabs["image"].data_ptr(), tabs["family"].data_ptr(),
            fams.offsets.ctypes.data_as(_native.POINTER(_native.c_int32)), fams.J, fams.F, None, 1e-6, 30, out.data_ptr(),
            out[2:].data_ptr(), n_lost.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), None))
    # a series-expansion lens and a user-written body: the models of the ray-shoot VJP's refusals, its words
    from gigalens_amd import workloads
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.simulator import LensSimulator
    from tests import helpers as H
    from tests.test_gpu_image_positions import _rows, _sim as _point_sim
    from tests.test_user_profile_compile import SIS_BODY
    wl = workloads.make("C6S", num_pix=32, batch=2, n_galaxies=8, n_sources=1)
    sim_s = LensSimulator(wl.phys_model, wl.sim_config, bs=2)
    with pytest.raises(_native.UnsupportedLensError, match="series"):
        sim_s.image_plane_log_like_and_grad(H.sample_packed(wl, sim_s, seed=1), fams)

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    sim_u = _point_sim([UserSIS()], 8, 0.2, 2)
    with pytest.raises(_native.UnsupportedLensError, match="user-written"):
        sim_u.image_plane_log_like_and_grad(_rows(sim_u, np.array([[1.0, 0.0, 0.0]] * 2)), fams)


def test_native_workspace_and_unsupported_lenses(gl):
    from gigalens_amd import _native
    c, fams, _, _ = IC.data("epl_shear_quad")
    sim = _sim(gl, c["phys"], B)
    m, L = sim._model, _native.lib()
    J = fams.J
    fwd, full = L.gl_imgplane_loglike_workspace_bytes(m._h, B, J, 0, 0), L.gl_imgplane_loglike_workspace_bytes(m._h, B, J, 0, 1)
    src = L.gl_imgplane_loglike_workspace_bytes(m._h, B, J, 1, 1)  # explicit sources: J points in the list instead of 2 J
    assert 0 < fwd < full and 0 < src <= full and all(v % 256 == 0 for v in (fwd, src, full))
    assert full >= fwd + 2 * 2 * J * B * 4 + L.gl_lens_maps_vjp_workspace_bytes(m._h, B, 2 * J)
    tabs = fams.device_tables(sim.device)
    packed = torch.as_tensor(c["rows"], device=sim.device)
    ll, chi2, grad = (torch.empty(s, device=sim.device) for s in ((B,), (B,), (B, m.P)))
    n_lost = torch.empty(B, dtype=torch.int32, device=sim.device)
    ws = torch.empty(full, dtype=torch.uint8, device=sim.device)
    p = lambda v: v.data_ptr()
    off = fams.offsets.ctypes.data_as(_native.POINTER(_native.c_int32))
    args = [m._h, p(packed), B, p(tabs["image"]), p(tabs["family"]), off, J, fams.F, None, 1e-6, 30, p(ll), p(chi2), p(n_lost), None]
    assert L.gl_imgplane_loglike(*args, p(grad), None, p(ws), full - 1, None) == -4 and b"workspace too small" in L.gl_last_error()  # GL_ENOMEM
    assert L.gl_imgplane_loglike(*args, None, None, p(ws), fwd - 1, None) == -4
    assert L.gl_imgplane_loglike(*args, None, None, p(ws), fwd, None) == 0
    assert L.gl_imgplane_loglike(*args, p(grad), None, p(ws), full, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(ll).all() and torch.isfinite(grad).all() and n_lost.tolist() == [0] * B


# ---- 8. ImagePlaneProbModel -------------------------------------------------------------------------------------------------
def _lens_dicts(phys, rows):
    out, o = [], 0
    for lens in phys.lenses:
        out.append({k: rows[:, o + i] for i, k in enumerate(lens.params)})
        o += len(lens.params)
    return out


def _prob(gl, strong=False):
    """``(simulator, ImagePlaneProbModel, ForwardProbModel or None, z [B, d], families)`` on the quad; ``strong``: the source-plane
    position term of the same images."""
    from gigalens_amd.model import ForwardProbModel, ImagePlaneProbModel
    c, fams, _, _ = IC.data("epl_shear_quad")
    sim = _sim(gl, c["phys"], B)
    prior = _prior_of({"lens_mass": _lens_dicts(c["phys"], c["rows"])})
    fpm = None
    if strong:
        fpm = ForwardProbModel(prior, include_pixels=False, centroids_x=c["fam"]["x"], centroids_y=c["fam"]["y"],
                               centroids_errors_x=[IC.SIGMA], centroids_errors_y=[IC.SIGMA])
    pm = ImagePlaneProbModel(prior, fams, strong=fpm)
    z = pm.bij.inverse(prior.sample(B, seed=3)).to(pm.device)
    return sim, pm, fpm, z, fams


def _z_gate(g, want):
    return PC.grad_gate(g.double().cpu().numpy(), want.double().cpu().numpy())


def test_prob_model_log_prob_and_gradient(gl):
    sim, pm, _, z, fams = _prob(gl)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    zz = z.clone().requires_grad_(True)
    lp_a, red_a = pm.log_prob(sim, zz)
    (g_a,) = torch.autograd.grad(lp_a.sum(), zz)
    worst = _z_gate(g, g_a)
    print(f"log_prob_and_grad against autograd of log_prob: {worst:.3f} of the gate")
    assert torch.equal(lp, lp_a.detach()) and torch.equal(red, red_a.detach()) and worst <= 1.0
    # the terms: the likelihood at the packed rows of z, the prior, chi2 / (2 J)
    packed = sim._pack_partial(pm.bij.forward(z))
    res = sim.image_plane_log_like_and_grad(packed, fams)
    assert MC.rel_err((res["log_like"] + pm.log_prior(z)).cpu().numpy(), lp.cpu().numpy()) <= LL_RTOL
    assert torch.equal(red, res["chi2"] / (2.0 * fams.J))
    # the chain rule through the bijector: d log_prob / d z from the native gradient on the packed rows
    zz = z.clone().requires_grad_(True)
    pk = sim._pack_partial(pm.bij.forward(zz))
    (g_chain,) = torch.autograd.grad((pk * res["grad"]).sum() + pm.log_prior(zz).sum(), zz)
    worst = _z_gate(g, g_chain)
    print(f"gradient against the chain rule on the native packed gradient: {worst:.3f} of the gate")
    assert worst <= 1.0 and pm.n_position == 2.0 * fams.J and pm.include_positions and not pm.include_pixels


def test_prob_model_joined_with_the_source_plane_term(gl):
    sim, pm, fpm, z, fams = _prob(gl, strong=True)
    _, alone, _, _, _ = _prob(gl)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    lp_i, red_i, g_i = alone.log_prob_and_grad(sim, z)
    lp_s, red_s, g_s = fpm.log_prob_and_grad(sim, z)
    zz = z.clone().requires_grad_(True)
    prior = alone.log_prior(zz)
    (g_p,) = torch.autograd.grad(prior.sum(), zz)
    want_lp, want_g = lp_i - prior.detach() + lp_s, g_i - g_p + g_s  # one prior
    e_lp, worst = MC.rel_err(lp.cpu().numpy(), want_lp.cpu().numpy()), _z_gate(g, want_g)
    n_img, n_strong = 2.0 * fams.J, float(fpm._n_eff(sim))
    want_red = (red_i * n_img + red_s * n_strong) / (n_img + n_strong)
    e_red = MC.rel_err(red.cpu().numpy(), want_red.cpu().numpy())
    print(f"joint log_prob {e_lp:.2e}, gradient {worst:.3f} of the gate, reduced chi2 {e_red:.2e}")
    assert torch.isfinite(lp).all() and e_lp <= LL_RTOL and worst <= 1.0 and e_red <= LL_RTOL
    assert pm.n_position == n_img + fpm.n_position and pm.include_positions and not pm.include_pixels


def test_map_shrinks_chi2_as_the_float64_restatement_does(gl):
    """The noise-free quad, IC.MAP_BS samples that start with theta_E 2 % high: after IC.MAP_STEPS Adam steps of IC.MAP_LR the float64
    restatement under the same Adam on the CPU has shrunk chi2 by more than IC.MAP_FACTOR in every sample, and so has the GPU run.  A
    plumbing check, not a convergence study."""
    from gigalens_amd import prior as tfd
    from gigalens_amd.inference import Adam, ModellingSequence
    from gigalens_amd.model import ImagePlaneProbModel
    m = IC.map_case()
    first, last = IC.map_reference()
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    mu = dict(zip(m["names"], m["truth"].tolist()))
    dist = lambda k: tfd.LogNormal(float(np.log(mu[k])), IC.MAP_PRIOR[k]) if k == "theta_E" else tfd.Normal(mu[k], IC.MAP_PRIOR[k])
    prior = J({"lens_mass": S([J({k: dist(k) for k in lens.params}) for lens in m["phys"].lenses])})
    pm = ImagePlaneProbModel(prior, m["fams"])
    start = {"lens_mass": [{k: torch.as_tensor(v) for k, v in d.items()} for d in _lens_dicts(m["phys"], m["start"])]}
    z = ModellingSequence(m["phys"], pm, _cfg()).MAP(Adam(lr=IC.MAP_LR), start=start, n_samples=IC.MAP_BS, num_steps=IC.MAP_STEPS, graph=False)
    sim = _sim(gl, m["phys"], IC.MAP_BS)
    res0 = sim.image_plane_log_like_and_grad(torch.as_tensor(m["start"], device=sim.device), m["fams"], want_grad=False)
    _, red = pm.log_prob(sim, z)
    chi2_0, chi2_1 = res0["chi2"].cpu().numpy(), (red * 2.0 * m["fams"].J).detach().cpu().numpy()
    print(f"MAP on the image plane: chi2 {chi2_0.tolist()} -> {chi2_1.tolist()} (factor {(chi2_0 / chi2_1).tolist()}) after {IC.MAP_STEPS} "
          f"steps of {IC.MAP_LR}; float64 on the CPU: {first.tolist()} -> {last.tolist()} (factor {(first / last).tolist()})")
    assert np.all(first / last >= IC.MAP_FACTOR)
    assert MC.rel_err(chi2_0, first) <= 1e-4 and np.all(chi2_0 / chi2_1 >= IC.MAP_FACTOR)
