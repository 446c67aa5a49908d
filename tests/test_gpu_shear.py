"""The weak-lensing reduced-shear likelihood (csrc/gl_hessian_vjp.hip.h: gl_shear_loglike) on the GPU against ``torch.autograd`` on
the float64 restatement (tests/shear_cases.py): ``LensSimulator.shear_log_like_and_grad`` / ``reduced_shear`` on galaxies of both
branches of g^, with per-galaxy deflection scales, on a dPIS (the convergence excess) and on a cluster (a wide NFW halo and a dPIE
catalogue); ``WeakLensingProbModel`` alone and joined with a positions-only ``ForwardProbModel``; one MAP run.

Gates: ``log_like`` / ``chi2`` / ``model_g`` within max(LL_RTOL, 4 x the float32 CPU yardstick) of float64 (``MC.rel_err``); every
gradient element within max(1, 4 x yardstick) units of ``PC.grad_gate``, with 4 x yardstick <= 100 units asserted on the reference
alone; two calls bitwise equal.  Every figure is printed before it is asserted.

Measured on an MI355X: values within 5e-7 and gradients within 0.01 gate units for ``epl_shear|sie`` and ``dpis|sie`` at every N; the
``cluster`` case (Rs = 18 .. 22 arcsec, galaxies down to 0.03 Rs at N = 64 / 65) has values within 7e-5 and gradients at 9.8 / 10.0
gate units for N = 64 / 65 -- the float32 restatement sits at 9.4 / 9.6 there, the gate at 4 x that -- and 0.46 at N = 4161.  The MAP
run takes theta_E from 1.44 to 1.1999 (truth 1.2) in MAP_STEPS = 150 Adam steps of 1e-2."""
import numpy as np
import pytest
import torch

from tests import flux_cases as FC
from tests import mp_positions_cases as PC
from tests import multilens_cases as MC
from tests import shear_cases as SC
from tests.test_gpu_multilens_grad import _prior_of
from tests.test_gpu_parity import LL_RTOL, gl  # noqa: F401

pytestmark = pytest.mark.gpu
B = SC.B
_SIMS = {}


def _cfg():
    from gigalens_amd.simulator import SimulatorConfig
    return SimulatorConfig(delta_pix=MC.PIX, num_pix=8)  # (the camera plays no part in the shear term)


def _bound(gl, name, bs=B):
    """``(case, simulator, packed rows [bs, P])`` -- one simulator per (case, batch size)."""
    c = SC.ll_case(name)
    if (name, bs) not in _SIMS:
        _SIMS[name, bs] = gl.LensSimulator(c["phys"], _cfg(), bs=bs)
    sim = _SIMS[name, bs]
    return c, sim, torch.as_tensor(c["rows"][:bs], device=sim.device)


def _cat(cat, scales=True):
    from gigalens_amd.model import ShearCatalogue
    return ShearCatalogue(cat["x"], cat["y"], cat["e1"], cat["e2"], cat["sigma"], scales=cat["scales"] if scales else None)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", SC.N_GAL)
@pytest.mark.parametrize("name", SC.LL_CASES)
def test_value_and_gradient_against_float64(gl, name, n):
    c, cat, ref, yard = SC.ll_data(name, n)
    _, sim, packed = _bound(gl, name)
    assert 4 * yard["grad"] <= SC.GATE_CAP, (name, n, yard)  # the case, not the cap, is what changes if this fails
    res = sim.shear_log_like_and_grad(packed, _cat(cat))
    assert res["log_like"].shape == (B,) and res["chi2"].shape == (B,) and res["model_g"].shape == (2, n, B)
    assert res["grad"].shape == (B, sim._model.P) and all(v.dtype == torch.float32 for v in res.values())
    assert torch.isfinite(res["grad"]).all()
    err = {k: MC.rel_err(res[k].cpu().numpy(), ref[k]) for k in ("log_like", "chi2", "model_g")}
    worst = PC.grad_gate(res["grad"].cpu().numpy(), ref["grad"])
    print(f"shear {name} N={n}: " + ", ".join(f"{k} {err[k]:.2e} (float32 yardstick {yard[k]:.2e})" for k in err) +
          f", gradient worst element {worst:.3f} of the gate (float32 yardstick {yard['grad']:.3f})")
    for k in err:
        assert err[k] <= max(LL_RTOL, 4 * yard[k]), (name, n, k, err[k], yard[k])
    assert worst <= max(1.0, 4 * yard["grad"]), (name, n, worst, yard["grad"])


def test_value_does_not_depend_on_the_gradient_and_calls_repeat(gl):
    c, cat, _, _ = SC.ll_data("epl_shear|sie", 4161)
    _, sim, packed = _bound(gl, "epl_shear|sie")
    sc = _cat(cat)
    a = sim.shear_log_like_and_grad(packed, sc)
    b = sim.shear_log_like_and_grad(packed, sc)
    for k in ("log_like", "chi2", "model_g", "grad"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k  # two calls give identical bits
    f = sim.shear_log_like_and_grad(packed, sc, want_grad=False)
    assert f["grad"] is None
    for k in ("log_like", "chi2", "model_g"):
        assert torch.equal(_bits(a[k]), _bits(f[k])), k
    _, sim1, _ = _bound(gl, "epl_shear|sie", 1)
    for s in range(B):  # a sample alone gives the bits it has in its batch
        one = sim1.shear_log_like_and_grad(packed[s:s + 1], sc)
        assert torch.equal(_bits(one["log_like"][0]), _bits(a["log_like"][s])) and torch.equal(_bits(one["chi2"][0]), _bits(a["chi2"][s]))
        assert torch.equal(_bits(one["grad"][0]), _bits(a["grad"][s])) and torch.equal(_bits(one["model_g"][:, :, 0]), _bits(a["model_g"][:, :, s]))


def test_scales_of_one_and_reduced_shear(gl):
    c, cat, _, _ = SC.ll_data("dpis|sie", 65)
    _, sim, packed = _bound(gl, "dpis|sie")
    ones = dict(cat, scales=np.ones_like(cat["scales"]))
    a = sim.shear_log_like_and_grad(packed, _cat(cat, scales=False))
    b = sim.shear_log_like_and_grad(packed, _cat(ones))
    for k in ("log_like", "chi2", "model_g", "grad"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k  # no scales = scales of one, bit for bit
    # reduced_shear: the same g^ from the Hessian maps with torch operations (the kernel contracts some of them into FMAs)
    x, y = torch.as_tensor(cat["x"], device=sim.device)[:, None], torch.as_tensor(cat["y"], device=sim.device)[:, None]
    for scale, res in ((1.0, a), (0.7, sim.shear_log_like_and_grad(packed, _cat(dict(cat, scales=np.float32(0.7)))))):
        g1, g2 = sim.reduced_shear(x, y, packed, deflection_scale=scale)
        assert g1.shape == (65, B)
        e = MC.rel_err(torch.stack([g1, g2]).cpu().numpy(), res["model_g"].cpu().numpy())
        print(f"reduced_shear against model_g, scale {scale}: {e:.2e}")
        assert e <= LL_RTOL
    assert bool((a["model_g"] ** 2).sum(dim=0).max() <= 1.0 + 1e-6)  # |g^| <= 1 on either branch


def test_chi2_does_not_depend_on_the_order_of_the_galaxies(gl):
    c, cat, ref, _ = SC.ll_data("epl_shear|sie", 4161)
    _, sim, packed = _bound(gl, "epl_shear|sie")
    a = sim.shear_log_like_and_grad(packed, _cat(cat))
    b = sim.shear_log_like_and_grad(packed, _cat(SC.permuted(cat)))
    e_chi2, e_ll = MC.rel_err(b["chi2"].cpu().numpy(), a["chi2"].cpu().numpy()), MC.rel_err(b["log_like"].cpu().numpy(), a["log_like"].cpu().numpy())
    worst = PC.grad_gate(b["grad"].cpu().numpy(), ref["grad"])
    print(f"permuted catalogue: chi2 {e_chi2:.2e}, log_like {e_ll:.2e}, gradient {worst:.3f} of the gate against float64")
    assert e_chi2 <= LL_RTOL and e_ll <= LL_RTOL and worst <= 1.0


def test_native_workspace_and_refusals(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    c, cat, _, _ = SC.ll_data("epl_shear|sie", 65)
    _, sim, packed = _bound(gl, "epl_shear|sie")
    m, L = sim._model, _native.lib()
    fwd, full = L.gl_shear_loglike_workspace_bytes(m._h, B, 65, 0), L.gl_shear_loglike_workspace_bytes(m._h, B, 65, 1)
    assert 0 < fwd < full and fwd % 256 == 0 and full % 256 == 0
    assert full >= fwd + 4 * 65 * B * 4 + L.gl_lens_hessian_vjp_workspace_bytes(m._h, B, 65)
    t = {k: torch.as_tensor(v, device=sim.device) for k, v in cat.items()}
    ll, chi2, grad = (torch.empty(s, device=sim.device) for s in ((B,), (B,), (B, m.P)))
    ws = torch.empty(full, dtype=torch.uint8, device=sim.device)
    p = lambda v: v.data_ptr()
    args = [m._h, p(packed), B, p(t["x"]), p(t["y"]), p(t["scales"]), p(t["e1"]), p(t["e2"]), p(t["sigma"]), 65, p(ll), p(chi2), None]
    assert L.gl_shear_loglike(*args, p(grad), p(ws), full - 1, None) == -4 and b"workspace too small" in L.gl_last_error()  # GL_ENOMEM
    assert L.gl_shear_loglike(*args, None, p(ws), fwd - 1, None) == -4
    assert L.gl_shear_loglike(*args, None, p(ws), fwd, None) == 0
    assert L.gl_shear_loglike(*args, p(grad), p(ws), full, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(ll).all() and torch.isfinite(grad).all()
    sim_p = gl.LensSimulator(PhysicalModel([SIS(), SIS()], [], [], multiplane=MC._mp([0.4, 0.9])), _cfg(), bs=2)
    pp = torch.tensor([[1.0, 0.0, 0.0, 0.5, 0.1, 0.1]] * 2, device=sim_p.device)
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim_p.shear_log_like_and_grad(pp, _cat(cat))


# ---- WeakLensingProbModel -------------------------------------------------------------------------------------------
def _prob(gl, n=65, strong=False):
    """``(simulator, WeakLensingProbModel, ForwardProbModel or None, z [B, d])`` on the ``epl_shear|sie`` lenses; ``strong``: with the
    positions-only ``plain`` families of tests/flux_cases.py."""
    from gigalens_amd.model import ForwardProbModel, WeakLensingProbModel
    _, cat, _, _ = SC.ll_data("epl_shear|sie", n)
    _, sim, _ = _bound(gl, "epl_shear|sie")
    lp = MC.map_case("epl_shear|sie")["lens_params"]
    prior = _prior_of({"lens_mass": lp})
    fpm = None
    if strong:
        fams = FC.case("plain")["fams"]
        fpm = ForwardProbModel(prior, include_pixels=False, centroids_x=[f["x"] for f in fams], centroids_y=[f["y"] for f in fams],
                               centroids_errors_x=[f["ex"] for f in fams], centroids_errors_y=[f["ey"] for f in fams])
    pm = WeakLensingProbModel(prior, _cat(cat), strong=fpm)
    z = pm.bij.inverse(prior.sample(B, seed=3)).to(pm.device)
    return sim, pm, fpm, z, cat


def _z_gate(g, want):
    return PC.grad_gate(g.double().cpu().numpy(), want.double().cpu().numpy())


def test_prob_model_log_prob_and_gradient(gl):
    sim, pm, _, z, cat = _prob(gl)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    zz = z.clone().requires_grad_(True)
    lp_a, red_a = pm.log_prob(sim, zz)
    (g_a,) = torch.autograd.grad(lp_a.sum(), zz)
    worst = _z_gate(g, g_a)
    print(f"log_prob_and_grad against autograd of log_prob: {worst:.3f} of the gate")
    assert torch.equal(lp, lp_a.detach()) and torch.equal(red, red_a.detach()) and worst <= 1.0
    # the terms: the shear likelihood at the packed rows of z, the prior, chi2 / (2 N)
    packed = sim._pack_partial(pm.bij.forward(z))
    res = sim.shear_log_like_and_grad(packed, pm.catalogue)
    assert MC.rel_err((res["log_like"] + pm.log_prior(z)).cpu().numpy(), lp.cpu().numpy()) <= LL_RTOL
    assert torch.equal(red, res["chi2"] / (2.0 * cat["x"].size))
    # the chain rule through the bijector: d log_prob / d z from the native gradient on the packed rows
    zz = z.clone().requires_grad_(True)
    pk = sim._pack_partial(pm.bij.forward(zz))
    (g_chain,) = torch.autograd.grad((pk * res["grad"]).sum() + pm.log_prior(zz).sum(), zz)
    worst = _z_gate(g, g_chain)
    print(f"gradient against the chain rule on the native packed gradient: {worst:.3f} of the gate")
    assert worst <= 1.0


def test_prob_model_joined_with_strong_lensing(gl):
    sim, pm, fpm, z, cat = _prob(gl, strong=True)
    _, alone, _, _, _ = _prob(gl)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    lp_w, red_w, g_w = alone.log_prob_and_grad(sim, z)
    lp_s, red_s, g_s = fpm.log_prob_and_grad(sim, z)
    zz = z.clone().requires_grad_(True)
    prior = alone.log_prior(zz)
    (g_p,) = torch.autograd.grad(prior.sum(), zz)
    want_lp, want_g = lp_w - prior.detach() + lp_s, g_w - g_p + g_s  # one prior
    e_lp, worst = MC.rel_err(lp.cpu().numpy(), want_lp.cpu().numpy()), _z_gate(g, want_g)
    n_shear, n_strong = 2.0 * cat["x"].size, float(fpm._n_eff(sim))
    want_red = (red_w * n_shear + red_s * n_strong) / (n_shear + n_strong)
    e_red = MC.rel_err(red.cpu().numpy(), want_red.cpu().numpy())
    print(f"joint log_prob {e_lp:.2e}, gradient {worst:.3f} of the gate, reduced chi2 {e_red:.2e}")
    assert torch.isfinite(lp).all() and e_lp <= LL_RTOL and worst <= 1.0 and e_red <= LL_RTOL
    assert pm.n_position == n_shear + fpm.n_position and pm.include_positions and not pm.include_pixels


MAP_STEPS, MAP_LR = 150, 1e-2


def test_map_recovers_the_einstein_radius_from_shear_alone(gl):
    """SIS + Shear truth, noise-free ellipticities of 256 galaxies, 8 samples that start with theta_E 20 % high: after MAP_STEPS Adam
    steps of MAP_LR the best sample's theta_E is within a tenth of the starting offset.  A plumbing check, not a convergence study."""
    from gigalens_amd import prior as tfd
    from gigalens_amd.inference import Adam, ModellingSequence
    from gigalens_amd.model import PhysicalModel, ShearCatalogue, WeakLensingProbModel
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sis import SIS
    n, bs, theta_E = 256, 8, 1.2
    phys = PhysicalModel([SIS(), Shear()], [], [])
    truth = [{"theta_E": theta_E, "center_x": 0.05, "center_y": -0.03}, {"gamma1": 0.03, "gamma2": -0.02}]
    r = np.random.default_rng(11)
    rad, phi = r.uniform(2.0, 6.0, n), r.uniform(0, 2 * np.pi, n)  # outside the Einstein radius: the weak branch
    x, y = (rad * np.cos(phi)).astype(np.float32), (rad * np.sin(phi)).astype(np.float32)
    sim1 = gl.LensSimulator(phys, _cfg(), bs=1)
    one = [{k: torch.tensor([v], dtype=torch.float32) for k, v in d.items()} for d in truth]
    e1, e2 = sim1.reduced_shear(torch.as_tensor(x)[:, None], torch.as_tensor(y)[:, None], one)
    cat = ShearCatalogue(x, y, e1[:, 0].cpu().numpy(), e2[:, 0].cpu().numpy(), 0.25)
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J({"lens_mass": S([J({"theta_E": tfd.LogNormal(float(np.log(theta_E)), 0.3), "center_x": tfd.Normal(0.05, 0.1),
                                  "center_y": tfd.Normal(-0.03, 0.1)}),
                               J({"gamma1": tfd.Normal(0.03, 0.05), "gamma2": tfd.Normal(-0.02, 0.05)})])})
    pm = WeakLensingProbModel(prior, cat)
    jit = np.linspace(-0.02, 0.02, bs).astype(np.float32)
    start = {"lens_mass": [{"theta_E": torch.full((bs,), 1.2 * theta_E), "center_x": torch.as_tensor(0.05 + jit),
                            "center_y": torch.as_tensor(-0.03 - jit)},
                           {"gamma1": torch.full((bs,), 0.03), "gamma2": torch.full((bs,), -0.02)}]}
    z = ModellingSequence(phys, pm, _cfg()).MAP(Adam(lr=MAP_LR), start=start, n_samples=bs, num_steps=MAP_STEPS, graph=False)
    sim = gl.LensSimulator(phys, _cfg(), bs=bs)
    lp, _ = pm.log_prob(sim, z)
    best = int(torch.argmax(lp))
    got = float(pm.bij.forward(z)["lens_mass"][0]["theta_E"][best])
    print(f"MAP on shear alone: theta_E {1.2 * theta_E:.4f} -> {got:.4f} (truth {theta_E}) after {MAP_STEPS} steps of {MAP_LR}")
    assert abs(got - theta_E) <= 0.1 * 0.2 * theta_E
