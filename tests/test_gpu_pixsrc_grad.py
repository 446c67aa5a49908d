"""LensSimulator.source_evidence_and_grad (gl_pixsrc_evidence_grad + gl_lens_maps_vjp) and model.SourceEvidenceProbModel on the
GPU against the two-stage float64 oracle of tests/pixsrc_grad_cases.py, on the cases of tests/pixsrc_cases.py with their data.

Gates: GRAD_RTOL_COL (tests/test_gpu_parity.py: float32 gradients at reduced sizes, per element relative to its column's scale) for
``grad`` and ``grad_pose``; 4e-3 of a sample's largest |dE/dbeta| for ``grad_beta``.  The conditions under which these gates are
fair -- four times the float32 yardstick and four times the effect of moving every ray by one float32 ulp stay under
GRAD_RTOL_COL, no float64 ray inside the grid closer than 1e-4 to a grid line -- are asserted on the reference alone."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pixsrc_cases as PC
from tests import pixsrc_grad_cases as GC
from tests.test_gpu_parity import GRAD_RTOL_COL, gl  # noqa: F401
from tests.test_gpu_pixsrc import _call, _sim, _tensors

pytestmark = pytest.mark.gpu

BETA_RTOL = 4e-3
_RUNS = {}


def _grad_call(sim, c, obs, err, lam, **over):
    return sim.source_evidence_and_grad(_tensors(c["params"]), obs, err, **{**c["kw"], "strength": lam, **over})


def _run(gl, name):  # noqa: F811
    """One simulator and one GPU call per case, shared by the tests (left unchanged)."""
    if name not in _RUNS:
        c, obs, err, lam, _, _ = GC.case_oracle(name)
        sim = _sim(gl, c)
        _RUNS[name] = (sim, {k: v.cpu().numpy() for k, v in _grad_call(sim, c, obs, err, lam).items()})
    return _RUNS[name]


def _pose_err(g, g_o):
    return H.grad_col_err(g, g_o)


def _beta_err(g, g_o):
    """[B]: per sample the largest error of grad_beta relative to the sample's largest |dE/dbeta| (0 where the reference vanishes
    identically and so does the result)."""
    scale = np.abs(g_o).max(axis=(0, 2))
    err = np.abs(g - g_o).max(axis=(0, 2))
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)


def _oracle_cols(sim, o):
    """The oracle's [B, P] gradient and the lens columns (mass and light) it is compared on."""
    cols = [k for k, s in enumerate(sim._layout.slots) if s[0] in ("lens_mass", "lens_light")]
    return GC.packed_grad(sim, o), cols


@pytest.mark.parametrize("name", PC.CASES)
def test_conditions_on_the_reference(gl, name):  # noqa: F811
    c, obs, err, lam, o64, o32 = GC.case_oracle(name)
    sim, _ = _run(gl, name)
    g64, cols = _oracle_cols(sim, o64)
    g32, _ = _oracle_cols(sim, o32)
    yard = max(float(H.grad_col_err(g32[:, cols], g64[:, cols]).max()), float(_pose_err(o32["grad_pose"], o64["grad_pose"]).max()))
    # every ray moved by one float32 ulp (towards +inf): what the float32 ray-shoot alone may change
    fx, fy = o64["rays"]
    up = lambda a: np.nextafter(a.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    moved = GC.oracle(c, obs, err, lam, rays=(up(fx), up(fy)))
    gm, _ = _oracle_cols(sim, moved)
    ulp = max(float(H.grad_col_err(gm[:, cols], g64[:, cols]).max()), float(_pose_err(moved["grad_pose"], o64["grad_pose"]).max()))
    print(f"{name}: float32 yardstick {yard:.3g}, one-ulp ray sensitivity {ulp:.3g}, least distance to a grid line {o64['min_line_dist']:.3g}")
    assert 4 * yard <= GRAD_RTOL_COL
    assert 4 * ulp <= GRAD_RTOL_COL
    assert o64["min_line_dist"] >= 1e-4


@pytest.mark.parametrize("name", PC.CASES)
def test_gradient_against_float64(gl, name):  # noqa: F811
    c, obs, err, lam, o64, _ = GC.case_oracle(name)
    sim, got = _run(gl, name)
    g64, cols = _oracle_cols(sim, o64)
    assert got["ok"].all()
    e_grad = float(H.grad_col_err(got["grad"][:, cols], g64[:, cols]).max())
    e_pose = float(_pose_err(got["grad_pose"], o64["grad_pose"]).max())
    e_beta = float(_beta_err(got["grad_beta"], o64["grad_beta"]).max())
    print(f"{name}: grad {e_grad:.3g} / {GRAD_RTOL_COL:g}   grad_pose {e_pose:.3g} / {GRAD_RTOL_COL:g}   grad_beta {e_beta:.3g} / {BETA_RTOL:g}")
    other = [k for k in range(g64.shape[1]) if k not in cols]
    assert np.all(got["grad"][:, other] == 0.0)  # source-light columns
    assert got["grad"].dtype == np.float32 and got["grad"].shape == g64.shape and got["grad_pose"].shape == (c["B"], 3)
    assert e_grad <= GRAD_RTOL_COL
    assert e_pose <= GRAD_RTOL_COL
    assert e_beta <= BETA_RTOL


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


FORWARD = ("source", "model_image", "chi2", "reg", "log_det", "log_evidence", "ok")
GRADS = ("grad", "grad_pose", "grad_beta")


@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_outputs_are_reconstruct_sources_bits(gl, name):  # noqa: F811
    c, obs, err, lam, _, _ = GC.case_oracle(name)
    sim, got = _run(gl, name)
    fwd = {k: v.cpu().numpy() for k, v in _call(sim, c, obs, err, strength=lam).items()}
    for k in FORWARD:
        assert _same_bits(got[k], fwd[k]), k


def test_deterministic_and_batch_independent(gl):  # noqa: F811
    c, obs, err, lam, _, _ = GC.case_oracle("A")
    sim, got = _run(gl, "A")
    again = {k: v.cpu().numpy() for k, v in _grad_call(sim, c, obs, err, lam).items()}
    for k in GRADS + FORWARD:
        assert _same_bits(got[k], again[k]), k
    for b in range(c["B"]):  # a sample alone gives the bits it has in its batch
        c1 = dict(c, B=1, params={g: [{k: (np.asarray(v)[b:b + 1] if np.asarray(v).size == c["B"] else v) for k, v in d.items()} for d in lst]
                                 for g, lst in c["params"].items()})
        kw = dict(c["kw"])
        kw["pitch"], kw["center"] = kw["pitch"][b:b + 1], (kw["center"][0][b:b + 1], kw["center"][1][b:b + 1])
        c1["kw"] = kw
        sim1 = _sim(gl, c1)
        one = {k: v.cpu().numpy() for k, v in _grad_call(sim1, c1, obs[b:b + 1], err, lam[b:b + 1]).items()}
        assert _same_bits(one["grad"][0], got["grad"][b]) and _same_bits(one["grad_pose"][0], got["grad_pose"][b])
        assert _same_bits(one["grad_beta"][:, 0], got["grad_beta"][:, b])


def test_rays_that_are_not_finite(gl):  # noqa: F811
    """Case D: the sample whose every ray is NaN has an exactly zero gradient (and is ok: M = lambda R); the sample with one NaN
    pixel matches the oracle (test_gradient_against_float64) and that pixel's cotangent is exactly zero."""
    c, obs, err, lam, o64, _ = GC.case_oracle("D")
    sim, got = _run(gl, "D")
    assert got["ok"].all()
    assert np.all(got["grad"][1] == 0.0) and np.all(got["grad_pose"][1] == 0.0) and np.all(got["grad_beta"][:, 1] == 0.0)
    nan_ray = ~np.isfinite(o64["rays"][0][:, 2])
    assert nan_ray.sum() == 1 and np.all(got["grad_beta"][:, 2, nan_ray] == 0.0)
    assert np.all(np.isfinite(got["grad"])) and np.all(np.isfinite(got["grad_beta"]))


def test_broken_pivot_gives_nan_gradients(gl):  # noqa: F811
    """The construction of test_gpu_pixsrc.py::test_broken_pivot_is_flagged_not_raised: ok == False with NaN gradients, and the
    healthy sample beside it has the bits it has alone."""
    c, obs, err, _, _ = PC.data("C21")
    c2 = dict(c, B=2, params={g: [{k: np.repeat(v, 2) for k, v in d.items()} for d in lst] for g, lst in c["params"].items()})
    obs2 = np.repeat(obs, 2, axis=0)
    err2 = np.stack([np.full_like(err, 1e-25), err])
    lam2 = np.asarray([1e-30, c["kw"]["strength"][0]], dtype=np.float32)
    sim2 = _sim(gl, c2)
    got = {k: v.cpu().numpy() for k, v in _grad_call(sim2, c2, obs2, err2, lam2).items()}
    assert got["ok"].tolist() == [False, True]
    assert all(np.isnan(got[k][0]).all() for k in ("grad", "grad_pose")) and np.isnan(got["grad_beta"][:, 0]).all()
    _, alone = _run(gl, "C21")
    assert _same_bits(got["grad"][1], alone["grad"][0]) and _same_bits(got["grad_pose"][1], alone["grad_pose"][0])
    assert _same_bits(got["grad_beta"][:, 1], alone["grad_beta"][:, 0])


def test_planes_in_more_than_one_launch(gl):  # noqa: F811
    """Case B's geometry with three samples: 3 x 1023 planes exceed what one post-processing launch holds, so the contraction
    accumulates over at least two launches (and a sample's planes straddle them); compared with the unchunked oracle."""
    c, obs, err, lam, _, _ = GC.case_oracle("B")
    rep = lambda v: np.asarray(v)[[0, 1, 0]]
    c3 = dict(c, B=3, params={g: [{k: (rep(v) if np.asarray(v).size == 2 else v) for k, v in d.items()} for d in lst]
                             for g, lst in c["params"].items()})
    obs3, lam3 = rep(obs), rep(lam)
    sim = _sim(gl, c3)
    n_used = int(np.prod(c["cfg"].num_pix))
    lay = sim._model.pixsrc_grad_layout(3, c["kw"]["n_src"], n_used)
    assert lay["pc"] < 3 * 1023 and lay["cb"] == 3, lay
    got = {k: v.cpu().numpy() for k, v in _grad_call(sim, c3, obs3, err, lam3).items()}
    o = GC.oracle(c3, obs3, err, lam3)
    g64, cols = _oracle_cols(sim, o)
    e_grad = float(H.grad_col_err(got["grad"][:, cols], g64[:, cols]).max())
    e_beta = float(_beta_err(got["grad_beta"], o["grad_beta"]).max())
    print(f"planes in {-(-3 * 1023 // lay['pc'])} launches: grad {e_grad:.3g} / {GRAD_RTOL_COL:g}   grad_beta {e_beta:.3g} / {BETA_RTOL:g}")
    assert e_grad <= GRAD_RTOL_COL and e_beta <= BETA_RTOL
    _, two = _run(gl, "B")  # and the samples keep the bits they have in the two-sample call
    assert _same_bits(got["grad"][:2], two["grad"]) and _same_bits(got["grad"][2], two["grad"][0])


def test_samples_in_more_than_one_chunk(gl):  # noqa: F811
    """A 6 x 5 frame with 32 x 32 = 1024 nodes: a sample needs 4 (2 S n_pad + 2 n_pad + 2 S^2 + S) = 8 655 104 bytes, 31 fit into the
    256 MiB budget, so 32 samples run as chunks of 31 and 1.  The samples alternate between two parameter sets; every one is
    compared with the unchunked oracle of its set, and the last one (a chunk of its own) has the bits of the first of its set."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    f = PC._f32
    src = PC.case("C11")["params"]["source_light"]
    params2 = {"lens_mass": [{"theta_E": f(0.25, 0.22), "e1": f(0.1, -0.05), "e2": f(0.05, 0.08), "center_x": f(0.0, 0.01),
                              "center_y": f(0.0, -0.01)}, {"gamma1": f(0.02, -0.01), "gamma2": f(-0.01, 0.02)}], "source_light": src}
    kw = dict(n_src=(32, 32), pitch=f(0.02), center=(f(0.01), f(0.0)), regularization="gradient", strength=f(1.0), mask=None)
    c2 = dict(phys=PhysicalModel([SIE(), Shear()], [], [Sersic()]), cfg=SimulatorConfig(delta_pix=PC.DELTA_PIX, num_pix=(6, 5), supersample=1),
              psf=None, params=params2, kw=kw, sigma=0.01, B=2)
    rng = np.random.default_rng(7)
    obs2 = (0.05 + 0.01 * rng.normal(size=(2, 6, 5))).astype(np.float32)
    err = np.full((6, 5), 0.01, dtype=np.float32)
    lam2 = np.ones(2, dtype=np.float32)
    o = GC.oracle(c2, obs2, err, lam2)
    assert o["min_line_dist"] >= 1e-4
    B = 32
    sel = np.arange(B) % 2
    c32 = dict(c2, B=B, params={g: [{k: (np.asarray(v)[sel] if np.asarray(v).size == 2 else v) for k, v in d.items()} for d in lst]
                               for g, lst in params2.items()})
    sim = _sim(gl, c32)
    lay = sim._model.pixsrc_grad_layout(B, (32, 32), 30)
    assert lay["cb"] == 31 and lay["n_pad"] == 32, lay
    got = {k: v.cpu().numpy() for k, v in _grad_call(sim, c32, obs2[sel], err, lam2[sel]).items()}
    assert got["ok"].all()
    sim2 = _sim(gl, c2)
    g64, cols = _oracle_cols(sim2, o)
    e_grad = float(H.grad_col_err(got["grad"][:, cols], g64[sel][:, cols]).max())
    e_pose = float(_pose_err(got["grad_pose"], o["grad_pose"][sel]).max())
    e_beta = float(_beta_err(got["grad_beta"], o["grad_beta"][:, sel]).max())
    print(f"chunks of 31 + 1 samples: grad {e_grad:.3g} / {GRAD_RTOL_COL:g}   grad_pose {e_pose:.3g} / {GRAD_RTOL_COL:g}   grad_beta {e_beta:.3g} / {BETA_RTOL:g}")
    assert e_grad <= GRAD_RTOL_COL and e_pose <= GRAD_RTOL_COL and e_beta <= BETA_RTOL
    for k in ("grad", "grad_pose"):
        assert _same_bits(got[k][31], got[k][1]), k
    assert _same_bits(got["grad_beta"][:, 31], got["grad_beta"][:, 1])


def test_refusals(gl):  # noqa: F811
    from gigalens_amd import _native
    c, obs, err, lam, _, _ = GC.case_oracle("A")
    sim, _ = _run(gl, "A")
    with pytest.raises(ValueError, match="strength"):
        _grad_call(sim, c, obs, err, np.ones((3, 2), dtype=np.float32))
    packed = sim._pack_partial(_tensors(c["params"])).requires_grad_(True)
    with pytest.raises(NotImplementedError):  # reconstruct_source stays forward only
        sim.reconstruct_source(packed, obs, err, **c["kw"])
    with pytest.raises(NotImplementedError):  # and the gradient call takes plain inputs (SourceEvidenceProbModel is the autograd entry)
        sim.source_evidence_and_grad(packed, obs, err, **c["kw"])
    # lens planes, user-written lenses
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import SimulatorConfig
    from tests import multilens_cases as MC
    from tests.test_user_profile_compile import SIS_BODY
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    img, rms = np.zeros((8, 8), np.float32), np.ones((8, 8), np.float32)
    kw = dict(n_src=(3, 3), pitch=0.1)
    sis = {"theta_E": torch.tensor([0.3]), "center_x": torch.tensor([0.0]), "center_y": torch.tensor([0.01])}
    sim_p = gl.LensSimulator(PhysicalModel([SIS(), SIS()], [], [Sersic()], multiplane=MC._mp([0.4, 0.9], [2.0])), cfg, bs=1)
    with pytest.raises(_native.UnsupportedLensError):
        sim_p.source_evidence_and_grad({"lens_mass": [sis, sis]}, img, rms, **kw)

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    sim_u = gl.LensSimulator(PhysicalModel([UserSIS()], [], [Sersic()]), cfg, bs=1)
    with pytest.raises(_native.UnsupportedLensError, match="user-written"):
        sim_u.source_evidence_and_grad({"lens_mass": [sis]}, img, rms, **kw)


# ---- SourceEvidenceProbModel on the geometry of case A (no PSF: ModellingSequence builds its simulator from the config alone) -------
def _prob_case():
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import SourceEvidenceProbModel
    c = PC.case("A")
    B, kw = c["B"], dict(c["kw"])
    kw["pitch"], kw["center"], kw["strength"] = float(kw["pitch"][0]), (float(kw["center"][0][0]), float(kw["center"][1][0])), 2.0
    H_, W_ = c["cfg"].num_pix
    err = np.full((H_, W_), c["sigma"], dtype=np.float32)
    truth = {g: [{k: np.asarray(v)[:1] for k, v in d.items()} for d in lst] for g, lst in c["params"].items()}
    _, parts = PC.reconstruct(c["phys"], c["cfg"], None, truth, np.zeros((H_, W_), np.float32), err,
                              **{**kw, "strength": np.ones(1, np.float32), "mask": None}, return_parts="only")
    clean = parts[0][1] @ PC.smooth_source(kw["n_src"], 0).reshape(-1) - parts[0][2]
    obs = (clean.reshape(H_, W_) + c["sigma"] * np.random.default_rng(5).normal(size=(H_, W_))).astype(np.float32)
    t = truth
    N = lambda d, k, s: tfd.Normal(float(d[k][0]), s)
    prior = tfd.JointDistributionNamed(dict(
        lens_mass=tfd.JointDistributionSequential([
            tfd.JointDistributionNamed(dict(theta_E=tfd.LogNormal(float(np.log(t["lens_mass"][0]["theta_E"][0])), 0.1),
                                            e1=N(t["lens_mass"][0], "e1", 0.05), e2=N(t["lens_mass"][0], "e2", 0.05),
                                            center_x=N(t["lens_mass"][0], "center_x", 0.02), center_y=N(t["lens_mass"][0], "center_y", 0.02))),
            tfd.JointDistributionNamed(dict(gamma1=N(t["lens_mass"][1], "gamma1", 0.02), gamma2=N(t["lens_mass"][1], "gamma2", 0.02)))]),
        lens_light=tfd.JointDistributionSequential([
            tfd.JointDistributionNamed(dict(R_sersic=tfd.LogNormal(float(np.log(t["lens_light"][0]["R_sersic"][0])), 0.05),
                                            n_sersic=tfd.LogNormal(float(np.log(t["lens_light"][0]["n_sersic"][0])), 0.05),
                                            center_x=N(t["lens_light"][0], "center_x", 0.01), center_y=N(t["lens_light"][0], "center_y", 0.01),
                                            Ie=tfd.LogNormal(float(np.log(t["lens_light"][0]["Ie"][0])), 0.05)))])))
    pm = SourceEvidenceProbModel(prior, obs, err, n_src=kw["n_src"], pitch=kw["pitch"], center=kw["center"],
                                 regularization=kw["regularization"], strength=kw["strength"], mask=kw["mask"])
    return c, pm, B


def test_prob_model_value_and_gradient_agree(gl):  # noqa: F811
    """For eps with a predicted rise eps |g|^2 = 0.05, lp(z + eps g) - lp(z) lies within 25 % of the prediction for every sample:
    the margin is for curvature; the kink spacing makes smaller steps pointless."""
    c, pm, B = _prob_case()
    sim = gl.LensSimulator(c["phys"], c["cfg"], bs=B)
    z = pm.bij.inverse(pm.prior.sample(B, seed=11)).to(pm.device)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    assert lp.shape == (B,) and red.shape == (B,) and g.shape == z.shape
    assert torch.isfinite(lp).all() and torch.isfinite(g).all() and torch.isfinite(red).all()
    eps = 0.05 / (g.double() ** 2).sum(dim=1)
    lp2, _ = pm.log_prob(sim, z + (eps[:, None] * g.double()).float())
    rise = (lp2.double() - lp.double()).cpu().numpy()
    print("rise / predicted:", (rise / 0.05).tolist())
    assert np.all(np.abs(rise / 0.05 - 1.0) <= 0.25)
    zz = z.clone().requires_grad_(True)  # the autograd entry gives the same gradient
    pm.log_prob(sim, zz)[0].sum().backward()
    assert torch.equal(zz.grad, g)


def test_prob_model_gradient_against_the_oracle_chain(gl):  # noqa: F811
    """``g`` of ``log_prob_and_grad`` against float64 autograd of the oracle chain: the oracle's d E / d parameters (at the float32
    parameters the library receives) through the bijector, plus the prior and its log-Jacobian, all in float64."""
    c, pm, B = _prob_case()
    sim = gl.LensSimulator(c["phys"], c["cfg"], bs=B)
    z = pm.bij.inverse(pm.prior.sample(B, seed=25)).to(pm.device)  # (a draw whose rays keep 6.7e-4 from the grid lines)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    struct32 = pm.pack_bij.forward(pm._flat.forward(z))
    params = {grp: [{k: v.detach().cpu().numpy().astype(np.float32) for k, v in d.items()} for d in lst] for grp, lst in struct32.items()}
    params["source_light"] = c["params"]["source_light"]
    kw = dict(n_src=pm.n_src, pitch=np.float32(pm.pitch), center=(np.float32(pm.center[0]), np.float32(pm.center[1])),
              regularization=pm.regularization, strength=np.float32(pm.strength), mask=pm.mask)
    cc = dict(phys=c["phys"], cfg=c["cfg"], psf=None, params=params, kw=kw, B=B)
    obs = np.repeat(pm.observed_image.cpu().numpy()[None], B, axis=0)
    o = GC.oracle(cc, obs, pm.err_map.cpu().numpy(), np.full(B, pm.strength, dtype=np.float32))
    assert o["min_line_dist"] >= 1e-4
    flat = pm.prior.flat(torch.device("cpu"))
    z64 = z.detach().cpu().double().requires_grad_(True)
    x64 = flat.forward(z64)
    st = pm.pack_bij.forward(x64)
    tot = flat.log_prob(x64) + flat.fldj_columns(z64).sum(-1)
    for grp, key in (("lens_mass", "grad_lens"), ("lens_light", "grad_light")):
        for i, d in enumerate(st[grp]):
            for k, v in d.items():
                tot = tot + v * torch.as_tensor(o[key][i][k])
    (g64,) = torch.autograd.grad(tot.sum(), z64)
    e = float(H.grad_col_err(g.cpu().numpy(), g64.numpy()).max())
    lp64 = o["E"] + (flat.log_prob(x64) + flat.fldj_columns(z64).sum(-1)).detach().numpy()
    print(f"prob model: g {e:.3g} / {GRAD_RTOL_COL:g}   lp - oracle {np.abs(lp.cpu().numpy() - lp64).max():.3g}")
    assert e <= GRAD_RTOL_COL
    np.testing.assert_allclose(lp.cpu().numpy(), lp64, rtol=1e-5, atol=1e-3)


def test_map_raises_the_evidence(gl):  # noqa: F811
    from gigalens_amd.inference import Adam, ModellingSequence
    c, pm, B = _prob_case()
    start = pm.prior.sample(B, seed=3)
    start["lens_mass"][0]["theta_E"] = torch.as_tensor(np.full(B, 1.03 * 0.30, dtype=np.float32))  # theta_E off by 3 %
    sim = gl.LensSimulator(c["phys"], c["cfg"], bs=B)
    z0 = pm.bij.inverse(start).to(pm.device)
    lp0, _ = pm.log_prob(sim, z0)
    seq = ModellingSequence(c["phys"], pm, c["cfg"])
    z1 = seq.MAP(Adam(lr=2e-3), start=start, n_samples=B, num_steps=30, graph=False)
    lp1, _ = pm.log_prob(sim, torch.as_tensor(z1, device=pm.device))
    print("MAP: mean log_prob", float(lp0.mean()), "->", float(lp1.mean()))
    assert torch.isfinite(lp1).all()
    assert float(lp1.mean()) > float(lp0.mean())


def test_svi_and_hmc_run_on_the_stream_path(gl):  # noqa: F811
    """A few steps of ``ModellingSequence.SVI`` and ``HMC`` on the evidence: they need ``log_prob_and_grad``, ``init_centroids`` and the
    class attributes alone, and leave finite surrogates and samples."""
    from gigalens_amd.inference import Adam, ModellingSequence
    c, pm, B = _prob_case()
    assert not hasattr(pm, "_fused_ok")
    z0 = pm.bij.inverse(pm.prior.sample(1, seed=25))[0]
    seq = ModellingSequence(c["phys"], pm, c["cfg"])
    (mean, tril), losses = seq.SVI(Adam(lr=1e-3), start_mean=z0, n_vi=B, init_scales=1e-3, num_steps=4)
    assert len(losses) == 4 and np.all(np.isfinite(losses)) and torch.isfinite(mean).all() and torch.isfinite(tril).all()
    samples = seq.HMC((mean, tril), init_eps=0.05, init_l=2, n_hmc=B, num_burnin_steps=3, num_results=3, max_leapfrog_steps=3)
    samples = samples[0] if isinstance(samples, (tuple, list)) else samples
    assert torch.isfinite(torch.as_tensor(samples)).all()
