"""Point images in the pixel likelihood on the GPU (csrc/gl_ptimg.hip.h; LensSimulator.point_images, fit_point_images,
point_image_log_like_and_grad; model.PointImageProbModel) against the float64 restatement of tests/point_image_cases.py.

Gates.  ``point_images``: per pixel the bound of ``point_image_cases.render_bound`` (Higham's gamma_n on the sum of |terms|, n = 16 ss^2
+ 2, plus the effect of rounding (u, v) to float32) -- nothing in it is measured on the kernels.  ``chi2`` and ``log_like``: rtol 1e-5,
the project's chi^2 contract.  Amplitudes: four times the float32 floor -- the worst deviation from float64 of the restatement run in
float32 on the CPU with its pixel sums in three different orders (another valid summation order may not be worse than a few times
one of these; ``point_image_cases.float32_amplitude_floor``) --, at most 1e-4 of a sample's largest amplitude.  Gradients: tests/helpers.py ``grad_gate`` at GRAD_RTOL_COL with the
column scale from the float64 rows; elements beyond it must lie within four times the error of the restatement's own float32 run,
and may be at most 5 % of the elements."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import point_image_cases as PI
from tests import post_cases as PO
from tests.test_gpu_parity import GRAD_RTOL_COL, gl  # noqa: F401

pytestmark = pytest.mark.gpu

CHI2_RTOL = 1e-5
_SIMS, _FITS = {}, {}


def _sim(gl, cam_name, B):  # noqa: F811
    if (cam_name, B) not in _SIMS:
        cam = PI.camera(cam_name)
        _SIMS[(cam_name, B)] = gl.LensSimulator(PI.phys_model(), cam["cfg"], bs=B, supersampled_kernel=cam["psf"])
    return _SIMS[(cam_name, B)]


def _dev(sim, a):
    return torch.as_tensor(a, device=sim.device)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _fit_run(gl, name):  # noqa: F811
    """One simulator and one gradient call per case, shared by the tests (left unchanged)."""
    if name not in _FITS:
        c = PI.fit_case(name)
        sim = _sim(gl, PI.FIT_CASES[name], c["B"])
        packed = sim.pack({g: [{k: torch.as_tensor(v) for k, v in d.items()} for d in lst] for g, lst in c["params"].items()})
        res = sim.point_image_log_like_and_grad(packed, _dev(sim, c["x"]), _dev(sim, c["y"]), c["obs"], c["err"], mask=c["cam"]["mask"])
        _FITS[name] = (sim, packed, {k: v.cpu().numpy() for k, v in res.items()})
    return _FITS[name]


# ---- the render -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_name,J,B,first", PI.RENDER_CASES)
def test_point_images_against_the_restatement(gl, cam_name, J, B, first):  # noqa: F811
    c = PI.render_case(cam_name, J, B, first)
    sim = _sim(gl, cam_name, B)
    got = sim.point_images(_dev(sim, c["x"]), _dev(sim, c["y"]), _dev(sim, c["amp"])).cpu().numpy().astype(np.float64)
    D = PI.unit_images(c["cam"], torch.as_tensor(c["x"]).double(), torch.as_tensor(c["y"]).double()).numpy()
    want = (c["amp"].astype(np.float64)[:, :, None, None] * D).sum(axis=1)
    bound = PI.render_bound(c)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"{cam_name} J={J} B={B}: worst error / bound {ratio.max():.3g}; max |image| {np.abs(want).max():.3g}, max error {err.max():.3g}")
    assert got.shape == (B, c["cam"]["H"], c["cam"]["W"])
    assert np.all(np.isfinite(got))
    assert ratio.max() <= 1.0
    # where no image reaches, the pixel is exactly zero (positions that are not finite or far outside reach nowhere)
    assert np.all(got[want == 0.0] == 0.0)
    if first + B * J >= PI.N_RENDER_POSITIONS:  # (the case reaches the positions of that kind)
        assert (D == 0.0).all(axis=(2, 3)).sum() >= 5


@pytest.mark.parametrize("cam_name", ["plain9", "ss2_psf5", "ss2_psf3_mask"])
def test_point_images_at_nodes_against_post_apply(gl, cam_name):  # noqa: F811
    """At integer (u, v) the unit image is the model's own post-processing of a one-hot frame times ss^2 (scale 1).  The
    post-processing kernels are held to their own bound (tests/post_cases.py: gamma_n sum |terms|, n at most (kh + ss - 1) x 32 +
    9: rows of the effective kernel x the widest padded row, the partial sums, two roundings), the point image to `render_bound`."""
    cam = PI.camera(cam_name)
    ss = cam["ss"]
    Hs, Ws = cam["H"] * ss, cam["W"] * ss
    nodes = [(Hs // 2, Ws // 2), (0, 0), (Hs - 1, 2), (1, Ws - 1), (3, 5)]
    B = len(nodes)
    x, y = PI.xy_of(cam, np.array([[c] for _, c in nodes], dtype=np.float64), np.array([[r] for r, _ in nodes], dtype=np.float64))
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x) and np.array_equal(y32.astype(np.float64), y)  # the nodes are exact in float32
    sim = _sim(gl, cam_name, B)
    amp = np.ones((B, 1), dtype=np.float32)
    got = sim.point_images(_dev(sim, x32), _dev(sim, y32), _dev(sim, amp)).cpu().numpy().astype(np.float64)
    hot = torch.zeros((B, Hs, Ws), dtype=torch.float32, device=sim.device)
    for b, (r, c) in enumerate(nodes):
        hot[b, r, c] = 1.0
    if sim._model.has_post if hasattr(sim._model, "has_post") else (ss > 1 or cam["psf"] is not None):
        post = sim._model.post_apply(hot, scale=1.0).cpu().numpy().astype(np.float64) * (ss * ss)
    else:
        post = hot.cpu().numpy().astype(np.float64)
    kh = 1 if cam["psf"] is None else cam["psf"].shape[0]
    case = dict(cam=cam, x=x32, y=y32, amp=amp)
    D_abs = PI.unit_images(cam, torch.as_tensor(x), torch.as_tensor(y), "abs").numpy()[:, 0]
    bound = PI.render_bound(case) + PO.gamma((kh + ss - 1) * 32 + 9) * D_abs
    err = np.abs(got - post)
    print(f"{cam_name}: worst |point image - ss^2 post(one hot)| / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert np.all(err <= bound)
    assert np.all(got[post == 0.0] == 0.0)


def test_point_images_backward(gl):  # noqa: F811
    """``point_images(...).backward()`` is ``gl_ptimg_render_bwd`` (same bits) and the restatement's autograd."""
    cam_name, B, J = "ss2_psf5", 3, 4
    cam = PI.camera(cam_name)
    sim = _sim(gl, cam_name, B)
    u, v = PI._ring(cam, J, B, "backward", 2.4, 0.4)
    x, y = (a.astype(np.float32) for a in PI.xy_of(cam, u, v))
    r = PI._rng("backward")
    amp = r.uniform(0.5, 2.0, size=(B, J)).astype(np.float32)
    cot = r.normal(size=(B, cam["H"], cam["W"])).astype(np.float32)
    xt, yt, at = (_dev(sim, a).requires_grad_(True) for a in (x, y, amp))
    img = sim.point_images(xt, yt, at)
    (img * _dev(sim, cot)).sum().backward()
    gx, gy, ga = sim._model.ptimg_render_bwd(_dev(sim, x), _dev(sim, y), _dev(sim, amp), sim._point_transform(), _dev(sim, cot))
    for got, explicit in ((xt.grad, gx), (yt.grad, gy), (at.grad, ga)):
        assert _same_bits(got.cpu().numpy(), explicit.cpu().numpy())
    x64, y64, a64 = (torch.as_tensor(a).double().requires_grad_(True) for a in (x, y, amp))
    ref_img = (a64[:, :, None, None] * PI.unit_images(cam, x64, y64)).sum(dim=1)
    wx, wy, wa = torch.autograd.grad((ref_img * torch.as_tensor(cot).double()).sum(), [x64, y64, a64])
    for got, want, what in ((xt.grad, wx, "x"), (yt.grad, wy, "y"), (at.grad, wa, "amplitude")):
        e = float(H.grad_col_err(got.cpu().numpy(), want.numpy()).max())
        print(f"d/d{what}: {e:.3g} / {GRAD_RTOL_COL:g}")
        assert e <= GRAD_RTOL_COL


# ---- the fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PI.SOLVABLE)
def test_fit_against_the_restatement(gl, name):  # noqa: F811
    c, o = PI.fit_case(name), PI.fit_reference(name)
    sim, packed, got = _fit_run(gl, name)
    fwd = {k: v.cpu().numpy() for k, v in sim.fit_point_images(packed, _dev(sim, c["x"]), _dev(sim, c["y"]), c["obs"], c["err"],
                                                                 mask=c["cam"]["mask"]).items()}
    for k in fwd:  # the forward call gives the bits of the gradient call
        assert _same_bits(fwd[k], got[k]), k
    assert got["ok"].all() and got["chi2"].dtype == np.float64 and got["log_like"].dtype == np.float64
    floor = PI.float32_amplitude_floor(name)
    tol = min(4.0 * floor, PI.AMP_RTOL_CAP)
    e_amp = float(PI.amplitude_error(got["amplitudes"], o["amplitudes"]).max())
    e_chi2, e_ll = H.relerr(got["chi2"], o["chi2"]), float(np.max(np.abs(got["log_like"] - o["log_like"]) / np.abs(o["log_like"])))
    print(f"{name}: amplitudes {e_amp:.3g} / {tol:.3g} (float32 floor {floor:.3g})   chi2 {e_chi2:.3g}   log_like {e_ll:.3g} / {CHI2_RTOL:g}")
    assert e_amp <= tol
    assert np.allclose(got["chi2"], o["chi2"], rtol=CHI2_RTOL, atol=0.0)
    assert np.allclose(got["log_like"], o["log_like"], rtol=CHI2_RTOL, atol=0.0)
    # the model image is the extended image plus the render of the fitted amplitudes, term for term
    pts = sim.point_images(_dev(sim, c["x"]), _dev(sim, c["y"]), _dev(sim, got["amplitudes"])).cpu().numpy()
    assert _same_bits(got["model_image"], got["extended_image"] + pts)
    assert np.abs(got["model_image"] - o["model_image"]).max() <= 1e-4 * np.abs(o["model_image"]).max()


@pytest.mark.parametrize("name", sorted(PI.SINGULAR))
def test_singular_samples_are_flagged_and_the_others_unharmed(gl, name):  # noqa: F811
    c, o = PI.fit_case(name), PI.fit_reference(name)
    sim, packed, got = _fit_run(gl, name)
    bad = PI.SINGULAR[name]
    good = np.arange(c["B"]) != bad
    assert got["ok"].tolist() == good.tolist()
    for k in ("amplitudes", "model_image", "chi2", "log_like", "grad", "grad_x", "grad_y"):
        assert np.isnan(got[k][bad]).all(), k
        assert np.isfinite(got[k][good]).all(), k
    assert np.allclose(got["chi2"][good], o["chi2"][good], rtol=CHI2_RTOL, atol=0.0)
    assert float(PI.amplitude_error(got["amplitudes"][good], o["amplitudes"][good]).max()) <= PI.AMP_RTOL_CAP


@pytest.mark.parametrize("name", PI.SOLVABLE)
def test_gradient_against_autograd_through_the_solve(gl, name):  # noqa: F811
    o64, o32 = PI.fit_reference(name), PI.fit_reference(name, PI.F32)
    _, _, got = _fit_run(gl, name)
    n_bad = n_all = 0
    for k in ("grad", "grad_x", "grad_y"):
        ok, rep = H.grad_gate(got[k], o64[k], GRAD_RTOL_COL,
                              lambda S, k=k: np.abs(o32[k].astype(np.float64) - o64[k]) / S)
        print(f"{name} {k}: {rep}")
        assert ok, (k, rep)
        n_bad += rep["conditioned"]
        n_all += got[k].size
    assert n_bad <= 0.05 * n_all, (n_bad, n_all)


def test_input_checks(gl):  # noqa: F811
    c = PI.fit_case("quad")
    sim, packed, _ = _fit_run(gl, "quad")
    x, y = _dev(sim, c["x"]), _dev(sim, c["y"])
    with pytest.raises(ValueError):
        sim.fit_point_images(packed, x[:, :1].expand(-1, 9), y[:, :1].expand(-1, 9), c["obs"], c["err"])  # J = 9
    with pytest.raises(ValueError):
        sim.fit_point_images(packed, x, y[:, :2], c["obs"], c["err"])
    with pytest.raises(ValueError):
        sim.fit_point_images(packed, x, y, c["obs"][:, :-1], c["err"])
    bad = c["err"].copy()
    bad[3, 3] = 0.0
    with pytest.raises(ValueError):
        sim.fit_point_images(packed, x, y, c["obs"], bad)
    mask = np.ones_like(bad, dtype=bool)
    mask[3, 3] = False  # ... unless that pixel is not used
    assert sim.fit_point_images(packed, x, y, c["obs"], bad, mask=mask)["ok"].all()
    with pytest.raises(ValueError):
        sim.fit_point_images(packed, x, y, c["obs"], c["err"], mask=np.zeros_like(mask))
    with pytest.raises(ValueError):
        sim.point_images(x, y, x[:, :3])


def test_deterministic(gl):  # noqa: F811
    c = PI.fit_case("octet")
    sim, packed, got = _fit_run(gl, "octet")
    again = sim.point_image_log_like_and_grad(packed, _dev(sim, c["x"]), _dev(sim, c["y"]), c["obs"], c["err"], mask=c["cam"]["mask"])
    for k, v in again.items():
        assert _same_bits(v.cpu().numpy(), got[k]), k
    rc = PI.render_case("rot_even", 8, 3, 4)
    imgs = [sim3.point_images(_dev(sim3, rc["x"]), _dev(sim3, rc["y"]), _dev(sim3, rc["amp"])).cpu().numpy()
            for sim3 in [_sim(gl, "rot_even", 3)] * 2]
    assert _same_bits(*imgs)


# ---- the probabilistic model ------------------------------------------------------------------------------------------------
def _quasar(gl, B=4, seed=5):  # noqa: F811
    """A 12 x 12 synthetic quasar + host, rendered by the product: ``(phys, cfg, prior, truth, obs, err)``; the prior of the image
    positions is centred on the truth."""
    from gigalens_amd import prior as tfd
    from gigalens_amd.simulator import SimulatorConfig
    phys = PI.phys_model()
    cfg = SimulatorConfig(delta_pix=PI.DELTA_PIX, num_pix=12, supersample=1, kernel=PI.gauss_psf((5, 5), 1.2))
    xs = np.array([0.19, -0.17, 0.03, -0.05], dtype=np.float32)
    ys = np.array([0.04, -0.02, 0.18, -0.19], dtype=np.float32)
    N, LN, U = tfd.Normal, tfd.LogNormal, tfd.Uniform
    mass = tfd.JointDistributionNamed(dict(theta_E=LN(math.log(0.18), 0.05), e1=N(0, 0.05), e2=N(0, 0.05), center_x=N(0, 0.01),
                                           center_y=N(0, 0.01)))
    shear = tfd.JointDistributionNamed(dict(gamma1=N(0, 0.03), gamma2=N(0, 0.03)))
    src = tfd.JointDistributionNamed(dict(R_sersic=LN(math.log(0.06), 0.1), n_sersic=U(1.0, 2.0), center_x=N(0, 0.02), center_y=N(0, 0.02),
                                          Ie=LN(math.log(10.0), 0.2)))
    images = [tfd.JointDistributionNamed(dict(x=N(float(a), 0.05), y=N(float(b), 0.05))) for a, b in zip(xs, ys)]
    prior = tfd.JointDistributionNamed(dict(lens_mass=tfd.JointDistributionSequential([mass, shear]),
                                            source_light=tfd.JointDistributionSequential([src]),
                                            point_images=tfd.JointDistributionSequential(images)))
    sim = gl.LensSimulator(phys, cfg, bs=1)
    truth = prior.sample(1, seed=seed)
    truth["point_images"] = [{"x": torch.tensor([float(a)]), "y": torch.tensor([float(b)])} for a, b in zip(xs, ys)]
    flux = torch.tensor([[40.0, 55.0, 30.0, 45.0]], device=sim.device)
    clean = sim.simulate(truth).reshape(1, 12, 12) + sim.point_images(_dev(sim, xs[None]), _dev(sim, ys[None]), flux)
    err = np.full((12, 12), 0.3, dtype=np.float32)
    obs = clean[0].cpu().numpy() + err * np.random.default_rng(seed).normal(size=(12, 12)).astype(np.float32)
    return phys, cfg, prior, truth, obs.astype(np.float32), err


def _start(prior, truth, B, shift):
    """the truth repeated B times with every image position moved by ``shift`` pixels in a direction of its own"""
    r = np.random.default_rng(11)
    start = {g: [{k: torch.as_tensor(v).reshape(-1)[:1].repeat(B) for k, v in d.items()} for d in lst] for g, lst in truth.items()}
    for d in start["point_images"]:
        ang = torch.as_tensor(r.uniform(0, 2 * np.pi, size=B), dtype=torch.float32)
        d["x"] = d["x"] + shift * PI.DELTA_PIX * torch.cos(ang)
        d["y"] = d["y"] + shift * PI.DELTA_PIX * torch.sin(ang)
    return start


@pytest.mark.parametrize("sigma", [None, 0.02])
def test_prob_model_gradient_is_autograd_of_log_prob(gl, sigma):  # noqa: F811
    from gigalens_amd.model import PointImageProbModel
    phys, cfg, prior, truth, obs, err = _quasar(gl)
    B = 4
    pm = PointImageProbModel(prior, obs, err, source_plane_sigma=sigma)
    sim = gl.LensSimulator(phys, cfg, bs=B)
    z = pm.bij.inverse(_start(prior, truth, B, 0.3)).to(sim.device)
    lp, red, g = pm.log_prob_and_grad(sim, z)
    zz = z.clone().requires_grad_(True)
    lp2, red2 = pm.log_prob(sim, zz)
    (g2,) = torch.autograd.grad(lp2.sum(), zz)
    assert _same_bits(lp.cpu().numpy(), lp2.detach().cpu().numpy()) and _same_bits(g.cpu().numpy(), g2.cpu().numpy())
    assert torch.isfinite(lp).all() and torch.isfinite(g).all() and torch.isfinite(red).all()
    # log_prob is the simulator's log_like, the tie and the prior
    x = pm.bij.forward(z)
    px = torch.stack([d["x"] for d in x["point_images"]], dim=1)
    py = torch.stack([d["y"] for d in x["point_images"]], dim=1)
    res = sim.fit_point_images(sim._pack_partial(x), px, py, obs, err)
    want = res["log_like"] + pm.log_prior(z).double()
    if sigma is not None:
        maps = sim._lens_maps(px.t().contiguous(), py.t().contiguous(), sim._pack_partial(x))
        want = want + _dev(sim, PI.tie(maps[0].t().double().cpu(), maps[1].t().double().cpu(), sigma))
    assert torch.allclose(lp.double(), want, rtol=1e-5, atol=1e-3)


def test_source_plane_tie_gradient(gl):  # noqa: F811
    """The tie term's hand-written gradient (lens_maps_vjp for the lens columns, (I - H)^T for the positions) against float64
    autograd of the restatement through the oracle's ray shooting."""
    from gigalens_amd.model import _SourcePlaneTieFn
    from oracle import ref_torch as ref
    c = PI.fit_case("quad")
    sim, packed, _ = _fit_run(gl, "quad")
    sigma = 0.02
    p = packed.clone().requires_grad_(True)
    x, y = _dev(sim, c["x"]).requires_grad_(True), _dev(sim, c["y"]).requires_grad_(True)
    t = _SourcePlaneTieFn.apply(p, x, y, sim, sigma)
    t.sum().backward()
    p64 = c["packed"].clone().requires_grad_(True)
    x64, y64 = (torch.as_tensor(c[k]).double().requires_grad_(True) for k in ("x", "y"))
    rs = ref.RefSimulator(PI.phys_model(), c["cam"]["cfg"], c["B"], dtype=PI.F64)
    bx, by = rs.beta(x64.t(), y64.t(), PI.struct_of(p64)["lens_mass"])
    want = PI.tie(bx.t(), by.t(), sigma) + (c["J"] - 1) * math.log(2.0 * math.pi * sigma ** 2)
    wp, wx, wy = torch.autograd.grad(want.sum(), [p64, x64, y64])
    assert torch.allclose(t.double().cpu(), want.detach(), rtol=1e-4, atol=1e-4)
    lens_cols = [k for k, s in enumerate(sim._layout.slots) if s[0] == "lens_mass"]
    for got, ref_g, what in ((p.grad[:, lens_cols], wp[:, lens_cols], "lens"), (x.grad, wx, "x"), (y.grad, wy, "y")):
        e = float(H.grad_col_err(got.cpu().numpy(), ref_g.numpy()).max())
        print(f"tie d/d{what}: {e:.3g} / {GRAD_RTOL_COL:g}")
        assert e <= GRAD_RTOL_COL
    other = [k for k in range(p.shape[1]) if k not in lens_cols]
    assert torch.all(p.grad[:, other] == 0)


@pytest.mark.parametrize("graph", [False, True])
def test_map_steps_raise_log_prob(gl, graph):  # noqa: F811
    from gigalens_amd.inference import Adam, ModellingSequence
    from gigalens_amd.model import PointImageProbModel
    phys, cfg, prior, truth, obs, err = _quasar(gl)
    B = 4
    pm = PointImageProbModel(prior, obs, err, source_plane_sigma=0.05)
    start = _start(prior, truth, B, 0.3)
    sim = gl.LensSimulator(phys, cfg, bs=B)
    lp0 = pm.log_prob(sim, pm.bij.inverse(start).to(sim.device))[0]
    seq = ModellingSequence(phys, pm, cfg)
    z = seq.MAP(Adam(lr=1e-3), start=start, n_samples=B, num_steps=30, graph=graph)
    lp1 = pm.log_prob(sim, torch.as_tensor(z).to(sim.device))[0]
    print(f"graph={graph}: log_prob {lp0.tolist()} -> {lp1.tolist()}")
    assert torch.isfinite(lp1).all() and bool((lp1 > lp0).all())
