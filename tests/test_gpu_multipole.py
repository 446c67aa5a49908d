"""The multipole lens on the GPU (csrc/gl_multipole.h through the interpreter kernel, the point kernels and the lens planes) against
the float64 restatement of tests/multipole_cases.py: parity of the pixel-grid modes (with PSF and supersampling, two multipoles beside
an SIE with a shapelet source, the linear solve), of the point entries and the three point likelihoods with their gradients, of a
two-plane model with the multipole on the far plane; the identities kappa = a_m C / (2 r), the lens equation at the solver's images,
time delays against the float64 Fermat potential, the Einstein radius of SIS + multipole; a centre exactly on a pixel node; refusals
(among them the gradient of the position term on lens planes).

Tolerances.  VALUES (images, log-likelihoods, maps): the yardstick is the same restatement run in float32 on the CPU against
float64; the gate is 4 x that yardstick, computed here and printed before it is asserted.  GRADIENTS: ``helpers.grad_gate`` with the
column tolerance of the parity tests and the float32 conditioning bound measured on this composition; at most 2 % of a case's gradient
elements may pass through the conditioning bound alone (tests/test_multipole_host.py checks without a GPU that the float32
restatement itself stays inside that cap on these inputs).  The gradients of the point likelihoods use the gate of their own tests,
``5e-4 scale + 1e-6`` per element (``mp_positions_cases.grad_gate``)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import interp_cases as IC
from tests import mp_positions_cases as PC
from tests import multipole_cases as MC
from tests.test_gpu_parity import GRAD_RTOL_COL, gl  # noqa: F401

pytestmark = pytest.mark.gpu

COND_CAP = MC.COND_CAP
# The fused log_prob is checked as log_prob - log_prior against the log-likelihood, a float32 difference: the prior has to stay of the
# likelihood's size or smaller for that difference to keep the likelihood's digits.  The rows of a case lie far apart (65 draws of
# every parameter), so the prior around their mean is wide: two scales of each parameter.
PRIOR_WIDTH = 2.0
CASES = MC.PIXEL_CASES
_CACHE = {}


def _case(name):
    """The case's workload, rows, observation, float64 expectations and float32 yardstick errors -- computed once, shared, unchanged."""
    if name not in _CACHE:
        _CACHE[name] = MC.pixel_data(name)
    return _CACHE[name]


def _sim(gl, c):
    return gl.LensSimulator(c["wl"].phys_model, c["wl"].sim_config, bs=c["packed"].shape[0], supersampled_kernel=c["psf"])


def _ll_grad(c, shift=None):
    return MC.loglike_and_grad(c["wl"], c["packed"], c["obs"], psf=c["psf"], grid_shift=shift, mask=c.get("mask"))[2]


def _vjp_grad(c, shift=None):
    return MC.image_vjp(c["wl"], c["packed"], c["cot"], psf=c["psf"], grid_shift=shift)[1]


def grad_ok(c, g, g_o, grad_fn, what):
    ok, rep = H.grad_gate(g, g_o, GRAD_RTOL_COL, lambda S: MC.conditioning_bound(c["wl"], lambda sh: grad_fn(c, sh), g_o, S))
    print(what, rep)
    assert ok, (what, rep)
    assert rep["conditioned"] <= COND_CAP * np.asarray(g_o).size, (what, rep)


def _lens_cols(phys):
    return sum(len(l.params) for l in phys.lenses)


def _value_ok(got, want, yard, what, floor=0.0):
    """``got`` within 4 x the float32 yardstick of ``want`` (both relative to max |want|); every figure is printed first."""
    scale = max(np.abs(want).max(), 1e-300)
    e, gate = np.abs(got - want).max() / scale, 4 * max(np.abs(yard - want).max() / scale, floor)
    print(what, "error", e, "gate", gate)
    assert e <= gate, (what, e, gate)


# ---------------------------------------------------------------------------------------------------
# 1. the pixel-grid modes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pixel_modes_match_float64(gl, name):
    """simulate, its VJP, the log-likelihood, the fused value-and-gradient and log_prob with a prior, stream and graph."""
    c = _case(name)
    wl, packed = c["wl"], c["packed"]
    sim = _sim(gl, c)
    dev = sim.device
    pd = packed.to(dev)
    im_gate, ll_gate = 4 * c["im_yard"], 4 * c["ll_yard"]
    print(name, "float32 yardstick: image", c["im_yard"], "of max|image|, log-likelihood", c["ll_yard"], "relative")
    img = sim._model.simulate_fwd(pd).cpu().numpy()
    assert "gl_main_kernel" in sim._model.last_main_kernel()
    e = np.abs(img - c["im"]).max() / np.abs(c["im"]).max()
    print(name, "image error", e, "gate", im_gate)
    assert e <= im_gate
    g_img = sim._model.simulate_bwd(pd, torch.as_tensor(c["cot"], device=dev)).cpu().numpy()
    grad_ok(c, g_img, c["g_img"], _vjp_grad, name + " simulate VJP")
    obs = torch.as_tensor(c["obs"], device=dev)
    ll0, _, _ = sim._model.loglike(pd, obs, None, None, wl.background_rms, wl.exp_time, False)
    ll1, _, g = sim._model.loglike(pd, obs, None, None, wl.background_rms, wl.exp_time, True)
    for ll in (ll0, ll1):
        e = (np.abs(ll.cpu().numpy() - c["ll"]) / np.maximum(np.abs(c["ll"]), 1.0)).max()
        print(name, "log-likelihood error", e, "gate", ll_gate)
        assert e <= ll_gate
    grad_ok(c, g.cpu().numpy(), c["g"], _ll_grad, name + " log-likelihood gradient")
    # log_prob with prior and bijectors, fused: stream, then graph replay
    prior = IC.prior_around(wl, packed, width=PRIOR_WIDTH)
    pm = gl.ForwardProbModel(prior, c["obs"], wl.background_rms, wl.exp_time, include_positions=False)
    struct = {k: v for k, v in H.struct_from_packed(wl.phys_model, pd).items() if v}
    z = pm.bij.inverse(struct).to(dev).contiguous()

    def chain(gp, with_prior=True):
        zz = z.detach().clone().requires_grad_(True)
        s = (pm._packed_from_x(sim, pm._flat.forward(zz)) * torch.as_tensor(gp, dtype=torch.float32, device=dev)).sum()
        if with_prior:
            s = s + pm.log_prior(zz).sum()
        return torch.autograd.grad(s, zz)[0].cpu().numpy()

    def z_bound(S):
        fin = np.abs(c["g"])
        Sp = np.maximum(fin.max(axis=0, keepdims=True), 1e-3 * fin.max())
        return np.abs(chain(MC.conditioning_bound(wl, lambda sh: _ll_grad(c, sh), c["g"], Sp) * Sp, with_prior=False)) / S
    want_gz = chain(c["g"])
    for graph in (False, True, True):  # (the second graph call replays the captured one)
        lp, red, gz = pm.log_prob_and_grad(sim, z, graph=graph)
        e = (np.abs((lp - pm.log_prior(z)).cpu().numpy() - c["ll"]) / np.maximum(np.abs(c["ll"]), 1.0)).max()
        print(name, "graph" if graph else "stream", "log_prob - log_prior error", e)
        assert e <= ll_gate + 2e-6  # (+ the float32 sum of a prior of the same size as the likelihood)
        assert np.allclose(red.cpu().numpy(), c["red"], rtol=max(ll_gate, 1e-5))
        ok, rep = H.grad_gate(gz.cpu().numpy(), want_gz, GRAD_RTOL_COL, z_bound)
        print(name, "log_prob gradient", rep)
        assert ok and rep["conditioned"] <= COND_CAP * want_gz.size, rep


@pytest.mark.parametrize("model,grid,m", [("ESM", "33x31", 4), ("SMM", "16x16", 4)])
def test_lstsq_solves_the_amplitudes(gl, model, grid, m):
    """``lstsq_simulate`` behind a multipole: coefficients and image against the float64 pinv, within the float32 solve's own bound
    20 eps cond + 1e-5 of the largest coefficient (tests/test_gpu_lstsq.py)."""
    wl, packed = MC.case(model, grid, m=m, use_lstsq=True)
    full_wl, _ = MC.case(model, grid, m=m)
    obs = MC.observation(full_wl, packed)
    err = np.sqrt(wl.background_rms ** 2 + np.clip(obs, 0, None) / wl.exp_time).astype(np.float32)
    c_o, img_o = MC.lstsq(wl, packed, obs, err)
    rs = MC.ref_sim(wl, 3)
    st = IC.expected_image(rs, H.struct_from_packed(wl.phys_model, packed.double()), stacked=True)
    depth = st.shape[-1]
    st = st.reshape(3, -1, depth) / torch.as_tensor(err).double().reshape(1, -1, 1)
    cond = torch.linalg.cond(st.transpose(1, 2) @ st).numpy()
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=3)
    assert sim._model.num_linear() == depth
    pd = packed.to(sim.device)
    coeffs = sim.lstsq_simulate(pd, obs, err, return_coeffs=True).cpu().numpy()
    image = sim.lstsq_simulate(pd, obs, err).cpu().numpy()
    assert "gl_main_kernel" in sim._model.last_main_kernel()
    for b in range(3):
        tol = 20 * 1.2e-7 * cond[b] + 1e-5
        scale = np.abs(c_o[b]).max()
        print("lstsq sample", b, "cond", cond[b], "error", np.abs(coeffs[b] - c_o[b]).max() / scale, "tol", tol)
        assert np.abs(coeffs[b] - c_o[b]).max() <= tol * scale
        assert np.abs(image[b] - img_o[b]).max() <= tol * depth * np.abs(img_o[b]).max()


def test_centre_on_a_pixel_node(gl):
    """The multipole's centre exactly on a pixel node (0, 0) of the 33 x 31 grid: every output and gradient is finite, and the float64
    parity holds on all other pixels -- the image and VJP with that pixel's cotangent zero, the likelihood with that pixel masked."""
    c = _case("node")
    wl, packed = c["wl"], c["packed"]
    sim = _sim(gl, c)
    dev = sim.device
    on = (sim.img_X == 0) & (sim.img_Y == 0)
    assert int(on.sum()) == 1
    node = np.unravel_index(int(torch.nonzero(on.reshape(-1))[0]), c["obs"].shape)
    assert c["mask"][node] and c["mask"].sum() == 1
    pd = packed.to(dev)
    img = sim._model.simulate_fwd(pd).cpu().numpy()
    assert np.isfinite(img).all()
    keep = ~c["mask"]
    e = np.abs(img - c["im"])[:, keep].max() / np.abs(c["im"]).max()
    print("node: image error off the node", e, "gate", 4 * c["im_yard"])
    assert e <= 4 * c["im_yard"]
    g_img = sim._model.simulate_bwd(pd, torch.as_tensor(c["cot"], device=dev)).cpu().numpy()  # (the node's cotangent is zero)
    assert np.isfinite(g_img).all()
    grad_ok(c, g_img, c["g_img"], _vjp_grad, "node simulate VJP")
    full = sim._model.simulate_bwd(pd, torch.ones_like(torch.as_tensor(c["cot"], device=dev)))
    assert torch.isfinite(full).all()
    obs = torch.as_tensor(c["obs"], device=dev)
    ll_all, _, g_all = sim._model.loglike(pd, obs, None, None, wl.background_rms, wl.exp_time, True)
    assert torch.isfinite(ll_all).all() and torch.isfinite(g_all).all()
    mask = torch.as_tensor(keep.astype(np.float32), device=dev)
    ll, _, g = sim._model.loglike(pd, obs, None, mask, wl.background_rms, wl.exp_time, True)
    e = (np.abs(ll.cpu().numpy() - c["ll"]) / np.maximum(np.abs(c["ll"]), 1.0)).max()
    print("node: log-likelihood error off the node", e, "gate", 4 * c["ll_yard"])
    assert e <= 4 * c["ll_yard"]
    grad_ok(c, g.cpu().numpy(), c["g"], _ll_grad, "node log-likelihood gradient")
    # the point entries at the centre itself: exact zeros from the multipole, finite everything
    lens = wl.phys_model.lenses[2]
    zero = torch.zeros(1, 1, device=dev)
    kw = dict(a_m=torch.tensor([0.03]), phi_m=torch.tensor([0.4]), center_x=torch.tensor([0.0]), center_y=torch.tensor([0.0]))
    ax, ay = lens.deriv(zero, zero, **kw)
    assert float(ax) == 0.0 and float(ay) == 0.0 and float(lens.potential(zero, zero, **kw)) == 0.0
    assert all(float(h) == 0.0 for h in lens.hessian(zero, zero, **kw))


# ---------------------------------------------------------------------------------------------------
# 2. the point entries
# ---------------------------------------------------------------------------------------------------
def _point_model(gl, model, m, B=3, seed=0):
    """A lens-only model with ``B`` rows: ``(phys, simulator, rows [B, P] float32 on the CPU)``."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    lenses = MC.lenses_of(model, m)
    r = np.random.default_rng(900 + seed + 7 * m + sum(map(ord, model)))
    rows = torch.tensor([MC.lens_row(lenses, r) for _ in range(B)], dtype=torch.float32)
    phys = PhysicalModel(lenses, [], [])
    return phys, gl.LensSimulator(phys, SimulatorConfig(delta_pix=0.1, num_pix=33), bs=B), rows


@pytest.mark.parametrize("model,m,B", [("ESM", 4, 3), ("SMM", 3, 3), ("ESM", 8, 65), ("EM", 2, 1)])
def test_point_entries_match_float64(gl, model, m, B):
    """``beta``, ``magnification``, ``convergence``, ``shear``, ``rotation``, ``potential``, the plugin level of the multipole itself,
    ``beta_vjp`` and ``hessian_vjp`` at scattered points: values within 4 x the float32 restatement's own error, gradients under the
    column gate with the conditioning bound of a one-ulp shift of the points.

    ``magnification`` is the one value here that is NOT gated at 4 x the float32 restatement's own error of the same quantity.  The four
    Hessian components are (as are convergence and shear); det A = (1 - f_xx)(1 - f_yy) - f_xy f_yx is a difference of products of
    them, and the restatement's error of det A, a maximum over fewer than a hundred points, is at rounding level in some cases and
    says nothing about an implementation whose Hessian errors are of the yardstick's size but fall differently: measured on an
    MI355X, EPL + Multipole(2), B = 1: |d det| 7.3e-7 of max |det A| against 4 x 1.2e-7, while every Hessian component of the same
    call is inside 4 x its yardstick; gated on mu itself (which adds the distance to the critical curve) EPL + Shear + Multipole(8),
    B = 65 measured 1.9e-3 against 1.2e-3.  So det A = 1 / mu is held to the Hessian's yardstick carried through the determinant to
    first order, |d det| <= (|1 - f_xx| + |1 - f_yy| + |f_xy| + |f_yx|) max |dH|, times the same 4, plus the rounding of the float32
    reciprocal the entry returns; the plain figure is printed beside it."""
    phys, sim, rows = _point_model(gl, model, m, B)
    dev = sim.device
    pd = rows.to(dev)
    r = np.random.default_rng(5 + m)
    n = 97
    x = np.float32(r.uniform(-1.6, 1.6, n)).astype(np.float64)
    y = np.float32(r.uniform(-1.6, 1.6, n)).astype(np.float64)
    keep = np.ones(n, dtype=bool)  # points a tenth of an arcsec from every centre: 1 / r and the EPL's core stay tame
    k = 0
    for lens in phys.lenses:
        if "center_x" in lens.params:
            i = lens.params.index("center_x")
            for b in range(B):
                keep &= np.hypot(x - float(rows[b, k + i]), y - float(rows[b, k + i + 1])) > 0.1
        k += len(lens.params)
    x, y = x[keep], y[keep]
    want = MC.lens_maps(phys, rows.double(), x, y).numpy()
    yard = MC.lens_maps(phys, rows, x, y, dtype=torch.float32).double().numpy()
    xt, yt = torch.as_tensor(x, dtype=torch.float32, device=dev)[:, None], torch.as_tensor(y, dtype=torch.float32, device=dev)[:, None]
    lp = MC.lens_dicts(phys, pd)
    bx, by = sim.beta(xt, yt, lp)
    _value_ok(np.stack([bx.cpu().numpy(), by.cpu().numpy()]), want[:2], yard[:2], f"{model}{m} beta")
    f = want[2:6]
    fy = yard[2:6]
    det = lambda h: (1 - h[0]) * (1 - h[3]) - h[1] * h[2]
    _value_ok(sim.convergence(xt, yt, lp).cpu().numpy(), 0.5 * (f[0] + f[3]), 0.5 * (fy[0] + fy[3]), f"{model}{m} convergence")
    g1, g2 = sim.shear(xt, yt, lp)
    _value_ok(np.stack([g1.cpu().numpy(), g2.cpu().numpy()]), np.stack([0.5 * (f[0] - f[3]), f[1]]),
              np.stack([0.5 * (fy[0] - fy[3]), fy[1]]), f"{model}{m} shear")
    hess = sim._lens_maps(xt, yt, pd)[2:].cpu().numpy()
    _value_ok(hess, f, fy, f"{model}{m} Hessian (f_xx, f_xy, f_yx, f_yy)")
    # magnification, through det A = 1 / mu (see the docstring for why its gate is derived from the Hessian's yardstick)
    amp = (np.abs(1 - f[0]) + np.abs(1 - f[3]) + np.abs(f[1]) + np.abs(f[2])).max()
    det_gate = 4 * (amp * np.abs(fy - f).max() + 6e-8 * np.abs(det(f)).max())
    e_det = np.abs(1 / sim.magnification(xt, yt, lp).cpu().numpy().astype(np.float64) - det(f)).max()
    print(f"{model}{m} det A = 1 / magnification: error", e_det, "gate", det_gate, "(the float32 restatement's own:", np.abs(det(fy) - det(f)).max(), ")")
    assert e_det <= det_gate
    rot = sim.rotation(xt, yt, lp).cpu().numpy()
    assert np.abs(rot).max() <= 4 * max(np.abs(fy[1] - fy[2]).max(), 1.2e-7 * np.abs(f).max())  # one plane: symmetric to rounding
    _value_ok(sim.potential(xt, yt, pd).cpu().numpy(), want[6], yard[6], f"{model}{m} potential")
    # plugin level: the multipole on its own
    li = max(i for i, l in enumerate(phys.lenses) if l.name == MC.NAME)
    lens = phys.lenses[li]
    one = type("P", (), dict(lenses=[lens]))()
    c0 = sum(len(l.params) for l in phys.lenses[:li])
    w1 = MC.lens_maps(one, rows[:, c0:c0 + 4].double(), x, y).numpy()
    y1 = MC.lens_maps(one, rows[:, c0:c0 + 4], x, y, dtype=torch.float32).double().numpy()
    kw = {n_: rows[:, c0 + i] for i, n_ in enumerate(lens.params)}
    ax, ay = lens.deriv(xt, yt, **kw)
    _value_ok(np.stack([ax.cpu().numpy(), ay.cpu().numpy()]), np.stack([x[:, None] - w1[0], y[:, None] - w1[1]]),
              np.stack([x[:, None] - y1[0], y[:, None] - y1[1]]), f"{model}{m} plugin deriv", floor=1.2e-7)
    hs = lens.hessian(xt, yt, **kw)
    _value_ok(np.stack([h.cpu().numpy() for h in hs]), w1[2:6], y1[2:6], f"{model}{m} plugin hessian")
    _value_ok(lens.potential(xt, yt, **kw).cpu().numpy(), w1[6], y1[6], f"{model}{m} plugin potential")
    # kappa = a_m C / (2 r), from the closed form in float64
    kap = lens.convergence(xt, yt, **kw).cpu().numpy()
    a, ph, cx, cy = (rows[:, c0 + i].double().numpy()[None, :] for i in range(4))
    rr, phi = np.hypot(x[:, None] - cx, y[:, None] - cy), np.arctan2(y[:, None] - cy, x[:, None] - cx)
    _value_ok(kap, a * np.cos(lens.m * (phi - ph)) / (2 * rr), 0.5 * (y1[2] + y1[5]), f"{model}{m} kappa identity")
    # beta_vjp and hessian_vjp: cotangents on every point, gradient on the lens columns
    cots = [torch.as_tensor(r.normal(size=(x.size, B)), dtype=torch.float32) for _ in range(6)]

    def vjp_ref(dx=0.0, dy=0.0, dtype=torch.float64):
        rw = rows.to(dtype).clone().requires_grad_(True)
        xs = torch.as_tensor(x + dx, dtype=dtype)[:, None].repeat(1, B).requires_grad_(True)
        ys = torch.as_tensor(y + dy, dtype=dtype)[:, None].repeat(1, B).requires_grad_(True)
        qx, qy, h, _ = MC.maps_of(phys, rw, xs, ys)
        cd = [t.to(dtype) for t in cots]
        gb = torch.autograd.grad((qx * cd[0] + qy * cd[1]).sum(), rw, retain_graph=True)[0].numpy()
        gh = torch.autograd.grad(sum((h[k] * cd[2 + k]).sum() for k in range(4)), rw)[0].numpy()
        return gb, gh
    gb_o, gh_o = vjp_ref()
    d = float(np.spacing(np.float32(1.6)))

    def bound(which):
        def fn(S):
            out = 0
            for sx, sy in ((d, d), (d, -d)):
                out = np.maximum(out, np.abs(vjp_ref(sx, sy)[which] - (gb_o, gh_o)[which]) / S)
            return out
        return fn
    gb = sim.beta_vjp(xt, yt, pd, cots[0].to(dev), cots[1].to(dev)).cpu().numpy()
    gh = sim.hessian_vjp(xt, yt, pd, *[t.to(dev) for t in cots[2:]]).cpu().numpy()
    for got_, want_, which, what in ((gb, gb_o, 0, "beta_vjp"), (gh, gh_o, 1, "hessian_vjp")):
        ok, rep = H.grad_gate(got_, want_, GRAD_RTOL_COL, bound(which))
        print(model, m, what, rep)
        assert ok and rep["conditioned"] <= COND_CAP * want_.size, (what, rep)


@pytest.mark.parametrize("m", [3, 4, 8])
def test_point_likelihoods_match_float64(gl, m):
    """``stats_positions``, ``stats_fluxes`` and ``stats_time_delays`` of EPL + Shear + Multipole(m) with their gradients (autograd
    through the entries) on a four-image family (``multipole_cases.point_family``): values within 4 x the float32 restatement's
    error, every gradient element within ``5e-4 scale + 1e-6``."""
    from tests.test_gpu_multilens_grad import _prior_of
    phys, sim, rows = _point_model(gl, "ESM", m, 3, seed=1)
    fam = MC.point_family(phys, rows)
    assert fam["x"].size == 4
    lp0 = {"lens_mass": [{n_: rows[:, c0 + i].numpy() for i, n_ in enumerate(l.params)}
                         for l, c0 in zip(phys.lenses, np.cumsum([0] + [len(l.params) for l in phys.lenses[:-1]]))]}
    pm = gl.ForwardProbModel(_prior_of(lp0), include_pixels=False, centroids_x=[fam["x"]], centroids_y=[fam["y"]],
                             centroids_errors_x=[fam["ex"]], centroids_errors_y=[fam["ey"]], centroids_fluxes=[fam["flux"]],
                             centroids_fluxes_errors=[fam["flux_err"]], centroids_time_delays=[fam["delay"]],
                             centroids_time_delays_errors=[fam["delay_err"]], time_delay_distances=[None])
    refs = {"positions": (lambda dt: MC.stats_positions(phys, None, rows, [fam], dt), pm.stats_positions),
            "fluxes": (lambda dt: MC.stats_fluxes(phys, rows, [fam], dt), pm.stats_fluxes),
            "time delays": (lambda dt: MC.stats_time_delays(phys, rows, [fam], dt), pm.stats_time_delays)}
    for what, (ref_fn, entry) in refs.items():
        ll_o, g_o = ref_fn(torch.float64)
        ll_y, _ = ref_fn(torch.float32)
        p = rows.to(sim.device).clone().requires_grad_(True)
        ll, _ = entry(sim, p)
        (g,) = torch.autograd.grad(ll.sum(), p)
        e, yard = PC.MC.rel_err(ll.detach().cpu().numpy(), ll_o), PC.MC.rel_err(ll_y, ll_o)
        worst = PC.grad_gate(g.cpu().numpy(), g_o)
        print(f"m={m} {what}: log_like error {e:.3e} (float32 yardstick {yard:.3e}), gradient worst element {worst:.3f} of the gate")
        assert torch.isfinite(g).all()
        assert e <= 4 * yard
        assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------
# 3. identities
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 4])
def test_images_solve_the_float64_lens_equation_and_delays_follow_fermat(gl, m):
    """``image_positions`` of a source behind EPL + Multipole(m): every image maps back to the source in float64 within the solver's
    stated tolerance (8 eps of the window's largest coordinate) plus the float32 rounding of beta itself (as much again);
    ``time_delays`` equal the float64 Fermat-potential excess at those images within float32 rounding of the potential's terms."""
    phys, sim, rows = _point_model(gl, "EM", m, 3, seed=2)
    src = (0.05, 0.03)
    x, y, mu, n, dt = sim.time_delays(rows.to(sim.device), torch.full((3,), src[0]), torch.full((3,), src[1]), strict=True)
    window = max(abs(float(sim.img_X.min())), abs(float(sim.img_X.max())), abs(float(sim.img_Y.min())), abs(float(sim.img_Y.max())))
    tol = 2 * sim.IMAGE_TOL_EPS * float(np.finfo(np.float32).eps) * window
    for b in range(3):
        k = int(n[b, 0])
        assert k >= 2
        xs, ys = x[b, 0, :k].cpu().numpy().astype(np.float64), y[b, 0, :k].cpu().numpy().astype(np.float64)
        maps = MC.lens_maps(phys, rows[b:b + 1].double(), xs, ys).numpy()[:, :, 0]
        miss = np.hypot(maps[0] - np.float32(src[0]), maps[1] - np.float32(src[1])).max()
        print(f"m={m} sample {b}: {k} images, largest |beta - beta_s| {miss:.3e}, tolerance {tol:.3e}")
        assert miss <= tol
        phi = 0.5 * ((xs - np.float32(src[0])) ** 2 + (ys - np.float32(src[1])) ** 2) - maps[6]
        want = phi - phi.min()
        # float32 psi and the float32 result: rounding of terms of size max(|theta|^2 / 2, |psi|)
        bound = 8 * 6e-8 * max(np.abs(maps[6]).max(), 0.5 * window ** 2)
        e = np.abs(dt[b, 0, :k].cpu().numpy() - want).max()
        print(f"m={m} sample {b}: time-delay error {e:.3e} arcsec^2, bound {bound:.3e}")
        assert e <= bound


@pytest.mark.parametrize("m", [3, 4])
def test_einstein_radius_of_sis_plus_multipole(gl, m):
    """The tangential critical curve of SIS + multipole is r(phi) = theta_E - a_m C(phi) to first order in a_m (det A = 1 - (theta_E
    - a_m C) / r exactly, the Hessian being (.) t t^T for both); its area is pi theta_E^2 + (pi / 2) a_m^2 -- the first-order term
    integrates to zero -- so the effective radius is theta_E (1 + a_m^2 / (4 theta_E^2)).  Bound: that closed form against the
    contour's own discretisation error, chords of cells of side h inside a curve of radius R: relative area deficit <= h^2 / (8 R^2)
    per chord, here doubled for the marching-squares vertices."""
    phys, sim, rows = _point_model(gl, "SM", m, 3, seed=3)
    te = sim.einstein_radius(rows.to(sim.device), strict=True).cpu().numpy()
    th, a = rows[:, 0].double().numpy(), rows[:, 3].double().numpy()
    want = np.sqrt(th ** 2 + 0.5 * a ** 2)
    h = (float(sim.img_X.max()) - float(sim.img_X.min())) / (2 * 33)
    bound = 2 * h ** 2 / (8 * th ** 2) * th + 1e-6
    print(f"m={m}: Einstein radius {te}, theta_E {th}, closed form {want}, bound {bound}")
    assert (np.abs(te - want) <= bound).all()
    assert (np.abs(te - th) <= bound + 0.25 * a ** 2 / th).all()


# ---------------------------------------------------------------------------------------------------
# 4. lens planes
# ---------------------------------------------------------------------------------------------------
def test_two_planes_with_the_multipole_on_the_far_plane(gl):
    """EPL + Shear at z = 0.5, SIE + Multipole(4) at z = 1.0, a Sersic source at z = 3: ``simulate``, the fused ``log_prob_and_grad`` and
    the value of the position term against the float64 trace of tests/multipole_cases.py."""
    from tests.test_gpu_multilens_grad import _prior_of
    c = _case("planes")
    wl, packed, mp = c["wl"], c["packed"], c["mp"]
    sim = _sim(gl, c)
    dev = sim.device
    pd = packed.to(dev)
    img = sim.simulate(pd).cpu().numpy()
    e = np.abs(img - c["im"]).max() / np.abs(c["im"]).max()
    print("planes: image error", e, "gate", 4 * c["im_yard"])
    assert e <= 4 * c["im_yard"]
    prior = IC.prior_around(wl, packed, width=PRIOR_WIDTH)
    pm = gl.ForwardProbModel(prior, c["obs"], wl.background_rms, wl.exp_time, include_positions=False)
    struct = {k: v for k, v in H.struct_from_packed(wl.phys_model, pd).items() if v}
    z = pm.bij.inverse(struct).to(dev).contiguous()

    def chain(gp, with_prior=True):
        zz = z.detach().clone().requires_grad_(True)
        s = (pm._packed_from_x(sim, pm._flat.forward(zz)) * torch.as_tensor(gp, dtype=torch.float32, device=dev)).sum()
        if with_prior:
            s = s + pm.log_prior(zz).sum()
        return torch.autograd.grad(s, zz)[0].cpu().numpy()

    def z_bound(S):
        fin = np.abs(c["g"])
        Sp = np.maximum(fin.max(axis=0, keepdims=True), 1e-3 * fin.max())
        return np.abs(chain(MC.conditioning_bound(wl, lambda sh: _ll_grad(c, sh), c["g"], Sp) * Sp, with_prior=False)) / S
    want_gz = chain(c["g"])
    for graph in (False, True):
        lp, red, gz = pm.log_prob_and_grad(sim, z, graph=graph)
        e = (np.abs((lp - pm.log_prior(z)).cpu().numpy() - c["ll"]) / np.maximum(np.abs(c["ll"]), 1.0)).max()
        print("planes", "graph" if graph else "stream", "log_prob - log_prior error", e, "gate", 4 * c["ll_yard"] + 2e-6)
        assert e <= 4 * c["ll_yard"] + 2e-6
        ok, rep = H.grad_gate(gz.cpu().numpy(), want_gz, GRAD_RTOL_COL, z_bound)
        print("planes log_prob gradient", rep)
        assert ok and rep["conditioned"] <= COND_CAP * want_gz.size, rep
    # the position term: a ring of four images behind both planes
    nl = _lens_cols(wl.phys_model)
    fam = PC.family(mp, 3.0, (11, -9, 2, -3), (2, 3, -10, 9), 0.01)
    ll_o, g_o = MC.stats_positions(wl.phys_model, mp, packed[:, :nl], [fam])
    ll_y, _ = MC.stats_positions(wl.phys_model, mp, packed[:, :nl], [fam], torch.float32)
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.cosmology import MultiPlane
    phys_l = PhysicalModel(wl.phys_model.lenses, [], [], multiplane=MultiPlane(list(MC.Z_PLANES), [], MC.Z_SOURCE))
    sim_l = gl.LensSimulator(phys_l, wl.sim_config, bs=3)
    lp0 = {"lens_mass": [{k: v.numpy() for k, v in d.items()} for d in MC.lens_dicts(phys_l, packed[:, :nl])]}
    pmp = gl.ForwardProbModel(_prior_of(lp0), include_pixels=False, centroids_x=[fam["x"]], centroids_y=[fam["y"]],
                              centroids_errors_x=[fam["ex"]], centroids_errors_y=[fam["ey"]], centroids_redshifts=[fam["z"]])
    ll, _ = pmp.stats_positions(sim_l, packed[:, :nl].to(dev))
    e, yard = PC.MC.rel_err(ll.cpu().numpy(), ll_o), PC.MC.rel_err(ll_y, ll_o)
    print(f"planes positions: log_like error {e:.3e} (float32 yardstick {yard:.3e})")
    assert e <= 4 * yard
    # its gradient is refused: the multi-plane gradient kernel of the point likelihoods is built without the case (with it the
    # kernel spills registers); the refused call leaves the model as it was
    from gigalens_amd import _native
    p = packed[:, :nl].to(dev).clone().requires_grad_(True)
    with pytest.raises(_native.UnsupportedLensError, match="MULTIPOLE"):
        ll_g, _ = pmp.stats_positions(sim_l, p)
        torch.autograd.grad(ll_g.sum(), p)
    assert torch.equal(pmp.stats_positions(sim_l, packed[:, :nl].to(dev))[0], ll)


# ---------------------------------------------------------------------------------------------------
# 5. refusals and limits
# ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_as_it_was(gl):
    """A multipole beside a user-written ``hip_body`` profile is refused with ``UnsupportedLensError``, a ScalingRelation over a
    multipole inside a model with ``NativeLibraryError`` (the rule for a base without a fused kernel or a body); an order outside 2..8 never reaches the library; after a refused call a model computes what it did."""
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass import Multipole
    from gigalens_amd.profiles.mass.scaling_relation import ScalingRelation
    c = _case("ESM2-16x16-B1")
    sim = _sim(gl, c)
    pd = c["packed"].to(sim.device)
    before = sim._model.simulate_fwd(pd).clone()

    class Body(MassProfile):
        _name = "BODY"
        _params = ["k"]
        hip_body = "template <class R> __device__ void deriv(R x, R y, const R* p, R& fx, R& fy) { fx = p[0] * x; fy = p[0] * y; }"
    cfg = c["wl"].sim_config
    with pytest.raises(_native.UnsupportedLensError, match="MULTIPOLE"):
        gl.LensSimulator(PhysicalModel([Body(), Multipole(4)], [], [Sersic()]), cfg, bs=1)
    cat = {"lum": [1.0, 0.5], "center_x": [0.3, -0.2], "center_y": [0.1, 0.4], "phi_m": [0.0, 0.3]}
    with pytest.raises(_native.NativeLibraryError, match="plugin level only"):
        gl.LensSimulator(PhysicalModel([ScalingRelation(Multipole(4), ["a_m"], 1.0, {"a_m": 0.5}, cat)], [], [Sersic()]), cfg, bs=1)
    with pytest.raises(ValueError):
        Multipole(1)
    bad = Multipole(4)
    bad.m = 9  # past the Python check: gl_model_create answers GL_EINVAL
    with pytest.raises(_native.NativeLibraryError, match="multipole order"):
        gl.LensSimulator(PhysicalModel([bad], [], [Sersic()]), cfg, bs=1)
    assert torch.equal(sim._model.simulate_fwd(pd), before)
