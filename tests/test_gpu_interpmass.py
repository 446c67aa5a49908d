"""The interpolated lens on the GPU (csrc/gl_interp_mass.h through the interpreter kernel and the point kernels) against the float64
restatement of tests/interpmass_cases.py: equality with the built-in Shear, parity of the pixel-grid modes (with PSF and
supersampling, a ragged pixel region, per-source deflection scales, two interpolated lenses beside an SIE) and of the point entries,
the lens-equation solver and the critical curves against a float64 solve of the same interpolant, the apron edges and the refusals.

Tolerances.  VALUES (images, log-likelihoods, maps): the yardstick is the same restatement run in float32 on the CPU; the gate is
4 x its worst error relative to each case's own scale over the cases of this file (4: the kernel may order its 16-tap sum and fused
multiply-adds differently), printed before it is asserted.  GRADIENTS: ``helpers.grad_gate`` with the column tolerance of the
reduced-size parity tests and the float32 conditioning bound measured on this composition; at most 5 % of a case's gradient
elements may pass through the conditioning bound alone (the float32 restatement itself stays inside that cap on these inputs)."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import interp_cases as IC
from tests import interpmass_cases as MC
from tests.test_gpu_parity import GRAD_RTOL_COL, gl  # noqa: F401

pytestmark = pytest.mark.gpu

PSF = IC.gauss_psf(3, 0.8)
REGION = (np.hypot(*np.mgrid[-16:17, -15:16]) < 13).astype(np.float32)  # 33 x 31: a disc (ragged pixel list)
# name -> (model, grid, keyword arguments of interpmass_cases.case, supersampled PSF)
CASES = {
    "I-7x9": ("I", "7x9", dict(maps="5x4"), None),
    "IS-33x31": ("IS", "33x31", dict(maps="9x7"), None),
    "I-7x9-ss2-psf": ("I", "7x9", dict(maps="9x7", supersample=2), PSF),
    "IS-33x31-region": ("IS", "33x31", dict(maps="5x4", pix_region=REGION), None),
    "I2-33x31-scales": ("I2", "33x31", dict(maps="9x7", scales=(0.6, 1.3)), None),
    "IIS-7x9": ("IIS", "7x9", {}, None),
}
COND_CAP = 0.05  # share of a case's gradient elements that may pass through the conditioning bound alone
_CACHE = {}


def _case(name):
    """The case's workload, rows, observation, float64 expectations and float32 yardstick errors -- computed once, shared, unchanged."""
    if name not in _CACHE:
        model, grid, kw, psf = CASES[name]
        wl, packed = MC.case(model, grid, **kw)
        obs = MC.observation(wl, packed, psf)
        r = np.random.default_rng(3)
        cot = r.normal(size=(3,) + obs.shape).astype(np.float32)
        ll, red, g, im = MC.loglike_and_grad(wl, packed, obs, psf=psf)
        ll32, _, g32, im32 = MC.loglike_and_grad(wl, packed, obs, dtype=torch.float32, psf=psf)
        _, g_img = MC.image_vjp(wl, packed, cot, psf=psf)
        _CACHE[name] = dict(wl=wl, packed=packed, obs=obs, psf=psf, cot=cot, ll=ll, red=red, g=g, im=im, g_img=g_img, g32=g32,
                            im_yard=np.abs(im32 - im).max() / np.abs(im).max(), ll_yard=(np.abs(ll32 - ll) / np.maximum(np.abs(ll), 1.0)).max())
    return _CACHE[name]


@pytest.fixture(scope="module")
def gates():
    """4 x the worst float32-restatement error over this file's cases: (image gate, log-likelihood gate), both relative."""
    im = max(_case(n)["im_yard"] for n in CASES)
    ll = max(_case(n)["ll_yard"] for n in CASES)
    print(f"float32 yardstick maxima over {len(CASES)} cases: image {im:.3e} of max|image|, log-likelihood {ll:.3e} relative")
    return 4 * im, 4 * ll


def _sim(gl, c):
    return gl.LensSimulator(c["wl"].phys_model, c["wl"].sim_config, bs=3, supersampled_kernel=c["psf"])


def _ll_grad(c, shift=None):
    return MC.loglike_and_grad(c["wl"], c["packed"], c["obs"], psf=c["psf"], grid_shift=shift)[2]


def _vjp_grad(c, shift=None):
    return MC.image_vjp(c["wl"], c["packed"], c["cot"], psf=c["psf"], grid_shift=shift)[1]


def grad_ok(c, g, g_o, grad_fn, what):
    ok, rep = H.grad_gate(g, g_o, GRAD_RTOL_COL, lambda S: MC.conditioning_bound(c["wl"], lambda sh: grad_fn(c, sh), g_o, S))
    print(what, rep)
    assert ok, (what, rep)
    assert rep["conditioned"] <= COND_CAP * np.asarray(g_o).size, (what, rep)


def _lens_cols(phys):
    return sum(len(l.params) for l in phys.lenses)


def _mesh(sim, n=None):
    """The simulator's own grid points (float32, as the device holds them) as float64 numpy arrays."""
    return sim.img_X.cpu().numpy().astype(np.float64).reshape(-1), sim.img_Y.cpu().numpy().astype(np.float64).reshape(-1)


# ---------------------------------------------------------------------------------------------------
# 1. equality with the built-in Shear
# ---------------------------------------------------------------------------------------------------
def test_equals_the_builtin_shear(gl):
    """Maps sampled from a shear, the grid inside 1 <= u <= W - 2: simulate, all six rows of the lens maps and the log-likelihood with
    its gradient equal those of the built-in Shear.  Keys' kernel is exact on a linear field, so the two differ by float32 rounding
    of the sixteen-tap sum: images and log-likelihoods under this file's value rule against the Shear model's own float64
    expectation, the source gradient under the gradient rule; d/d scale_factor against the directional derivative
    gamma . d/d gamma of the Shear model (alpha is linear in both)."""
    from gigalens_amd import workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass import Interpolated
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    g1, g2, n, pitch = 0.125, -0.0625, (7, 9), 0.125
    ax, ay = MC.sampled((11, 13), pitch, lambda X, Y: (g1 * X + g2 * Y, g2 * X - g1 * Y))  # +-0.75 x +-0.625 arcsec: the field is +-0.45
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=n)
    src = [0.2, 1.5, 0.03, -0.02, 30.0]
    wl_i = workloads.Workload("IM-shear", PhysicalModel([Interpolated(ax, ay, pitch)], [], [Sersic()]), None, cfg, 3)
    wl_s = workloads.Workload("shear", PhysicalModel([Shear()], [], [Sersic()]), None, cfg, 3)
    sf = [1.0, 0.7, 1.3]
    rows_i = torch.tensor([[s, 0.0, 0.0] + src for s in sf], dtype=torch.float32)
    rows_s = torch.tensor([[s * g1, s * g2] + src for s in sf], dtype=torch.float32)
    obs = IC.observation(wl_s, rows_s)
    ll_o, _, g_o, im_o = IC.loglike_and_grad(wl_s, rows_s, obs)
    ll32, _, _, im32 = IC.loglike_and_grad(wl_s, rows_s, obs, dtype=torch.float32)
    im_gate = 4 * np.abs(im32 - im_o).max() / np.abs(im_o).max()
    ll_gate = 4 * (np.abs(ll32 - ll_o) / np.maximum(np.abs(ll_o), 1.0)).max()
    sim_i, sim_s = gl.LensSimulator(wl_i.phys_model, cfg, bs=3), gl.LensSimulator(wl_s.phys_model, cfg, bs=3)
    dev = sim_i.device
    u = (sim_i.img_X.cpu().numpy() / pitch + 6)
    assert u.min() >= 1 and u.max() <= 11
    im_i = sim_i._model.simulate_fwd(rows_i.to(dev)).cpu().numpy()
    im_s = sim_s._model.simulate_fwd(rows_s.to(dev)).cpu().numpy()
    assert "gl_main_kernel" in sim_i._model.last_main_kernel()
    for im in (im_i, im_s):
        e = np.abs(im - im_o).max() / np.abs(im_o).max()
        print("image error", e, "gate", im_gate)
        assert e <= im_gate
    maps_i = sim_i._model.lens_maps(rows_i.to(dev), sim_i.img_X[:, None], sim_i.img_Y[:, None]).cpu().numpy()
    maps_s = sim_s._model.lens_maps(rows_s.to(dev), sim_s.img_X[:, None], sim_s.img_Y[:, None]).cpu().numpy()
    # beta: float32 rounding of a sum of sixteen products of size <= 0.15; Hessian: the same sum over 1 / pitch
    assert np.abs(maps_i[:2] - maps_s[:2]).max() <= 32 * 6e-8 * 0.15
    assert np.abs(maps_i[2:] - maps_s[2:]).max() <= 32 * 6e-8 * 0.15 / pitch
    o = torch.as_tensor(obs, device=dev)
    ll_i, _, gi = sim_i._model.loglike(rows_i.to(dev), o, None, None, wl_i.background_rms, wl_i.exp_time, True)
    e = (np.abs(ll_i.cpu().numpy() - ll_o) / np.maximum(np.abs(ll_o), 1.0)).max()
    print("log-likelihood error", e, "gate", ll_gate)
    assert e <= ll_gate
    gi = gi.cpu().numpy()
    want = np.concatenate([(g_o[:, 0] * rows_s[:, 0].numpy() + g_o[:, 1] * rows_s[:, 1].numpy())[:, None] / np.asarray(sf)[:, None],
                           g_o[:, 2:]], axis=1)
    got = np.concatenate([gi[:, :1], gi[:, 3:]], axis=1)
    c = dict(wl=wl_s, packed=rows_s, obs=obs, psf=None)
    def shear_grad(c, shift=None):
        g = IC.loglike_and_grad(wl_s, rows_s, obs, grid_shift=shift)[2]
        return np.concatenate([(g[:, 0] * rows_s[:, 0].numpy() + g[:, 1] * rows_s[:, 1].numpy())[:, None] / np.asarray(sf)[:, None], g[:, 2:]], axis=1)
    ok, rep = H.grad_gate(got, want, GRAD_RTOL_COL, lambda S: IC.conditioning_bound(wl_s, lambda sh: shear_grad(c, sh), want, S))
    print("gradient", rep)
    assert ok and rep["conditioned"] <= COND_CAP * want.size, rep


# ---------------------------------------------------------------------------------------------------
# 2. parity of the pixel-grid modes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pixel_modes_match_float64(gl, gates, name):
    """simulate, its VJP, the log-likelihood, the fused value-and-gradient and log_prob with a prior, stream and graph."""
    c = _case(name)
    wl, packed = c["wl"], c["packed"]
    sim = _sim(gl, c)
    dev = sim.device
    pd = packed.to(dev)
    im_gate, ll_gate = gates
    img = sim._model.simulate_fwd(pd).cpu().numpy()
    assert "gl_main_kernel" in sim._model.last_main_kernel()
    e = np.abs(img - c["im"]).max() / np.abs(c["im"]).max()
    print(name, "image error", e, "gate", im_gate)
    assert e <= im_gate
    g_img = sim._model.simulate_bwd(pd, torch.as_tensor(c["cot"], device=dev)).cpu().numpy()
    grad_ok(c, g_img, c["g_img"], _vjp_grad, name + " simulate VJP")
    obs = torch.as_tensor(c["obs"], device=dev)
    mask = sim.img_region if wl.sim_config.pix_region is not None else None
    ll0, _, _ = sim._model.loglike(pd, obs, None, mask, wl.background_rms, wl.exp_time, False)
    ll1, _, g = sim._model.loglike(pd, obs, None, mask, wl.background_rms, wl.exp_time, True)
    for ll in (ll0, ll1):
        e = (np.abs(ll.cpu().numpy() - c["ll"]) / np.maximum(np.abs(c["ll"]), 1.0)).max()
        print(name, "log-likelihood error", e, "gate", ll_gate)
        assert e <= ll_gate
    grad_ok(c, g.cpu().numpy(), c["g"], _ll_grad, name + " log-likelihood gradient")
    # log_prob with prior and bijectors, fused: stream, then graph
    prior = IC.prior_around(wl, packed)
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
        print(name, "graph" if graph else "stream", "log_prob - log_prior error", e)
        assert e <= ll_gate + 2e-6  # (+ the float32 sum of a prior of the same size as the likelihood)
        assert np.allclose(red.cpu().numpy(), c["red"], rtol=max(ll_gate, 1e-5))
        ok, rep = H.grad_gate(gz.cpu().numpy(), want_gz, GRAD_RTOL_COL, z_bound)
        print(name, "log_prob gradient", rep)
        assert ok and rep["conditioned"] <= COND_CAP * want_gz.size, rep


# ---------------------------------------------------------------------------------------------------
# 2. (continued) the point entries and the plugin level
# ---------------------------------------------------------------------------------------------------
def _clear_of_nodes(phys, rows, x, y, min_px=1e-3):
    """True where ``(x, y)`` keeps ``min_px`` map pixels from every node line of every interpolated lens, for every row."""
    ok = np.ones(x.shape, dtype=bool)
    k = 0
    for lens in phys.lenses:
        if lens.name == MC.NAME:
            h, w = lens.alpha_x.shape
            for b in range(rows.shape[0]):
                u = (x - float(rows[b, k + 1])) / lens.pitch + 0.5 * (w - 1)
                v = (y - float(rows[b, k + 2])) / lens.pitch + 0.5 * (h - 1)
                ok &= (np.abs(u - np.round(u)) >= min_px) & (np.abs(v - np.round(v)) >= min_px)
        k += len(lens.params)
    return ok


@pytest.mark.parametrize("name", ["I-7x9", "IIS-7x9"])
def test_point_entries_match_float64(gl, name):
    """lens_maps (all six rows), the plugin ``deriv`` / ``hessian``, ``stats_positions`` with its gradient, ``beta_vjp`` and
    ``hessian_vjp`` at points inside the maps, in their apron and beyond.  Value gate: 4 x the float32 restatement's own error."""
    c = _case(name)
    wl, packed = c["wl"], c["packed"]
    phys = wl.phys_model
    nl = _lens_cols(phys)
    sim = _sim(gl, c)
    dev = sim.device
    pd = packed.to(dev)
    r = np.random.default_rng(5)
    half = 0.5 * MC.DELTA_PIX * 7
    x = np.float32(r.uniform(-1.6 * half, 1.6 * half, 160)).astype(np.float64)
    y = np.float32(r.uniform(-1.6 * half, 1.6 * half, 160)).astype(np.float64)
    keep = _clear_of_nodes(phys, packed.numpy().astype(np.float64), x, y)  # second derivatives jump on the node lines
    x, y = x[keep], y[keep]
    want = MC.lens_maps(phys, packed[:, :nl].double(), x, y).numpy()
    yard = MC.lens_maps(phys, packed[:, :nl], x, y, dtype=torch.float32).numpy()
    xt, yt = torch.as_tensor(x, dtype=torch.float32, device=dev)[:, None], torch.as_tensor(y, dtype=torch.float32, device=dev)[:, None]
    got = sim._model.lens_maps(pd, xt, yt).cpu().numpy()
    for rows_, what in ((slice(0, 2), "beta"), (slice(2, 6), "Hessian")):
        scale = np.abs(want[rows_]).max()
        gate = 4 * np.abs(yard[rows_] - want[rows_]).max() / scale
        e = np.abs(got[rows_] - want[rows_]).max() / scale
        print(name, what, "error", e, "gate", gate)
        assert e <= gate
    assert not np.array_equal(want[3], want[4])  # f_xy and f_yx differ (node noise): neither is symmetrised
    # plugin level: the first interpolated lens on its own
    lens = phys.lenses[0]
    kw = {n: packed[:, i] for i, n in enumerate(lens.params)}
    ax, ay = lens.deriv(xt, yt, **kw)
    hs = lens.hessian(xt, yt, **kw)
    one = type("P", (), dict(lenses=[lens]))()
    w1 = MC.lens_maps(one, packed[:, :3].double(), x, y).numpy()
    y1 = MC.lens_maps(one, packed[:, :3], x, y, dtype=torch.float32).numpy()
    sc = np.abs(np.stack([x[:, None] - w1[0], y[:, None] - w1[1]])).max()
    gate = 4 * max(np.abs(y1[:2] - w1[:2]).max() / sc, 1e-7)
    e = max(np.abs(ax.cpu().numpy() - (x[:, None] - w1[0])).max(), np.abs(ay.cpu().numpy() - (y[:, None] - w1[1])).max()) / sc
    print(name, "plugin deriv error", e, "gate", gate)
    assert e <= gate
    sc = np.abs(w1[2:]).max()
    gate = 4 * np.abs(y1[2:] - w1[2:]).max() / sc
    e = max(np.abs(hs[k].cpu().numpy() - w1[2 + k]).max() for k in range(4)) / sc
    print(name, "plugin hessian error", e, "gate", gate)
    assert e <= gate
    # beta_vjp and hessian_vjp: cotangents on every point, gradient on the lens columns
    cots = [torch.as_tensor(r.normal(size=(x.size, 3)), dtype=torch.float32) for _ in range(6)]

    def vjp_ref(dx=0.0, dy=0.0, dtype=torch.float64):
        rows = packed[:, :nl].to(dtype).clone().requires_grad_(True)
        xs = torch.as_tensor(x + dx, dtype=dtype)[:, None].repeat(1, 3).requires_grad_(True)
        ys = torch.as_tensor(y + dy, dtype=dtype)[:, None].repeat(1, 3).requires_grad_(True)
        bx, by, h = MC.maps_of(phys, rows, xs, ys)
        cd = [t.to(dtype) for t in cots]
        gb = torch.autograd.grad((bx * cd[0] + by * cd[1]).sum(), rows, retain_graph=True)[0].numpy()
        gh = torch.autograd.grad(sum((h[k] * cd[2 + k]).sum() for k in range(4)), rows)[0].numpy()
        return gb, gh
    gb_o, gh_o = vjp_ref()
    d = float(np.spacing(np.float32(1.6 * half)))

    def bound(which):
        def f(S):
            out = 0
            for sx, sy in ((d, d), (d, -d)):
                out = np.maximum(out, np.abs(vjp_ref(sx, sy)[which] - (gb_o, gh_o)[which]) / S)
            return out
        return f
    gb = sim.beta_vjp(xt, yt, pd, cots[0].to(dev), cots[1].to(dev)).cpu().numpy()[:, :nl]
    gh = sim.hessian_vjp(xt, yt, pd, *[t.to(dev) for t in cots[2:]]).cpu().numpy()[:, :nl]
    for got_, want_, which, what in ((gb, gb_o, 0, "beta_vjp"), (gh, gh_o, 1, "hessian_vjp")):
        ok, rep = H.grad_gate(got_, want_, GRAD_RTOL_COL, bound(which))
        print(name, what, rep)
        assert ok and rep["conditioned"] <= COND_CAP * want_.size, (what, rep)
    # the position likelihood of one family of four images with its gradient
    pick = np.argsort(np.hypot(x, y))[:40:10]
    cx, cy = np.float32(x[pick]), np.float32(y[pick])
    ex = ey = np.full(4, 0.01, dtype=np.float32)
    ll_o, g_o = MC.stats_positions(phys, packed[:, :nl], cx, cy, ex, ey)
    ll_y, _ = MC.stats_positions(phys, packed[:, :nl], cx, cy, ex, ey, dtype=torch.float32)
    sim._model.set_positions([cx], [cy], [ex], [ey])
    ll, _, g = sim._model.positions(pd, True)
    gate = 4 * (np.abs(ll_y - ll_o) / np.maximum(np.abs(ll_o), 1.0)).max()
    e = (np.abs(ll.cpu().numpy() - ll_o) / np.maximum(np.abs(ll_o), 1.0)).max()
    print(name, "position log-likelihood error", e, "gate", gate)
    assert e <= gate

    def pos_bound(S):
        out = 0
        for sx, sy in ((d, d), (d, -d)):
            out = np.maximum(out, np.abs(MC.stats_positions(phys, packed[:, :nl], cx.astype(np.float64) + sx, cy.astype(np.float64) + sy, ex, ey)[1] - g_o) / S)
        return out
    ok, rep = H.grad_gate(g.cpu().numpy()[:, :nl], g_o, GRAD_RTOL_COL, pos_bound)
    print(name, "position gradient", rep)
    assert ok and rep["conditioned"] <= COND_CAP * g_o.size, rep
    assert not g.cpu().numpy()[:, nl:].any()


# ---------------------------------------------------------------------------------------------------
# 3. the lens-equation solver and the critical curves on a 65 x 65 map
# ---------------------------------------------------------------------------------------------------
def test_solver_and_critical_curves_on_the_interpolant(gl):
    """A cored isothermal lens sampled on a 65 x 65 map.  ``image_positions``: every returned image solves the lens equation OF THE
    INTERPOLANT -- the float64 restatement maps it back onto the source within 2e-5 arcsec (the solver's float32 floor), its
    magnification is the restatement's within 1e-3 relative -- and the float64 Newton solve from each image stays within 2e-5.
    ``critical_curves``: every endpoint has |det(I - H)| of the float64 restatement below 2e-3 (the refinement's float32 floor
    over a Hessian of order 1)."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass import Interpolated
    from gigalens_amd.simulator import SimulatorConfig
    pitch = 0.05
    ax, ay = MC.sampled((65, 65), pitch, MC.cored_isothermal(1.0, 0.12))  # +-1.6 arcsec, theta_E ~ 0.9
    phys = PhysicalModel([Interpolated(ax, ay, pitch)], [], [Sersic()])
    sim = gl.LensSimulator(phys, SimulatorConfig(delta_pix=0.1, num_pix=30), bs=3)
    rows = torch.tensor([[1.0, 0.0, 0.0], [0.9, 0.013, -0.021], [1.1, -0.02, 0.017]], dtype=torch.float32)
    full = torch.cat([rows, torch.tensor([[0.2, 1.5, 0.0, 0.0, 10.0]]).repeat(3, 1)], dim=1).to(sim.device)
    sx, sy = torch.tensor([0.05, 0.08, -0.06]), torch.tensor([0.03, -0.04, 0.07])
    xs, ys, mu, n = sim.image_positions(full, sx.to(sim.device), sy.to(sim.device), window=(-1.45, 1.45, -1.45, 1.45), num_cells=60)
    n = n.cpu().numpy().reshape(3)
    assert (n == 3).all(), n  # a cored lens inside its radial caustic: three images
    for b in range(3):
        px = xs[b].reshape(-1)[:n[b]].cpu().numpy().astype(np.float64)
        py = ys[b].reshape(-1)[:n[b]].cpu().numpy().astype(np.float64)
        m = MC.lens_maps(phys, rows[b:b + 1].double(), px, py).numpy()[:, :, 0]
        assert np.hypot(m[0] - float(sx[b]), m[1] - float(sy[b])).max() <= 2e-5
        mu_o = 1.0 / ((1 - m[2]) * (1 - m[5]) - m[3] * m[4])
        assert np.abs(mu[b].reshape(-1)[:n[b]].cpu().numpy() / mu_o - 1).max() <= 1e-3
        for _ in range(3):  # float64 Newton on the same interpolant from the returned images
            m = MC.lens_maps(phys, rows[b:b + 1].double(), px, py).numpy()[:, :, 0]
            rx, ry = float(sx[b]) - m[0], float(sy[b]) - m[1]
            det = (1 - m[2]) * (1 - m[5]) - m[3] * m[4]
            px, py = px + ((1 - m[5]) * rx + m[3] * ry) / det, py + ((1 - m[2]) * ry + m[4] * rx) / det
        assert np.hypot(px - xs[b].reshape(-1)[:n[b]].cpu().numpy(), py - ys[b].reshape(-1)[:n[b]].cpu().numpy()).max() <= 2e-5
    res = sim.critical_curves(full, window=(-1.45, 1.45, -1.45, 1.45), num_cells=60)
    assert bool(res["closed"].all()) and set(np.unique(res["kind"].cpu().numpy())) == {-1, 0, 1}
    for b in range(3):
        seg = res["critical"][b, :int(res["n"][b])].cpu().numpy().astype(np.float64).reshape(-1, 2)
        m = MC.lens_maps(phys, rows[b:b + 1].double(), seg[:, 0], seg[:, 1]).numpy()[:, :, 0]
        assert np.abs((1 - m[2]) * (1 - m[5]) - m[3] * m[4]).max() <= 2e-3
    assert bool(torch.isfinite(sim.einstein_radius(full)).all())


# ---------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals(gl):
    from gigalens_amd import _native
    from gigalens_amd.cosmology import MultiPlane
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass import Interpolated
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    gx, gy = np.meshgrid(np.arange(4, dtype=np.float32), np.arange(4, dtype=np.float32))
    comps = [_native.gl_component(14, 0, 0, 0), _native.gl_component(16, 0, 0, 0)]
    m = _native.Model(comps, 1, 0, 1, 4, 4, 1, gx.ravel(), gy.ravel(), None, 1.0)
    rows = torch.tensor([[1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=m.device)
    with pytest.raises(_native.NativeLibraryError, match="without deflection maps"):  # maps never attached
        m.simulate_fwd(rows)
    ones = np.ones((2, 2), dtype=np.float32)
    with pytest.raises(_native.NativeLibraryError, match="1..2048"):
        m.set_lens_maps(0, np.ones((1, 2049), dtype=np.float32), np.ones((1, 2049), dtype=np.float32), 0.1)
    with pytest.raises(_native.NativeLibraryError, match="not finite"):
        m.set_lens_maps(0, ones, np.array([[1.0, np.nan], [0.0, 0.0]], dtype=np.float32), 0.1)
    with pytest.raises(_native.NativeLibraryError, match="pitch"):
        m.set_lens_maps(0, ones, ones, 0.0)
    with pytest.raises(_native.NativeLibraryError, match="not a GL_INTERPOL_MASS lens"):
        m.set_lens_maps(1, ones, ones, 0.1)
    with pytest.raises(_native.NativeLibraryError, match="without deflection maps"):  # the refused calls left the model as it was
        m.simulate_fwd(rows)
    m.set_lens_maps(0, ones, ones, 0.1)
    assert tuple(m.simulate_fwd(rows).shape) == (1, 4, 4)
    with pytest.raises(_native.NativeLibraryError, match="not finite"):  # ... and a refused call after a good one keeps the good maps
        m.set_lens_maps(0, ones * np.inf, ones, 0.1)
    assert tuple(m.simulate_fwd(rows).shape) == (1, 4, 4)

    c = _case("IS-33x31")
    sim = _sim(gl, c)
    pd = c["packed"].to(sim.device)
    lens_rows = pd[:, :8]
    z = torch.zeros(3, device=sim.device)
    for call in (lambda: sim.potential(z, z, lens_rows), lambda: sim.fermat_potential(z, z, z, z, lens_rows),
                 lambda: sim.time_delays(lens_rows, z, z, time_delay_distance=1000.0),
                 lambda: sim._model.lens_potential(pd, z, z)):
        with pytest.raises(_native.UnsupportedLensError, match="INTERPOL_SCALED|interpolated lens"):
            call()
    pos = np.array([0.3, -0.2, 0.1], dtype=np.float32)
    sim._model.set_positions([pos], [pos[::-1].copy()], [np.full(3, 0.01, np.float32)], [np.full(3, 0.01, np.float32)])
    with pytest.raises(_native.UnsupportedLensError, match="interpolated lens"):  # the time-delay likelihood term
        sim._model.set_position_delays(np.array([0.0, 1.0, 2.0]), np.full(3, 0.1), np.array([np.nan]))
    lens = c["wl"].phys_model.lenses[0]
    with pytest.raises(_native.UnsupportedLensError, match="INTERPOL_SCALED"):
        lens.potential(z, z, scale_factor=1.0, center_x=0.0, center_y=0.0)
    mp = MultiPlane([0.3, 0.6], [1.5], 1.5)
    with pytest.raises(_native.UnsupportedLensError, match="INTERPOL_SCALED"):  # lens planes, at construction
        gl.LensSimulator(PhysicalModel([lens, SIE()], [], [Sersic()], multiplane=mp), c["wl"].sim_config, bs=3)

    class UserSheet(MassProfile):  # a user-written profile beside an interpolated lens: refused, typed
        _name, _params = "USER_SHEET", ["kappa", "center_x", "center_y"]
        hip_body = "template <class R> __device__ void deriv(R x, R y, const R* p, R& fx, R& fy) { fx = p[0] * (x - p[1]); fy = p[0] * (y - p[2]); }"
    with pytest.raises(_native.UnsupportedLensError, match="GL_INTERPOL_MASS"):
        gl.LensSimulator(PhysicalModel([lens, UserSheet()], [], [Sersic()]), SimulatorConfig(delta_pix=0.1, num_pix=8), bs=1)


# ---------------------------------------------------------------------------------------------------
# 5. apron edges: an exact node, a ray outside, a NaN ray
# ---------------------------------------------------------------------------------------------------
def test_apron_edges(gl):
    """Points with u in [-2, -1) and [W, W + 1] (taps beyond the apron, clamped), on exact nodes, outside the range and not finite:
    deflection and Hessian against the restatement under the value rule; outside and NaN: exactly beta = theta (NaN stays NaN in
    theta itself), Hessian exactly 0."""
    from gigalens_amd.profiles.mass import Interpolated
    h, w, pitch = 5, 4, 0.25  # dyadic pitch: the float32 coordinates below are the pixel coordinates they are meant to be
    ax, ay = MC.make_maps(h, w, pitch)
    lens = Interpolated(ax, ay, pitch)
    u = np.array([-2.0, -1.75, -1.5, -1.0 - 2 ** -10, 4.0, 4.25, 4.75, 5.0, 0.0, 1.0, 3.0, 2.5, -2.25, 5.25, 40.0, np.nan, 1.5, np.inf])
    v = np.array([0.5, 1.25, -1.5, 5.5, 2.0, -2.0, 6.0, 3.5, 0.0, 2.0, 4.0, 1.75, 1.0, 2.0, 1.0, 1.0, np.nan, 2.0])
    x, y = (u - 0.5 * (w - 1)) * pitch, (v - 0.5 * (h - 1)) * pitch
    kw = dict(scale_factor=torch.tensor([1.0, 0.5, -2.0]), center_x=torch.zeros(3), center_y=torch.zeros(3))
    xt, yt = torch.as_tensor(x, dtype=torch.float32)[:, None], torch.as_tensor(y, dtype=torch.float32)[:, None]
    gx, gy = (t.cpu().numpy() for t in lens.deriv(xt, yt, **kw))
    hs = np.stack([t.cpu().numpy() for t in lens.hessian(xt, yt, **kw)])
    out = ~((u >= -2) & (u <= w + 1) & (v >= -2) & (v <= h + 1))  # (NaN compares false: out)
    assert out.sum() == 6
    assert not gx[out].any() and not gy[out].any() and not hs[:, out].any()
    ins = ~out
    rows = torch.stack([kw["scale_factor"], kw["center_x"], kw["center_y"]], dim=1)
    one = type("P", (), dict(lenses=[lens]))()
    tx, ty = MC.deflection(torch.as_tensor(x[ins])[:, None].repeat(1, 3), torch.as_tensor(y[ins])[:, None].repeat(1, 3), ax, ay, pitch,
                           rows[:, 0].double(), rows[:, 1].double(), rows[:, 2].double())
    t32x, t32y = MC.deflection(torch.as_tensor(x[ins], dtype=torch.float32)[:, None].repeat(1, 3),
                               torch.as_tensor(y[ins], dtype=torch.float32)[:, None].repeat(1, 3), ax, ay, pitch, rows[:, 0], rows[:, 1], rows[:, 2])
    scale = float(max(tx.abs().max(), ty.abs().max()))
    gate = 4 * max(float((t32x.double() - tx).abs().max()), float((t32y.double() - ty).abs().max()), 6e-8 * scale) / scale
    e = max(np.abs(gx[ins] - tx.numpy()).max(), np.abs(gy[ins] - ty.numpy()).max()) / scale
    print("apron deflection error", e, "gate", gate)
    assert e <= gate
    node = (u == np.round(u)) & (v == np.round(v)) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    assert node.sum() == 3  # on a node the interpolant IS the map value (w(0) = 1, every other weight 0)
    for i in np.flatnonzero(node):
        assert np.array_equal(gx[i], np.float32(ax[int(v[i]), int(u[i])]) * kw["scale_factor"].numpy())
    # the Hessian away from the node lines (it jumps there), against autograd of the restatement
    with np.errstate(invalid="ignore"):  # (the infinite coordinate)
        clear = ins & (np.abs(u - np.round(u)) > 1e-3) & (np.abs(v - np.round(v)) > 1e-3)
    w64 = MC.lens_maps(one, rows.double(), x[clear], y[clear]).numpy()
    w32 = MC.lens_maps(one, rows, x[clear], y[clear], dtype=torch.float32).numpy()
    sc = np.abs(w64[2:]).max()
    gate = 4 * max(np.abs(w32[2:] - w64[2:]).max(), 6e-8 * sc) / sc
    e = np.abs(hs[:, clear] - w64[2:]).max() / sc
    print("apron Hessian error", e, "gate", gate)
    assert e <= gate
    # the same rays through a model: an image whose lens is absent on a ray renders the source at theta itself
    c = _case("I-7x9")
    sim = _sim(gl, c)
    far = c["packed"].clone()
    far[:, 1] = 100.0  # the maps far off the field: every ray outside the range
    none = far.clone()
    none[:, 0] = 0.0
    im_far = sim._model.simulate_fwd(far.to(sim.device))
    im_none = sim._model.simulate_fwd(none.to(sim.device))
    assert torch.equal(im_far, im_none) and float(im_far.abs().max()) > 0
    nan_rows = c["packed"].clone()
    nan_rows[1, 1] = float("nan")  # a NaN centre: every ray of that sample fails the range test, the lens is absent
    im_nan = sim._model.simulate_fwd(nan_rows.to(sim.device))
    assert torch.equal(im_nan[1], im_none[1])
