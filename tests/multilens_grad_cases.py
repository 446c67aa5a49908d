"""Cases and float64 reference of the multi-plane gradient (csrc/gl_multiplane_bwd.hip.h): tests/test_multilens_grad_host.py pins
the reference and the kernel's specification without a GPU, tests/test_gpu_multilens_grad.py runs the kernels against them.

The reference is ``torch.autograd`` on the float64 restatement of tests/multilens_cases.py -- ``plane_sums`` / ``target_beta`` /
``stats_pixels`` unchanged, the render (``image_t``) restated here to take leaf tensors, i.e. the columns of one packed ``[B, P]``
float64 tensor that requires grad, so the gradient comes out in the library's packed order.

``reverse_recursion`` is the kernel's specification written out in torch: abar and thetabar, the planes backwards.  It is fed with
every lens's own float64 Jacobian (autograd on that one lens at the ray's position on its plane) and must equal autograd on the
whole composition.

Gate of a gradient (``gate``): ``helpers.grad_gate`` with the project's ``GRAD_RTOL_COL`` -- every element within 3e-4 of the scale of
its own parameter column, or, for at most ``MAX_CONDITIONED`` elements of a case, within that + 4 x the float32 conditioning bound of
the element.  The bound is ``helpers.float32_conditioning_bound`` restated for the plane recursion: any float32 implementation rounds
a position of the size of the field to one ulp of it each time it forms one -- the grid theta, ``theta_j = theta - sum C_ij a_i`` on
every later plane, ``beta_s`` of every source -- so the float64 restatement is run with each of those positions displaced by
``d = ulp(max |theta|)`` (uniformly along (+,+) and (+,-), and by two draws of noise of that rms, independent per position), and the
largest change of each gradient element relative to its column scale is the bound."""
import functools

import numpy as np
import torch

from tests import helpers
from tests import multilens_cases as MC

F64 = torch.float64
GRAD_RTOL_COL = 3e-4   # tests/test_gpu_parity.py
MAX_CONDITIONED = 2    # elements of a case that may pass through the conditioning bound


# ---------------------------------------------------------------------------------------------------------------------
# the restatement on leaf tensors
# ---------------------------------------------------------------------------------------------------------------------
def pack_np(phys, params):
    """``[B, P]`` float64 packed rows of the float32 values in ``params`` (the library's column order), on the CPU."""
    bs = max(int(np.size(v)) for lst in params.values() for d in lst for v in d.values())
    return phys._packing().pack(params, bs, "cpu").double()


def _shift(shift, key, x, y):
    if shift is None:
        return x, y
    dx, dy = shift(key)
    return x + dx, y + dy


def plane_sums_t(phys, mp, lens_params, x, y, shift=None):
    """``MC.plane_sums`` with an optional displacement of the ray's position on every plane behind the first (``shift(("plane", j))``)."""
    if shift is None:
        return MC.plane_sums(phys, mp, lens_params, x, y)
    from oracle import ref_torch as ref
    C = torch.as_tensor(np.asarray(mp.lens_scales, dtype=np.float32)).to(x.dtype)
    consts = MC._consts(phys, x.dtype)
    sums = []
    for j in range(mp.K):
        xj, yj = x, y
        for i in range(j):
            xj, yj = xj - C[i, j] * sums[i][0], yj - C[i, j] * sums[i][1]
        if j:
            xj, yj = _shift(shift, ("plane", j), xj, yj)
        ax = ay = 0
        for l, lens in enumerate(phys.lenses):
            if int(mp.plane_of_lens[l]) == j:
                fx, fy = ref.mass_deriv(lens, xj, yj, **lens_params[l], **consts[l])
                ax, ay = ax + fx, ay + fy
        sums.append((ax, ay))
    return sums


def image_t(phys, cfg, psf, mp, pt, bs, shift=None):
    """``MC.image`` (every part) on a structure ``pt`` of float64 tensors: the image ``[bs, H, W]`` and its ``RefSimulator``."""
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(phys, cfg, bs, dtype=F64, supersampled_kernel=psf)
    X, Y = _shift(shift, "theta", rs.img_X, rs.img_Y)
    Hs, Ws = rs.wcs.n_x * rs.supersample, rs.wcs.n_y * rs.supersample
    rr, cc = torch.from_numpy(rs.region[:, 0]), torch.from_numpy(rs.region[:, 1])
    img = torch.zeros((Hs, Ws, bs), dtype=F64)
    for lm, p, c in zip(phys.lens_light, pt.get("lens_light", []), rs._consts("lens_light_constants", len(phys.lens_light))):
        img = img.index_put((rr, cc), ref.light_eval(lm, X, Y, **p, **c), accumulate=True)
    sums = plane_sums_t(phys, mp, pt["lens_mass"], X, Y, shift)
    for s, (lm, p, c) in enumerate(zip(phys.source_light, pt["source_light"], rs._consts("source_light_constants", len(phys.source_light)))):
        bx, by = _shift(shift, ("source", s), *MC.target_beta(sums, X, Y, mp.source_scales[:, s]))
        img = img.index_put((rr, cc), ref.light_eval(lm, bx, by, **p, **c), accumulate=True)
    nan = torch.isnan(img)
    img = torch.where(nan, torch.zeros_like(img), img)
    ret = ref.psf_pool(img.permute(2, 0, 1)[:, None], rs.flat_kernel, rs.supersample)[:, 0]
    return ret * rs.conversion_factor, rs, int(nan.sum())


def stats_t(im, rs, obs, error_map=None):
    """``MC.stats_pixels``; with ``error_map`` the noise is that map instead of ``background_rms`` / ``exp_time``."""
    if error_map is None:
        return MC.stats_pixels(im, rs, obs, MC.BG, MC.TEXP)
    err = torch.as_tensor(np.asarray(error_map, dtype=np.float32)).to(im.dtype)
    o = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(im.dtype)
    reg = rs.img_region
    chi2 = torch.sum(((im - o) / err) ** 2 * reg, dim=(-2, -1))
    norm = torch.sum(torch.log(2 * np.pi * err ** 2) * reg, dim=(-2, -1))
    return -0.5 * (chi2 + norm), chi2 / torch.count_nonzero(reg).to(im.dtype)


def _leaf(c):
    packed = pack_np(c["phys"], c["params"]).clone().requires_grad_(True)
    return packed, helpers.struct_from_packed(c["phys"], packed)


def loglike_grad(c, obs, error_map=None, shift=None):
    """``(log_like [B], d log_like / d packed [B, P], image [B, H, W], number of NaN pixels)`` of case ``c`` in float64."""
    packed, pt = _leaf(c)
    im, rs, n_nan = image_t(c["phys"], c["cfg"], c["psf"], c["mp"], pt, c["B"], shift)
    ll, _ = stats_t(im, rs, obs, error_map)
    (g,) = torch.autograd.grad(ll.sum(), packed)
    return ll.detach().numpy(), g.numpy(), im.detach().numpy(), n_nan


def image_vjp(c, cotangent, shift=None):
    """The VJP of the float64 image with ``cotangent`` ``[B, H, W]``: ``[B, P]``."""
    packed, pt = _leaf(c)
    im, _, _ = image_t(c["phys"], c["cfg"], c["psf"], c["mp"], pt, c["B"], shift)
    (g,) = torch.autograd.grad((im * torch.as_tensor(np.asarray(cotangent, dtype=np.float64))).sum(), packed)
    return g.numpy()


def conditioning_bound(c, grad_fn, g64, S, seed=0):
    """The float32 conditioning bound of every element of ``g64`` (module docstring); ``grad_fn(shift)`` is the float64 gradient with
    the positions displaced by ``shift``."""
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(c["phys"], c["cfg"], 1, dtype=F64, supersampled_kernel=c["psf"])
    d = float(np.spacing(np.float32(max(float(rs.img_X.abs().max()), float(rs.img_Y.abs().max())))))
    n = rs.img_X.shape[0]
    rng = np.random.default_rng(seed)

    def noise():
        drawn = {}

        def shift(key):
            if key not in drawn:
                drawn[key] = (torch.as_tensor(d * rng.normal(size=(n, 1))), torch.as_tensor(d * rng.normal(size=(n, 1))))
            return drawn[key]
        return shift
    out = np.zeros_like(g64)
    for sh in (lambda key: (d, d), lambda key: (d, -d), noise(), noise()):
        out = np.maximum(out, np.abs(grad_fn(sh) - g64) / np.maximum(S, 1e-300))
    return out


def gate(g, g64, bound_fn, what):
    """Print the worst element and the number of conditioned ones, then apply the gate of the module docstring."""
    ok, rep = helpers.grad_gate(g, g64, GRAD_RTOL_COL, bound_fn)
    print(f"{what}: worst element {rep['worst']:.3e} of its column scale, {rep['conditioned']} beyond {GRAD_RTOL_COL:g}"
          + (f" (worst {rep['worst_over_bound']:.2f} x its conditioning bound)" if rep["conditioned"] else ""))
    assert np.isfinite(np.asarray(g)).all(), what
    assert ok, (what, rep)
    assert rep["conditioned"] <= MAX_CONDITIONED, (what, rep)
    return rep


def assert_well_posed(g64, n_nan, what):
    """Every column has a scale of its own and no pixel is NaN: the column metric cannot degenerate."""
    assert n_nan == 0, (what, n_nan)
    assert np.isfinite(g64).all(), what
    scale = np.abs(g64).max(axis=0)
    assert (scale > 0).all(), (what, scale)
    return scale


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
f = MC._f32
ZOO_CASES = ("zoo_a", "zoo_b")


@functools.lru_cache(maxsize=None)
def zoo_case(name):
    """Every lens kind on a plane behind the first (the position adjoint of a lens is used only there), 14 x 14 at 0.2 arcsec, three
    samples; lens centres 0.37 px off the pixel centres; two smooth sources, a SersicEllipse in front of the last plane and a Sersic
    behind every plane."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW, NFW_ELLIPSE
    from gigalens_amd.profiles.mass.piemd import DPIE, DPIS
    from gigalens_amd.profiles.mass.piep import DPIEP
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.profiles.mass.tnfw import TNFW
    from gigalens_amd.simulator import SimulatorConfig
    px = 0.2
    o = 0.37 * px + px / 2  # pixel centres of an even grid lie at odd multiples of px / 2

    def at(*k):  # centres at whole pixels + o
        return f(*[v * px + o for v in k])
    sie = {"theta_E": f(0.9, 0.8, 1.0), "e1": f(0.1, -0.05, 0.15), "e2": f(-0.05, 0.1, 0.0), "center_x": at(0, 1, -1), "center_y": at(-1, 0, 0)}
    sis = {"theta_E": f(0.9, 0.8, 1.0), "center_x": at(0, 1, -1), "center_y": at(-1, 0, 0)}
    src = [{"R_sersic": f(0.4, 0.5, 0.35), "n_sersic": f(1.0, 0.8, 1.2), "e1": f(0.1, -0.1, 0.0), "e2": f(0.05, 0.0, -0.1),
            "center_x": f(0.15, -0.1, 0.2), "center_y": f(-0.1, 0.2, 0.05), "Ie": f(120.0, 150.0, 100.0)},
           {"R_sersic": f(0.45, 0.35, 0.5), "n_sersic": f(1.0, 1.2, 0.8), "center_x": f(-0.2, 0.1, 0.0), "center_y": f(0.1, -0.15, 0.2),
            "Ie": f(150.0, 110.0, 130.0)}]
    if name == "zoo_a":
        lenses, zl, zs = [SIE(), EPL(), Shear(), NFW(), DPIS(), DPIE(), SIS()], [0.3, 0.7, 0.7, 0.7, 0.7, 1.4, 1.4], [1.0, 2.5]
        lp = [sie,
              {"theta_E": f(0.4, 0.3, 0.45), "gamma": f(2.1, 1.9, 2.2), "e1": f(0.1, -0.05, 0.15), "e2": f(-0.05, 0.1, 0.0),
               "center_x": at(2, -1, 1), "center_y": at(1, 2, -2)},
              {"gamma1": f(0.03, -0.02, 0.04), "gamma2": f(-0.02, 0.03, 0.01)},
              {"Rs": f(1.0, 0.8, 1.2), "alpha_Rs": f(0.3, 0.25, 0.4), "center_x": at(-2, 1, 0), "center_y": at(1, -2, 2)},
              {"theta_E": f(0.3, 0.25, 0.4), "r_core": f(0.1, 0.15, 0.08), "r_cut": f(1.5, 1.2, 2.0), "center_x": at(-1, 2, -2),
               "center_y": at(-2, -1, 1)},
              {"theta_E": f(0.35, 0.45, 0.3), "r_core": f(0.08, 0.1, 0.05), "r_cut": f(1.5, 2.0, 1.2), "center_x": at(1, -2, 2),
               "center_y": at(-2, 1, -1), "e1": f(0.1, -0.1, 0.05), "e2": f(0.0, 0.08, -0.1)},
              {"theta_E": f(0.3, 0.25, 0.35), "center_x": at(-2, 2, 0), "center_y": at(2, -2, -1)}]
    elif name == "zoo_b":
        lenses, zl, zs = [SIS(), TNFW(), NFW_ELLIPSE(), DPIEP(), Shear(), SIE()], [0.3, 0.6, 0.6, 1.0, 1.5, 1.5], [1.2, 2.5]
        lp = [sis,
              {"Rs": f(1.0, 0.8, 1.2), "alpha_Rs": f(0.3, 0.25, 0.4), "r_trunc": f(2.0, 2.5, 1.5), "center_x": at(2, -1, 1),
               "center_y": at(1, 2, -2)},
              {"Rs": f(1.2, 1.0, 0.8), "alpha_Rs": f(0.35, 0.3, 0.25), "e1": f(0.08, -0.1, 0.05), "e2": f(-0.05, 0.05, 0.1),
               "center_x": at(-2, 1, 0), "center_y": at(1, -2, 2)},
              {"theta_E": f(0.35, 0.45, 0.3), "Ra": f(0.08, 0.1, 0.05), "Rs": f(1.5, 2.0, 1.2), "center_x": at(1, -2, 2),
               "center_y": at(-2, 1, -1), "e1": f(0.1, -0.1, 0.05), "e2": f(0.0, 0.08, -0.1)},
              {"gamma1": f(0.03, -0.02, 0.04), "gamma2": f(-0.02, 0.03, 0.01)},
              {"theta_E": f(0.3, 0.25, 0.4), "e1": f(-0.1, 0.15, 0.05), "e2": f(0.08, -0.02, 0.1), "center_x": at(-2, 2, 0),
               "center_y": at(2, -2, -1)}]
    else:
        raise KeyError(name)
    mp = MC._mp(zl, zs)
    lights = ([], [SersicEllipse(), Sersic()])
    params = {"lens_mass": lp, "lens_light": [], "source_light": src}
    cfg = SimulatorConfig(delta_pix=px, num_pix=14)
    return dict(phys=PhysicalModel(lenses, *lights), phys_mp=PhysicalModel(lenses, *lights, multiplane=mp), mp=mp, cfg=cfg, psf=None,
                params=params, B=3)


def plain_case(num_pix, B):
    """The ``plain16`` model on a ``num_pix`` square grid with the first ``B`` samples (more than one partial row per sample)."""
    from gigalens_amd.simulator import SimulatorConfig
    c = dict(MC.render_case("plain16"))
    c["cfg"] = SimulatorConfig(delta_pix=0.2 * 16 / num_pix, num_pix=num_pix)  # the same field of view
    c["params"] = {g: [{k: v[:B] for k, v in d.items()} for d in lst] for g, lst in c["params"].items()}
    c["B"] = B
    return c


@functools.lru_cache(maxsize=None)
def empty_plane_case():
    """The lens set of ``test_empty_second_plane_equals_the_scaled_single_plane`` -- SIE + Shear on plane 1, a zero-strength SIS alone
    on plane 2 -- in front of one Sersic source at z = 1.8, 12 x 12, three samples; ``phys_1`` is the single-plane model it equals
    (``source_light_scales = C_1s``) for every column but the empty lens's own."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import SimulatorConfig
    base = MC.map_case("shared")["lens_params"]
    lp = [base[0], base[2], {"theta_E": f(0.0, 0.0, 0.0), "center_x": base[1]["center_x"], "center_y": base[1]["center_y"]}]
    lenses, lights = [SIE(), Shear(), SIS()], ([], [Sersic()])
    mp = MC._mp([0.4, 0.4, 0.9], [1.8])
    params = {"lens_mass": lp, "lens_light": [],
              "source_light": [{"R_sersic": f(0.3, 0.25, 0.35), "n_sersic": f(1.0, 1.5, 1.2), "center_x": f(0.05, -0.1, 0.1),
                                "center_y": f(-0.05, 0.1, 0.0), "Ie": f(120.0, 150.0, 100.0)}]}
    return dict(phys=PhysicalModel(lenses, *lights), phys_mp=PhysicalModel(lenses, *lights, multiplane=mp), mp=mp,
                phys_1=PhysicalModel(lenses, *lights, source_light_scales=[float(np.float32(mp.source_scales[0, 0]))]),
                cfg=SimulatorConfig(delta_pix=0.2, num_pix=12), psf=None, params=params, B=3, shared_cols=list(range(7)) + list(range(10, 15)))


@functools.lru_cache(maxsize=None)
def unused_plane_case():
    """``plain16`` without its far source: the SIS plane (z = 1.0) lies behind the only source (z = 0.8) and deflects nothing.  The
    render ignores it; its three columns (7..9) have an exactly zero gradient and nothing of it may leak into the others."""
    from gigalens_amd.model import PhysicalModel
    c = dict(MC.render_case("plain16"))
    ph = c["phys"]
    mp = MC._mp([0.5, 0.5, 1.0], [0.8])
    lights = (ph.lens_light, ph.source_light[:1])
    c.update(phys=PhysicalModel(ph.lenses, *lights), phys_mp=PhysicalModel(ph.lenses, *lights, multiplane=mp), mp=mp,
             params=dict(c["params"], source_light=c["params"]["source_light"][:1]), shared_cols=list(range(7)) + list(range(10, 22)))
    return c


def case(name):
    if name in MC.RENDER_CASES:
        return MC.render_case(name)
    if name == "unused_plane":
        return unused_plane_case()
    if name in ZOO_CASES:
        return zoo_case(name)
    if name == "empty_plane":
        return empty_plane_case()
    if name.startswith("plain") and "x" in name:  # "plain<num_pix>x<B>"
        n, B = name[5:].split("x")
        return plain_case(int(n), int(B))
    raise KeyError(name)


def observation(c, seed=11):
    """A seeded noisy observation of the first sample of case ``c`` (float32 ``[H, W]``), as ``MC.render_data`` draws it."""
    with torch.no_grad():
        im, _, _ = image_t(c["phys"], c["cfg"], c["psf"], c["mp"], MC._tensors(c["params"], F64), c["B"])
    clean = im[0].numpy()
    r = np.random.default_rng(seed)
    return (clean + r.normal(size=clean.shape) * np.sqrt(MC.BG ** 2 + np.clip(clean, 0, None) / MC.TEXP)).astype(np.float32)


def error_map_of(obs):
    """A noise map for the cases that run with ``error_map``: the noise model evaluated on the observation (float32)."""
    return np.sqrt(MC.BG ** 2 + np.clip(obs, 0, None) / MC.TEXP).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grad_data(name, with_error_map=False):
    """``(case, obs, error_map or None, log_like64 [B], grad64 [B, P], bound_fn)`` -- computed once and shared (left unchanged).
    ``bound_fn(S)`` is the conditioning bound, evaluated only when an element needs it."""
    c = case(name)
    obs = MC.render_data(name)[1] if name in MC.RENDER_CASES else observation(c)
    em = error_map_of(obs) if with_error_map else None
    ll, g, _, n_nan = loglike_grad(c, obs, em)
    assert_well_posed(g[:, c["shared_cols"]] if "shared_cols" in c else g, n_nan, name)
    return c, obs, em, ll, g, loglike_bound(c, obs, em, g)


def loglike_bound(c, obs, em, g64, cols=None):
    """``bound_fn(S)`` of the log-likelihood gradient ``g64`` of case ``c`` (``cols``: of these columns alone)."""
    sel = (lambda g: g) if cols is None else (lambda g: g[:, cols])
    return lambda S: conditioning_bound(c, lambda sh: sel(loglike_grad(c, obs, em, sh)[1]), sel(g64), S)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's specification: the reverse recursion
# ---------------------------------------------------------------------------------------------------------------------
def reverse_recursion(phys, mp, lens_params, x, y, targets):
    """The gradient of ``sum_t <betabar_t, beta_t>`` with respect to every lens parameter by the recursion the kernel runs.
    ``lens_params``: dicts of float64 tensors; ``x, y`` ``(n, B)``; ``targets``: ``[(T [K] couplings, betabar_x, betabar_y)]``.
    Returns one dict of gradients (shaped like the parameters) per lens.

    Forward: ``a_i`` and ``theta_j`` (``MC.plane_sums``).  Backward: ``abar_i = -sum_t T_it betabar_t`` over the targets plane i
    deflects; then the planes from the last to the first -- when plane j is reached ``abar_j`` is complete; every lens l on it is
    differentiated ON ITS OWN at ``theta_j`` with cotangent ``abar_j`` (autograd on that one lens: its parameter gradient and its
    position cotangent ``thetabar``), and ``abar_i -= C_ij thetabar`` for every plane i in front of j.  ``thetabar`` of plane 0 is
    dropped."""
    from oracle import ref_torch as ref
    K = mp.K
    C = np.asarray(mp.lens_scales, dtype=np.float32).astype(np.float64)
    consts = MC._consts(phys, x.dtype)
    with torch.no_grad():
        det = [{k: v.detach() for k, v in d.items()} for d in lens_params]
        sums = MC.plane_sums(phys, mp, det, x, y)
    abar = [[torch.zeros_like(x), torch.zeros_like(y)] for _ in range(K)]
    for T, gbx, gby in targets:
        T = np.asarray(T, dtype=np.float32).astype(np.float64)
        for i in range(K):
            if T[i] != 0.0:
                abar[i][0] = abar[i][0] - T[i] * gbx
                abar[i][1] = abar[i][1] - T[i] * gby
    grads = [None] * len(phys.lenses)
    order = [l for j in range(K) for l in range(len(phys.lenses)) if int(mp.plane_of_lens[l]) == j]
    for l in reversed(order):
        j = int(mp.plane_of_lens[l])
        xj, yj = x, y
        for i in range(j):
            xj, yj = xj - C[i, j] * sums[i][0], yj - C[i, j] * sums[i][1]
        xj, yj = xj.detach().clone().requires_grad_(True), yj.detach().clone().requires_grad_(True)
        p = {k: v.detach().clone().requires_grad_(True) for k, v in lens_params[l].items()}
        fx, fy = ref.mass_deriv(phys.lenses[l], xj, yj, **p, **consts[l])
        out = torch.autograd.grad((abar[j][0] * fx + abar[j][1] * fy).sum(), [xj, yj] + list(p.values()), allow_unused=True)
        tbx, tby = out[0], out[1]
        grads[l] = {k: (g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(p.items(), out[2:])}
        for i in range(j):
            abar[i][0] = abar[i][0] - C[i, j] * tbx
            abar[i][1] = abar[i][1] - C[i, j] * tby
    return grads


def two_shear_gradients():
    """Two pure-shear planes (``MC.two_shear_case``) and the loss ``L = 1/2 sum_points |beta - beta_0|^2``:
    ``beta = M theta``, ``M = I - T1 G1 - T2 G2 (I - C12 G1)``.  Returns ``dict(closed, autograd, recursion)`` of the gradient with
    respect to (gamma1, gamma2) of plane 1 and of plane 2, ``[4]`` float64 each."""
    phys, _, mp, lp, T, _ = MC.two_shear_case()
    x, y = MC.points(70)
    th = np.stack([x, y]).astype(np.float64)                       # [2, n]
    beta0 = np.stack([0.3 * y, -0.2 * x]).astype(np.float64)       # any fixed target
    C12, T1, T2 = (float(np.float32(v)) for v in (mp.lens_scales[0, 1], T[0], T[1]))
    g = [float(np.float32(v).reshape(-1)[0]) for v in (lp[0]["gamma1"], lp[0]["gamma2"], lp[1]["gamma1"], lp[1]["gamma2"])]
    E = [np.array([[1.0, 0.0], [0.0, -1.0]]), np.array([[0.0, 1.0], [1.0, 0.0]])]
    G1, G2 = g[0] * E[0] + g[1] * E[1], g[2] * E[0] + g[3] * E[1]
    M = np.eye(2) - T1 * G1 - T2 * G2 @ (np.eye(2) - C12 * G1)
    r = M @ th - beta0
    dM = [-T1 * E[0] + T2 * C12 * G2 @ E[0], -T1 * E[1] + T2 * C12 * G2 @ E[1],
          -T2 * E[0] @ (np.eye(2) - C12 * G1), -T2 * E[1] @ (np.eye(2) - C12 * G1)]
    closed = np.array([np.sum(r * (d @ th)) for d in dM])
    xt, yt = torch.as_tensor(th[0])[:, None], torch.as_tensor(th[1])[:, None]
    b0x, b0y = torch.as_tensor(beta0[0])[:, None], torch.as_tensor(beta0[1])[:, None]
    leaves = [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).double().reshape(1).requires_grad_(True) for k, v in d.items()} for d in lp]
    bx, by = MC.target_beta(MC.plane_sums(phys, mp, leaves, xt, yt), xt, yt, T)
    L = 0.5 * ((bx - b0x) ** 2 + (by - b0y) ** 2).sum()
    flat = [leaves[0]["gamma1"], leaves[0]["gamma2"], leaves[1]["gamma1"], leaves[1]["gamma2"]]
    auto = np.array([float(v) for v in torch.autograd.grad(L, flat)])
    rec = reverse_recursion(phys, mp, leaves, xt, yt, [(T, (bx - b0x).detach(), (by - b0y).detach())])
    recursion = np.array([float(rec[0]["gamma1"]), float(rec[0]["gamma2"]), float(rec[1]["gamma1"]), float(rec[1]["gamma2"])])
    return dict(closed=closed, autograd=auto, recursion=recursion)


def map_case_gradients(name):
    """``MC.map_case(name)``'s lens set, 70 points, three samples, ``L = sum <w, beta_target>`` with fixed weights: the gradient of
    every lens parameter by autograd on the whole composition and by ``reverse_recursion``, as two flat float64 arrays."""
    c = MC.map_case(name)
    x, y = MC.points(70)
    B = 3
    xt = torch.as_tensor(x.astype(np.float64))[:, None].repeat(1, B)
    yt = torch.as_tensor(y.astype(np.float64))[:, None].repeat(1, B)
    r = np.random.default_rng(5)
    wx, wy = torch.as_tensor(r.normal(size=(70, B))), torch.as_tensor(r.normal(size=(70, B)))
    leaves = [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).double().requires_grad_(True) for k, v in d.items()}
              for d in c["lens_params"]]
    bx, by = MC.target_beta(MC.plane_sums(c["phys"], c["mp"], leaves, xt, yt), xt, yt, c["target"])
    flat = [v for d in leaves for v in d.values()]
    # (a plane at or behind the target does not deflect it: its lenses' parameters are unused, their gradient is zero)
    auto = [torch.zeros_like(v) if a is None else a for v, a in zip(flat, torch.autograd.grad((wx * bx + wy * by).sum(), flat, allow_unused=True))]
    rec = reverse_recursion(c["phys"], c["mp"], leaves, xt, yt, [(c["target"], wx, wy)])
    return (np.concatenate([a.numpy().ravel() for a in auto]),
            np.concatenate([rec[l][k].numpy().ravel() for l, d in enumerate(leaves) for k in d]))
