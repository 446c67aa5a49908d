"""The point-likelihood kernels (csrc/gl_positions.hip.h, gl_multiplane_pos.hip.h, gl_fluxes.hip.h, gl_tdelays.hip.h) on the GPU at
every launch edge of tests/points_cases.py against float64: the image positions (one plane, scaled families, lens planes), the flux
ratios and the time delays alone, and their fused sums through ``log_prob_and_grad`` with ``include_pixels=False`` -- per sample AND
per (sample, family) through ``gl_position_family_terms``, the optional outputs with their NaN patterns, the packed gradient.

Gates (those of tests/test_gpu_mp_positions.py, test_gpu_fluxes.py and test_gpu_tdelays.py): every value within 4 x the float32 CPU
yardstick of the same case against float64, relative to the largest value of its array; every gradient element within
``5e-4 scale + 1e-6`` (``PC.grad_gate`` <= 1); the columns of no lens exactly 0; two calls bitwise equal; the value independent of
whether the gradient was asked for; a sample evaluated alone gives the bits it has inside its batch.  The fused sums are compared
with the FLOAT64 prior plus the float64 sum of the restated terms (``points_cases.fused``), never with the GPU's own unfused calls.
Before every case the model's workspace is filled with NaN: an element no thread wrote shows up as NaN, not as what the previous
call left.  Every figure is printed with its yardstick before it is asserted."""
import numpy as np
import pytest
import torch

from tests import multilens_cases as MC
from tests import mp_positions_cases as PC
from tests import points_cases as X
from tests.test_gpu_multilens_grad import _t
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
_SIMS, _PMS = {}, {}
EXTRAS = {"positions": (), "fluxes": ("S", "model"), "delays": ("scale", "offset", "model")}


def _cfg():
    from gigalens_amd.simulator import SimulatorConfig
    return SimulatorConfig(delta_pix=MC.PIX, num_pix=8)  # (the camera plays no part in the point-image terms)


def _prior(c):
    """A Normal around the first sample for every column (``points_cases.prior_normal``): Identity bijectors."""
    from gigalens_amd import prior as tfd
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    return J({g: S([J({k: tfd.Normal(*X.prior_normal(v[0])) for k, v in d.items()}) for d in lst]) for g, lst in c["params"].items() if lst})


def _bound(gl, shape, lens_set, fluxes=True, delays=True):
    """``(case, simulator, ForwardProbModel with the case's families and the measurements asked for, packed rows)``."""
    c = X.case(shape, lens_set)
    if (shape, lens_set) not in _SIMS:
        _SIMS[shape, lens_set] = gl.LensSimulator(c["phys_mp"] if c["phys_mp"] is not None else c["phys"], _cfg(), bs=c["B"])
    sim = _SIMS[shape, lens_set]
    key = (shape, lens_set, fluxes, delays)
    if key not in _PMS:
        _PMS[key] = gl.ForwardProbModel(_prior(c), include_pixels=False, **X.centroids(c, fluxes, delays))
    return c, sim, _PMS[key], sim.pack(_t(c["params"]))


def _poison(model, B):
    model._workspace(B).fill_(255)  # every float of the workspace: NaN


def _call(model, c, term, packed, want_grad):
    """``dict(log_like, chi2, grad, fam, + the optional outputs)`` of one term alone, as device tensors."""
    if term == "positions":
        entry = model.multiplane_positions if c["phys_mp"] is not None else model.positions
        out = entry(packed, want_grad)
    elif term == "fluxes":
        out = model.position_fluxes(packed, want_grad, want_model=True)
    else:
        out = model.position_delays(packed, want_grad, want_model=True)
    d = dict(zip(("log_like", "chi2", "grad") + EXTRAS[term], out))
    d["fam"] = model.position_family_terms(packed.shape[0])
    return d


def _same(a, b):
    """Identical bits, the NaN of a family without a measurement included."""
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _host(d):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in d.items() if v is not None}


def _family_sum(fam):
    """The float32 sum over the families in family order: the operation of P4."""
    acc = np.zeros((fam.shape[0], 2), dtype=np.float32)
    for k in range(fam.shape[1]):
        acc = acc + fam[:, k].astype(np.float32)
    return acc


def _gate_values(label, dev, yard, keys):
    print(f"{label}: " + ", ".join(f"{k} {dev[k]:.2e} (float32 yardstick {yard[k]:.2e})" for k in keys))
    ratios = {k: (dev[k] / (4 * yard[k]) if yard[k] else (0.0 if dev[k] == 0 else np.inf)) for k in keys}
    print(f"   worst value figure {max(ratios.values()):.3f} of its gate ({max(ratios, key=ratios.get)})")
    return ratios


# ---- 1: every term alone ---------------------------------------------------------------------------------------------
TERM_CASES = [(shape, s, t) for shape, s in X.CASES for t in X.terms_of(shape, s)]


@pytest.mark.parametrize("shape,lens_set,term", TERM_CASES, ids=[f"{a}-{b}-{t}" for a, b, t in TERM_CASES])
def test_term_alone(gl, shape, lens_set, term):
    c, ref, yard = X.data(shape, lens_set, term)
    _, sim, pm, packed = _bound(gl, shape, lens_set)
    B, L = c["B"], c["lens_cols"]
    model = pm._bind_positions(sim)
    assert (model.n_images, model.n_families, model.P) == (sum(c["sizes"]), len(c["sizes"]), c["P"])
    _poison(model, B)
    a = _call(model, c, term, packed, True)
    b = _call(model, c, term, packed, True)
    n = _call(model, c, term, packed, False)
    got = _host(a)
    dev = X.deviations(dict(got, **{k: got[k] for k in EXTRAS[term]}), ref, term)  # (asserts that the NaN patterns agree)
    worst = PC.grad_gate(got["grad"][:, :L], ref["grad"][:, :L])
    ratios = _gate_values(f"{shape}-{lens_set} {term}", dev, yard, X.VALUE_KEYS[term])
    print(f"   gradient worst element {worst:.3f} of the gate (float32 yardstick {'-' if yard['grad'] is None else format(yard['grad'], '.3f')})")
    for k in ("log_like", "chi2", "grad", "fam"):
        assert torch.isfinite(a[k]).all(), f"{k}: an element no thread wrote, or a NaN of the kernels"
    assert all(_same(a[k], b[k]) for k in a), "two calls must give identical bits"
    assert n["grad"] is None and all(_same(a[k], n[k]) for k in a if k != "grad"), "the value does not depend on the gradient being asked for"
    assert np.array_equal(_family_sum(a["fam"].cpu().numpy()), np.stack([a["log_like"].cpu().numpy(), a["chi2"].cpu().numpy()], axis=-1))
    assert (got["grad"][:, L:] == 0).all(), "the columns of no lens"
    for k in EXTRAS[term]:
        assert got[k].shape == ref[k].shape, k
    assert max(ratios.values()) <= 1.0, ratios
    assert worst <= 1.0


# ---- 2: the fused sums against float64 -------------------------------------------------------------------------------
FUSED_CASES = [(shape, s, cb) for shape, s in X.CASES for cb in X.combos_of(shape, s)]


@pytest.mark.parametrize("shape,lens_set,combo", FUSED_CASES, ids=[f"{a}-{b}-{'+'.join(cb)}" for a, b, cb in FUSED_CASES])
def test_fused_sum(gl, shape, lens_set, combo):
    c, ref, yard = X.fused(shape, lens_set, combo)
    _, sim, pm, packed = _bound(gl, shape, lens_set, "fluxes" in combo, "delays" in combo)
    B = c["B"]
    assert pm.n_position == 2.0 * sum(c["sizes"]) and bool(pm.n_flux) == ("fluxes" in combo) and bool(pm.n_delay) == ("delays" in combo)
    z = pm.bij.inverse({g: lst for g, lst in _t(c["params"]).items() if lst}).to(sim.device).contiguous()
    cols = pm._perm(sim)[0]
    assert pm._perm(sim)[1].numel() == 0 and torch.equal(z.index_select(1, cols), packed)  # Identity bijectors: z IS the case's rows
    pm.log_prob_and_grad(sim, z)  # binds the prior and the families, sizes the workspace
    model = pm._bind_positions(sim)
    _poison(model, B)
    lp, red, gz = pm.log_prob_and_grad(sim, z)
    fam = model.position_family_terms(B)
    lp2, red2, gz2 = pm.log_prob_and_grad(sim, z)
    fam2 = model.position_family_terms(B)
    lp0, red0 = pm.log_prob(sim, z)
    for name, t in (("log_prob", lp), ("red_chi2", red), ("gradient", gz), ("family terms", fam)):
        assert torch.isfinite(t).all(), f"{name}: an element no thread wrote, or a NaN of the kernels"
    assert torch.equal(lp, lp2) and torch.equal(red, red2) and torch.equal(gz, gz2) and torch.equal(fam, fam2), "two calls must give identical bits"
    assert torch.equal(lp, lp0.detach()) and torch.equal(red, red0.detach()), "the value does not depend on the gradient being asked for"
    g = gz.index_select(1, cols).cpu().numpy().astype(np.float64)  # z columns -> the packed order of the reference
    famh = fam.cpu().numpy().astype(np.float64)
    dev = dict(log_prob=MC.rel_err(lp.cpu().numpy(), ref["log_prob"]), red_chi2=X._rel0(red.cpu().numpy(), ref["red_chi2"]),
               fam_ll=MC.rel_err(famh[..., 0], ref["fam"][..., 0]), fam_chi2=X._rel0(famh[..., 1], ref["fam"][..., 1]))
    worst = PC.grad_gate(g, ref["grad"])
    ratios = _gate_values(f"{shape}-{lens_set} fused {'+'.join(combo)}", dev, yard, ("log_prob", "red_chi2", "fam_ll", "fam_chi2"))
    print(f"   gradient worst element {worst:.3f} of the gate (float32 yardstick {'-' if yard['grad'] is None else format(yard['grad'], '.3f')})")
    # a family without a measurement keeps, bit for bit, what the position kernel left in its elements
    entry = model.multiplane_positions if c["phys_mp"] is not None else model.positions
    entry(packed, True)
    fam_pos = model.position_family_terms(B)
    none = [k for k, kind in enumerate(X.modes(shape)) if kind == "none"]
    measured = [k for k, kind in enumerate(X.modes(shape)) if kind != "none"]
    assert torch.equal(fam[:, none], fam_pos[:, none])
    assert not torch.equal(fam[:, measured], fam_pos[:, measured])
    assert max(ratios.values()) <= 1.0, ratios
    assert worst <= 1.0


# ---- 3: a sample alone -----------------------------------------------------------------------------------------------
ALONE_CASES = [(shape, s) for shape, s in X.CASES if X.SHAPES[shape][0] > 1]


def _picks(B, F, J):
    """The first and the last sample and those whose elements straddle thread 64 of the B F and of the B J grids."""
    picks = {0, B - 1}
    for n in (F, J):
        if 64 % n and 64 // n < B:
            picks.add(64 // n)
    return sorted(picks)


@pytest.mark.parametrize("shape,lens_set", ALONE_CASES, ids=[f"{a}-{b}" for a, b in ALONE_CASES])
def test_sample_alone_has_the_bits_of_its_batch(gl, shape, lens_set):
    c, sim, pm, packed = _bound(gl, shape, lens_set)
    B, F, J = c["B"], len(c["sizes"]), sum(c["sizes"])
    model = pm._bind_positions(sim)
    picks = _picks(B, F, J)
    if B * F > 64:
        assert any(b * F < 64 < (b + 1) * F for b in picks) or 64 % F == 0
    if B * J > 64:
        assert any(b * J < 64 < (b + 1) * J for b in picks) or 64 % J == 0
    for term in X.held(shape, lens_set):
        _poison(model, B)
        batch = _call(model, c, term, packed, True)
        for b in picks:
            _poison(model, 1)
            one = _call(model, c, term, packed[b:b + 1].contiguous(), True)
            for k in batch:
                assert _same(one[k][0], batch[k][b]), (term, b, k)
    print(f"{shape}-{lens_set}: samples {picks} alone give the bits of the batch of {B}")
