"""The stream-path probabilistic models on their shared base, without a GPU: ``SourceEvidenceProbModel``, ``PointImageProbModel``,
``WeakLensingProbModel`` and ``ImagePlaneProbModel`` over a stub simulator whose likelihood methods return fixed float32 tensors
(``B = 3`` samples, ``P = 5`` packed columns).  ``log_prob`` is the stub's value plus ``log_prior``, bit for bit; the reduced
chi^2 divides by the model's own data count; ``log_prob_and_grad`` returns detached tensors whose gradient is that of a plain
torch restatement built from the stub's ``grad`` (the same float32 operations, so ``torch.equal``); a joined ``strong`` model adds
its term with the prior counted once; ``ModellingSequence._event_size`` of every model class; and what ``model._GradFn`` asks of
the entry it wraps."""
import numpy as np
import pytest
import torch

from gigalens_amd import _native
from gigalens_amd import model as M
from gigalens_amd import prior as tfd
from gigalens_amd.inference import ModellingSequence

B, P, N_GAL, N_USED = 3, 5, 3, 10
REGION = torch.zeros(4, 4)
REGION.view(-1)[:N_USED] = 1.0
J_, S_ = tfd.JointDistributionNamed, tfd.JointDistributionSequential
LENS_PRIOR = J_(dict(lens_mass=S_([J_(dict(theta_E=tfd.LogNormal(0.1, 0.2), center_x=tfd.Normal(0.05, 0.3)))])))
IMAGE_PRIOR = J_(dict(point_images=S_([J_(dict(x=tfd.Normal(0.9, 0.1), y=tfd.Normal(-0.4, 0.2)))])))
Z = torch.tensor([[0.3, -0.2], [-1.1, 0.7], [0.05, 1.4]])
OBS, ERR = np.zeros((4, 4), np.float32), np.ones((4, 4), np.float32)


def _fixed(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class _Simulator:
    """What the four models read of a ``LensSimulator``: fixed results, and the arguments of the last call."""
    img_region = REGION
    results = {
        "shear": dict(log_like=_fixed(1, B), chi2=_fixed(2, B).abs(), grad=_fixed(3, B, P)),
        "image_plane": dict(log_like=_fixed(4, B), chi2=_fixed(5, B).abs(), grad=_fixed(6, B, P), n_lost=torch.zeros(B, dtype=torch.int32)),
        "evidence": dict(log_evidence=_fixed(7, B), chi2=_fixed(8, B).abs(), grad=_fixed(9, B, P)),
        "point_image": dict(log_like=_fixed(10, B), chi2=_fixed(11, B).abs(), grad=_fixed(12, B, P), grad_x=_fixed(13, B, 1),
                            grad_y=_fixed(14, B, 1)),
    }

    def _pack_partial(self, struct):
        a, b = tfd.nest_flatten(struct)  # every leaf in one column, constants beside them: the graph is kept
        return torch.stack([a, b, torch.full_like(a, 1.5), torch.full_like(a, -0.5), torch.ones_like(a)], dim=1)

    def _record(self, name, *tensors, **kw):
        assert all(not t.requires_grad and t.dtype == torch.float32 for t in tensors)
        self.last = (name, tensors, kw)
        return {k: v.clone() for k, v in self.results[name].items()}  # (fresh tensors, as every native call returns)

    def shear_log_like_and_grad(self, packed, catalogue, want_grad=True):
        return self._record("shear", packed, catalogue=catalogue, want_grad=want_grad)

    def image_plane_log_like_and_grad(self, packed, families, want_grad=True):
        return self._record("image_plane", packed, families=families, want_grad=want_grad)

    def source_evidence_and_grad(self, packed, obs, err, **kw):
        return self._record("evidence", packed, obs=obs, err=err, **kw)

    def point_image_log_like_and_grad(self, packed, x, y, obs, err, mask=None):
        return self._record("point_image", packed, x, y, obs=obs, err=err, mask=mask)


class _Strong(M.ForwardProbModel):
    """A ``ForwardProbModel`` by type with a fixed ``log_prob``: pixels, eight position data, four fluxes, three delays."""
    lp, red = _fixed(20, B), _fixed(21, B).abs()
    include_pixels, include_positions, n_position, n_flux, n_delay = True, True, 8.0, 4.0, 3.0

    def __init__(self):
        pass

    def log_prob(self, simulator, z):
        return self.lp, self.red

    def _n_eff(self, simulator):
        return N_USED


@pytest.fixture(autouse=True)
def on_the_cpu(monkeypatch):
    monkeypatch.setattr(_native, "device", lambda: torch.device("cpu"))


def _catalogue():
    return M.ShearCatalogue([0.5, -1.0, 2.0], [1.0, 0.3, -0.7], [0.01, -0.02, 0.03], [0.0, 0.01, -0.01], 0.3)


def _families():
    return M.ImageFamilies([[1.0, -1.0], [0.5, -0.4]], [[0.0, 0.1], [0.9, -0.8]], 0.02)


# name -> (constructor(strong), the stub result it reads, its value key, its own data count, the gradient keys of its inputs)
MODELS = {
    "shear": (lambda strong=None: M.WeakLensingProbModel(LENS_PRIOR, _catalogue(), strong), "shear", "log_like", 2.0 * N_GAL),
    "image_plane": (lambda strong=None: M.ImagePlaneProbModel(LENS_PRIOR, _families(), strong), "image_plane", "log_like", 2.0 * 4),
    "evidence": (lambda: M.SourceEvidenceProbModel(LENS_PRIOR, OBS, ERR, n_src=(4, 4), pitch=0.1), "evidence", "log_evidence",
                 float(N_USED)),
    "point_image": (lambda: M.PointImageProbModel(IMAGE_PRIOR, OBS, ERR), "point_image", "log_like", float(N_USED)),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_log_prob_is_the_native_value_plus_the_prior(name):
    make, key, value, n_own = MODELS[name]
    pm, sim, res = make(), _Simulator(), _Simulator.results[MODELS[name][1]]
    lp, red = pm.log_prob(sim, Z)
    assert torch.equal(lp, res[value] + pm.log_prior(Z)) and torch.equal(red, res["chi2"] / n_own)
    assert not lp.requires_grad and not red.requires_grad
    called, tensors, kw = sim.last
    assert called == key and torch.equal(tensors[0], sim._pack_partial(pm.pack_bij.forward(pm._flat.forward(Z))))
    if name in ("shear", "image_plane"):
        assert kw["want_grad"] is True  # (these entries are asked for their gradient always)
    if name == "evidence":
        assert kw == dict(obs=pm.observed_image, err=pm.err_map, n_src=(4, 4), pitch=0.1, center=(0.0, 0.0), regularization="gradient",
                          strength=1.0, mask=None)
    if name == "point_image":
        assert torch.equal(tensors[1], pm._flat.forward(Z)[:, :1]) and torch.equal(tensors[2], pm._flat.forward(Z)[:, 1:])


@pytest.mark.parametrize("name", list(MODELS))
def test_log_prob_and_grad_is_the_gradient_of_the_restatement(name):
    make, key, value, n_own = MODELS[name]
    pm, sim, res = make(), _Simulator(), _Simulator.results[key]
    lp, red, g = pm.log_prob_and_grad(sim, Z)
    assert torch.equal(pm.log_prob_and_grad(sim, Z, graph=True)[2], g)  # (accepted and ignored)
    assert not (lp.requires_grad or red.requires_grad or g.requires_grad) and g.shape == Z.shape

    zz = Z.clone().requires_grad_(True)
    x = pm._flat.forward(zz)
    struct = pm.pack_bij.forward(x)
    inputs = [(sim._pack_partial(struct), res["grad"])]
    if name == "point_image":
        inputs += [(struct["point_images"][0]["x"][:, None], res["grad_x"]), (struct["point_images"][0]["y"][:, None], res["grad_y"])]
    ll = res[value]
    for t, grad in inputs:  # value: the stub's; gradient with respect to t: the stub's grad
        lin = (t * grad).sum(dim=tuple(range(1, t.dim())))
        ll = ll + (lin - lin.detach())
    ref = ll + (pm._flat.log_prob(x) + pm._flat.fldj_columns(zz).sum(-1))
    (g_ref,) = torch.autograd.grad(ref.sum(), zz)
    assert torch.equal(lp, res[value] + pm.log_prior(Z)) and torch.equal(red, res["chi2"] / n_own)
    assert torch.equal(g, g_ref) and bool(g.abs().min() > 0)
    # the likelihood's part is there: the prior alone gives another gradient in every column
    (g_prior,) = torch.autograd.grad(pm.log_prior(zz).sum(), zz)
    assert bool(((g - g_prior).abs() > 0).all())


@pytest.mark.parametrize("name", ["shear", "image_plane"])
def test_a_joined_strong_model_carries_the_prior(name):
    make, key, value, n_own = MODELS[name]
    strong, sim, res = _Strong(), _Simulator(), _Simulator.results[key]
    pm = make(strong)
    lp, red = pm.log_prob(sim, Z)
    assert torch.equal(lp, res[value] + strong.lp)
    assert torch.equal(red, (res["chi2"] + strong.red * float(N_USED)) / (n_own + float(N_USED)))
    assert (pm.include_pixels, pm.include_positions, pm.n_position) == (True, True, n_own + 8.0 + 4.0 + 3.0)
    assert (pm.n_flux, pm.n_delay) == (0.0, 0.0)  # (counted inside n_position)
    alone = make()
    assert (alone.include_pixels, alone.include_positions, alone.n_position) == (False, True, n_own)
    strong.include_positions = False  # a pixel-only strong model adds no point data
    assert make(strong).n_position == n_own
    with pytest.raises(TypeError, match="strong must be a ForwardProbModel over the same prior"):
        make(object())


def test_event_size_of_every_model_class():
    """``ModellingSequence._event_size`` = the region's pixel count with ``include_pixels`` + ``n_position + n_flux + n_delay`` with
    ``include_positions``: the figures below are that formula for the ten used pixels of the stub region."""
    sim = _Simulator()
    size = lambda pm: ModellingSequence(None, pm, None)._event_size(sim)
    assert size(MODELS["evidence"][0]()) == 10.0
    assert size(MODELS["point_image"][0]()) == 10.0
    assert size(M.BackwardProbModel(LENS_PRIOR, OBS, 0.1, 100.0)) == 10.0
    assert size(MODELS["shear"][0]()) == 6.0
    assert size(MODELS["shear"][0](_Strong())) == 10.0 + 6.0 + 15.0
    assert size(MODELS["image_plane"][0]()) == 8.0
    assert size(MODELS["image_plane"][0](_Strong())) == 10.0 + 8.0 + 15.0
    assert size(M.ForwardProbModel(LENS_PRIOR, OBS, 0.1, 100.0, include_positions=False)) == 10.0
    xy = [np.asarray([1.0, -1.0, 0.3], np.float32)]
    both = M.ForwardProbModel(LENS_PRIOR, OBS, 0.1, 100.0, centroids_x=xy, centroids_y=xy, centroids_errors_x=[0.01],
                              centroids_errors_y=[0.01], centroids_fluxes=[np.asarray([1.0, np.nan, 0.5], np.float32)],
                              centroids_fluxes_errors=[0.1])
    assert size(both) == 10.0 + 6.0 + 2.0
    for pm in (MODELS["evidence"][0](), MODELS["point_image"][0](), M.BackwardProbModel(LENS_PRIOR, OBS, 0.1, 100.0)):
        assert (pm.include_pixels, pm.include_positions, pm.n_position, pm.n_flux, pm.n_delay) == (True, False, 0.0, 0.0, 0.0)
        assert pm.init_centroids(B) is None


# ---- the autograd glue ----------------------------------------------------------------------------------------------------------
def _entry(calls):
    def fn(a, b, want):
        assert not a.requires_grad and not b.requires_grad
        calls.append(want)
        return (a.sum(1) + b.sum(1), a[:, 0] * 2.0), (torch.full_like(a, 3.0), torch.full_like(b, 5.0))
    return fn


def test_gradfn_asks_for_no_gradient_and_keeps_none_when_no_input_needs_one():
    calls, packed = [], []
    a, b = torch.ones(B, 2), torch.ones(B, 4)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
        out, stat = M._GradFn.apply(_entry(calls), a, b)
    assert calls == [False] and packed == [] and not out.requires_grad and not stat.requires_grad
    assert torch.equal(out, torch.full((B,), 6.0)) and torch.equal(stat, torch.full((B,), 2.0))


def test_gradfn_scales_every_kept_gradient_by_the_cotangent_of_the_first_output():
    calls, packed = [], []
    a, b = torch.ones(B, 2, requires_grad=True), torch.ones(B, 4)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
        out, stat = M._GradFn.apply(_entry(calls), a, b)
    assert calls == [True] and len(packed) == 2 and out.requires_grad and not stat.requires_grad
    w = torch.tensor([1.0, -2.0, 0.5])
    (ga,) = torch.autograd.grad((out * w).sum(), a)
    assert torch.equal(ga, w[:, None] * torch.full((B, 2), 3.0))
    b.requires_grad_(True)
    out, _ = M._GradFn.apply(_entry(calls), a.detach(), b)
    (gb,) = torch.autograd.grad((out * w).sum(), b)
    assert calls == [True, True] and torch.equal(gb, w[:, None] * torch.full((B, 4), 5.0))


@pytest.mark.parametrize("needs_grad", [False, True], ids=["forward_only", "with_gradient"])
def test_the_native_terms_are_forward_only_without_a_gradient_wanted(needs_grad):
    """The pixel term (``model.loglike``) and the point terms (``positions`` and its kin) are asked for their gradient only when
    the packed rows require one."""
    calls = []
    packed = torch.ones(B, P, requires_grad=needs_grad)
    ll, chi2, grad = _fixed(30, B), _fixed(31, B).abs(), _fixed(32, B, P)

    class Native:
        def loglike(self, p, obs, err, mask, bg_rms, exp_time, want):
            calls.append(("loglike", obs, err, mask, bg_rms, exp_time, want))
            return ll.clone(), chi2.clone(), grad if want else None  # (fresh tensors, as every native call returns)

    def positions(p, want):
        calls.append(("positions", want))
        return ll.clone(), chi2.clone(), grad if want else None

    for got in (M._log_like(packed, Native(), "obs", "err", None, 0.0, 1.0), M._point_term(packed, positions)):
        assert torch.equal(got[0], ll) and torch.equal(got[1], chi2) and got[0].requires_grad == needs_grad and not got[1].requires_grad
        if needs_grad:
            (g,) = torch.autograd.grad(got[0].sum(), packed)
            assert torch.equal(g, grad)
    assert calls == [("loglike", "obs", "err", None, 0.0, 1.0, needs_grad), ("positions", needs_grad)]
