"""The binding between a ``ForwardProbModel``, a simulator and its native model, without a GPU: which fused entry every public
call reaches and with which arguments (``ForwardProbModel._fused``), when the prior and the image positions are handed over, and
when a captured graph's entry (``model._GraphEntry``) still holds.

The native model is the real ``_native.Model`` over a library that records its calls and does nothing, so the bookkeeping under test
(``prior_owner``, ``positions_owner``, ``generation``, the workspaces) is the code that runs on the GPU; only the two fused entries
are replaced, by ones that record their arguments and return CPU tensors."""
import contextlib
import types

import numpy as np
import pytest
import torch

from gigalens_amd import _native
from gigalens_amd.model import ForwardProbModel, _GraphEntry
from tests import mp_positions_cases as PC

B, N_PIX = 3, 8
WORKSPACE_BYTES = 1000  # per sample, of the library below


class _Library:
    """Every ``gl_*`` symbol: records its name, succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return WORKSPACE_BYTES * args[1] if name == "gl_workspace_bytes" else 0
        return fn


class _RecordingModel(_native.Model):
    def __init__(self):
        super().__init__([], 0, 0, 0, N_PIX, N_PIX, 1, np.zeros(N_PIX * N_PIX), np.zeros(N_PIX * N_PIX), None, 1.0)
        self.fused = []  # (entry, want_grad, chi2_divisor, terms, obs, err, mask, bg_rms, exp_time)

    def _record(self, entry, z, obs, err, mask, bg_rms, exp_time, want_grad, chi2_divisor, terms):
        assert not z.requires_grad
        self.fused.append((entry, want_grad, chi2_divisor, terms, obs, err, mask, bg_rms, exp_time))
        zero = torch.zeros(z.shape[0])
        return zero, zero.clone(), zero.clone(), torch.ones_like(z) if want_grad else None

    def logprob(self, *args):
        return self._record("logprob", *args)

    def multiplane_logprob(self, *args):
        return self._record("multiplane_logprob", *args)


@pytest.fixture
def library(monkeypatch):
    lib = _Library()
    monkeypatch.setattr(_native, "lib", lambda: lib)
    monkeypatch.setattr(_native, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return lib


def _simulator(planes, masked=False):
    """What ``ForwardProbModel`` reads of a ``LensSimulator``, around a recording native model."""
    c = PC.case("k2")
    phys = c["phys_mp"] if planes else c["phys"]
    region = torch.ones(N_PIX, N_PIX)
    return types.SimpleNamespace(_model=_RecordingModel(), _layout=phys._packing(), phys_model=phys, img_region=region,
                                 sim_config=types.SimpleNamespace(pix_region=region.numpy() if masked else None),
                                 _mp=phys.multiplane, _n_eff=None, _linear_cols_dev=None, _lp_graphs={}, _lp_captures=0)


def _prob_model(terms, planes, sigma=0.01, **kw):
    from gigalens_amd import prior as tfd
    c = PC.case("k2")
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), sigma) for k, v in d.items()}) for d in c["params"]["lens_mass"]])))
    args = dict(include_pixels=bool(terms & 1), include_positions=bool(terms & 2))
    if terms & 1:
        args.update(observed_image=np.zeros((N_PIX, N_PIX), np.float32), background_rms=0.2, exp_time=100.0)
    if terms & 2:
        args.update(PC.centroids(c))
        if not planes:  # one plane, no MultiPlane: the families sit on the source plane
            args["centroids_redshifts"] = None
    args.update(kw)
    return ForwardProbModel(prior, **args)


def _z(pm, requires_grad=False):
    return torch.zeros(B, len(pm._paths), requires_grad=requires_grad)


# ---- the dispatch table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True], ids=["one_plane", "planes"])
@pytest.mark.parametrize("terms", [1, 2, 3], ids=["pixels", "positions", "both"])
def test_every_public_call_reaches_the_one_fused_entry(library, planes, terms):
    """``log_prob`` (with and without a gradient wanted), ``log_prob_and_grad`` and ``term_log_prob_and_grad`` of each term the model
    has: the native entry, ``want_grad``, ``terms``, the divisor (the region's pixel count with the pixel term, else 1) and the image
    arguments."""
    sim, pm = _simulator(planes), _prob_model(terms, planes)
    model = sim._model
    entry = "multiplane_logprob" if planes else "logprob"
    divisor = lambda t: float(N_PIX * N_PIX) if t & 1 else 1.0
    image = (pm.observed_image, None, None, pm.background_rms or 0.0, pm.exp_time or 1.0)
    assert (image[3:] == (float(np.float32(0.2)), 100.0)) if terms & 1 else (image == (None, None, None, 0.0, 1.0))

    lp, red = pm.log_prob(sim, _z(pm))
    assert model.fused.pop() == (entry, False, divisor(terms), terms) + image and not lp.requires_grad
    z = _z(pm, requires_grad=True)
    lp, red = pm.log_prob(sim, z)
    assert model.fused.pop() == (entry, True, divisor(terms), terms) + image
    lp.sum().backward()
    assert torch.equal(z.grad, torch.ones_like(z)) and not red.requires_grad
    out = pm.log_prob_and_grad(sim, _z(pm))
    assert model.fused.pop() == (entry, True, divisor(terms), terms) + image and len(out) == 3
    for name, bit in (("pixels", 1), ("positions", 2)):
        if terms & bit:
            out = pm.term_log_prob_and_grad(sim, _z(pm), name)
            assert model.fused.pop() == (entry, True, divisor(bit), bit) + image and len(out) == 3
    assert model.fused == []
    # handed over once for all of these calls, the positions only by a model that has them
    assert library.calls.count("gl_model_set_prior") == 1
    assert library.calls.count("gl_model_set_positions") == (1 if terms & 2 else 0)
    assert library.calls.count("gl_model_set_position_targets") == (1 if terms & 2 and planes else 0)
    assert model.prior_owner is pm and model.positions_owner is (pm if terms & 2 else None)


def test_the_mask_is_the_region_when_the_configuration_has_one(library):
    sim, pm = _simulator(False, masked=True), _prob_model(1, False)
    pm.log_prob_and_grad(sim, _z(pm))
    assert sim._model.fused.pop()[4:7] == (pm.observed_image, None, sim.img_region)
    err = _prob_model(1, False, error_map=np.ones((N_PIX, N_PIX), np.float32))
    err.log_prob_and_grad(sim, _z(err))
    assert sim._model.fused.pop()[4:] == (err.observed_image, err.error_map, sim.img_region, 0.0, 1.0)


def test_the_position_term_alone_binds_no_positions_for_the_pixel_term(library):
    """``term_log_prob_and_grad(..., "pixels")`` of a model with both terms: the positions are handed over by the first call that
    has the position term on."""
    sim, pm = _simulator(False), _prob_model(3, False)
    pm.term_log_prob_and_grad(sim, _z(pm), "pixels")
    assert library.calls.count("gl_model_set_positions") == 0 and sim._model.positions_owner is None
    pm.term_log_prob_and_grad(sim, _z(pm), "positions")
    assert library.calls.count("gl_model_set_positions") == 1 and sim._model.positions_owner is pm


@pytest.mark.parametrize("planes", [False, True], ids=["one_plane", "planes"])
def test_the_prior_is_handed_over_again_only_after_another_model_bound(library, planes):
    sim, a, b = _simulator(planes), _prob_model(3, planes), _prob_model(3, planes, sigma=0.02)
    count = lambda name: library.calls.count(name)
    for _ in range(3):
        a.log_prob_and_grad(sim, _z(a))
    assert (count("gl_model_set_prior"), count("gl_model_set_positions")) == (1, 1)
    b.log_prob(sim, _z(b))
    assert (count("gl_model_set_prior"), count("gl_model_set_positions")) == (2, 2) and sim._model.prior_owner is b
    b.log_prob(sim, _z(b))
    a.log_prob_and_grad(sim, _z(a))
    a.term_log_prob_and_grad(sim, _z(a), "positions")
    assert (count("gl_model_set_prior"), count("gl_model_set_positions")) == (3, 3)
    assert sim._model.prior_owner is a and sim._model.positions_owner is a


def test_refusals_on_lens_planes(library):
    sim = _simulator(True)
    none = _prob_model(0, True)
    for call in (lambda: none.log_prob(sim, _z(none)), lambda: none.log_prob_and_grad(sim, _z(none)),
                 lambda: none.term_log_prob_and_grad(sim, _z(none), "pixels")):
        with pytest.raises(_native.UnsupportedLensError, match="2 lens planes and no likelihood term"):
            call()
    unplaced = _prob_model(3, True, centroids_redshifts=None)
    for call in (lambda: unplaced.log_prob(sim, _z(unplaced)), lambda: unplaced.log_prob_and_grad(sim, _z(unplaced)),
                 lambda: unplaced.term_log_prob_and_grad(sim, _z(unplaced), "pixels")):
        with pytest.raises(_native.UnsupportedLensError, match="its image positions need centroids_redshifts"):
            call()
    pixels = _prob_model(1, True)
    with pytest.raises(_native.UnsupportedLensError, match="the model carries no image positions"):
        pixels.term_log_prob_and_grad(sim, _z(pixels), "positions")
    assert sim._model.fused == [] and library.calls.count("gl_model_set_prior") == 0  # refused before anything was handed over


# ---- what a captured graph's entry checks ---------------------------------------------------------------------------------------
def _entry(pm, sim, terms):
    """The entry a capture of ``pm`` on ``sim`` would leave (no graph: the decision alone is under test)."""
    z = _z(pm)
    pm._fused(sim, z, True, terms)
    return _GraphEntry(None, z, None, pm, sim, terms)


@pytest.mark.parametrize("terms", [1, 3], ids=["pixels", "both"])
def test_an_entry_holds_until_the_native_model_is_bound_again(library, terms):
    sim, pm, other = _simulator(False), _prob_model(terms, False), _prob_model(terms, False, sigma=0.02)
    model = sim._model
    ent = _entry(pm, sim, terms)
    assert ent.valid(sim)
    pm.log_prob_and_grad(sim, _z(pm))  # its own calls, other batch sizes and workspaces included, change nothing
    pm.log_prob(sim, torch.zeros(1, len(pm._paths)))
    model._workspace(1)
    assert ent.valid(sim) and ent.generation == model.generation

    changes = {
        "set_prior by another model": lambda: other._bind_prior(sim),
        "set_positions": lambda: model.set_positions([np.zeros(2)], [np.zeros(2)], [np.ones(2)], [np.ones(2)]),
        "set_source_scales": lambda: model.set_source_scales([1.0]),
        "set_timing": lambda: model.set_timing(4, 2),
        "a replaced observed_image": lambda: setattr(pm, "observed_image", pm.observed_image.clone()),
    }
    for what, change in changes.items():
        ent = _entry(pm, sim, terms)
        assert ent.valid(sim), what
        change()
        assert not ent.valid(sim), what
        pm._fused(sim, _z(pm), True, terms)  # binding again does not bring the freed buffers back
        assert not ent.valid(sim), what
    if terms & 2:
        ent = _entry(pm, sim, terms)
        other._bind_positions(sim)
        assert model.prior_owner is pm and not ent.valid(sim)


def test_every_setter_moves_the_generation_and_only_some_drop_the_workspace(library):
    model = _RecordingModel()
    model.N = 4
    on_gpu = types.SimpleNamespace(is_cuda=True, shape=(3, 2, 4), contiguous=lambda: on_gpu, data_ptr=lambda: 0)
    setters = [  # (call, the workspace layout follows it)
        (lambda: model.set_catalogue(0, 1, (0, 1, 2), np.zeros((2, 3))), True),
        (lambda: model.set_light_image(0, np.zeros((2, 2))), False),
        (lambda: model.set_source_scales([1.0]), True),
        (lambda: model.set_lens_planes([0], np.zeros((1, 1)), np.zeros((1, 1))), True),
        (lambda: model.set_position_targets(np.zeros((1, 1))), False),
        (lambda: model.set_position_scales([1.0]), False),
        (lambda: model.set_position_fluxes([1.0, 2.0], [0.1, 0.1]), False),
        (lambda: model.set_position_fluxes(None, None), False),
        (lambda: model.set_series(0, 1.0, on_gpu), False),
        (lambda: model.set_series_hessian(0, on_gpu), False),
        (lambda: model.set_prior([], np.zeros(0)), False),
        (lambda: model.set_positions([np.zeros(2)], [np.zeros(2)], [np.ones(2)], [np.ones(2)]), True),
        (lambda: model.set_timing(1, 1), False),
    ]
    for k, (call, layout) in enumerate(setters):
        ws = model._workspace(2)
        model.prior_owner, model.positions_owner = "p", "q"
        call()
        assert model.generation == k + 1
        assert (model._ws == {}) if layout else (model._workspace(2) is ws), k
        # set_prior (10) and set_positions (11) take the binding from its owner, nothing else does
        assert (model.prior_owner, model.positions_owner) == ((None, "q") if k == 10 else ("p", None) if k == 11 else ("p", "q")), k


def test_the_workspace_holds_one_batch_size_at_a_time(library):
    sim, pm = _simulator(False), _prob_model(1, False)
    model = sim._model
    ent = _entry(pm, sim, 1)
    ws3 = model._workspace(B)
    assert ent.workspace is ws3 and ws3.numel() == WORKSPACE_BYTES * B and list(model._ws) == [B]
    ws2 = model._workspace(2)
    assert list(model._ws) == [2] and model._workspace(2) is ws2
    assert model._workspace(B) is not ws3 and list(model._ws) == [B]  # dropped by the model; the entry keeps the one it captured
    assert ent.workspace is ws3 and ent.valid(sim)
    assert model._scratch("lstsq", 10) is model._scratch("lstsq", 200) and model._scratch("lstsq", 300).numel() == 300
    assert list(model._scratch_bufs) == ["lstsq"]
