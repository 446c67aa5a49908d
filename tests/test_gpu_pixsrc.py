"""LensSimulator.reconstruct_source (csrc/gl_pixsrc.hip.h) on the GPU against the float64 restatement of tests/pixsrc_cases.py.

Cases (tests/pixsrc_cases.py ``case``; shapes where the kernels can go wrong, not workload size):
  A    SIE + Shear | Sersic lens light, 12 x 10 at supersample 2, 5 x 3 Gaussian PSF (``supersampled_kernel``), 7 x 6 nodes, B = 3 with
       per-sample pitch and centre, an L-shaped corner masked; curvature, strengths 2, 1, 4; noise rms 0.02
  B    EPL + Shear, 40 x 36, 3 x 3 PSF, 33 x 31 = 1023 nodes, B = 2; gradient, strengths [[1, 10, 100], [2, 20, 200]]; noise rms 0.05
  C11, C21   no PSF, supersample 1, 9 x 8, 1 x 1 and 2 x 1 nodes, B = 1; identity, strength 0.5; noise rms 0.01
  D    11 x 13 at supersample 2, 3 x 3 PSF, 5 x 9 nodes centred at x = 0.27 (half of the rays miss the grid), B = 3: a regular SIE,
       an SIE at e = 0 (every deflection NaN: all rows zero, the source exactly zero) and an SIE centred exactly on a supersampled
       pixel (NaN at that pixel alone); gradient, strength 3; noise rms 0.02
Observed images: the float64 restatement's ``lens light + F s_true`` of a smooth ``s_true`` plus seeded Gaussian noise at ``err_map``.

Value gates ("gate = 4 x that"): the yardstick of a quantity is the error of the restatement run in float32 on
the CPU against float64 -- arrays normalised by their largest absolute element, scalars by ``|chi2| + |log_det| + S`` -- taken, as
in tests/test_gpu_interp.py, as the worst over the cases of this file; the gate is 4 x that, printed with the kernel's error before
it is asserted.  With the strengths and noise levels above the reference has ``cond(M)`` between 1 and 431 (<= 1e4 asserted) and
the gates are of order 1e-6 (<= 1e-2 for ``source``, <= 1e-3 for the rest asserted): neither can hide a failure."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pixsrc_cases as PC
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = PC.ARRAYS + PC.SCALARS
_RUNS = {}


def _tensors(params):
    return {g: [{k: torch.as_tensor(v) for k, v in d.items()} for d in lst] for g, lst in params.items()}


def _sim(gl, c):
    return gl.LensSimulator(c["phys"], c["cfg"], bs=c["B"], supersampled_kernel=c["psf"])


def _call(sim, c, obs, err, **over):
    return sim.reconstruct_source(_tensors(c["params"]), obs, err, **{**c["kw"], **over})


def _run(gl, name):
    """One GPU call per case, shared by the tests (left unchanged)."""
    if name not in _RUNS:
        c, obs, err, _, _ = PC.data(name)
        sim = _sim(gl, c)
        _RUNS[name] = (sim, {k: v.cpu().numpy() for k, v in _call(sim, c, obs, err).items()})
    return _RUNS[name]


def _S(c):
    return int(np.prod(c["kw"]["n_src"]))


@pytest.fixture(scope="module")
def gates():
    """4 x the worst float32-restatement error over this file's cases, per quantity."""
    worst = {k: 0.0 for k in KEYS}
    for name in PC.CASES:
        c, _, _, ref, f32 = PC.data(name)
        e = PC.errors(f32, ref, _S(c))
        print(f"float32 yardstick {name}: " + ", ".join(f"{k} {e[k]:.3e}" for k in KEYS))
        worst = {k: max(worst[k], e[k]) for k in KEYS}
    print("float32 yardstick maxima: " + ", ".join(f"{k} {worst[k]:.3e}" for k in KEYS))
    return {k: 4 * v for k, v in worst.items()}


def test_conditions_on_the_reference(gates):
    """What keeps a gate from hiding a failure, asserted on the reference alone."""
    for name in PC.CASES:
        _, _, _, ref, f32 = PC.data(name)
        assert ref["ok"].all() and f32["ok"].all()
        assert np.all(ref["cond"] <= 1e4), (name, ref["cond"])
    assert gates["source"] <= 1e-2
    for k in KEYS[1:]:
        assert gates[k] <= 1e-3, (k, gates[k])


@pytest.mark.parametrize("name", PC.CASES)
def test_values_against_float64(gl, gates, name):
    c, _, _, ref, _ = PC.data(name)
    _, got = _run(gl, name)
    assert got["ok"].all()
    for k in KEYS + ("ok",):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    e = PC.errors(got, ref, _S(c))
    for k in KEYS:
        print(f"{name} {k}: kernel error {e[k]:.3e}, gate {gates[k]:.3e}")
    for k in KEYS:
        assert e[k] <= gates[k], (name, k, e[k], gates[k])


def test_nan_rays_have_zero_rows(gl):
    """Case D: the sample whose every deflection is NaN (SIE at e = 0) reconstructs the zero source exactly, and stays finite."""
    _, got = _run(gl, "D")
    assert np.all(got["source"][1] == 0) and np.all(got["model_image"][1] == 0)
    assert np.isfinite(got["log_evidence"]).all() and np.abs(got["source"][2]).max() > 0


def test_model_image_is_the_interpolated_render(gl):
    """Two independent GPU paths: ``model_image - lens light`` on the used pixels == ``simulate_images`` of a second simulator with
    the same lens whose one source is ``Interpolated(returned source, order=1)`` at the same pose (gate: the image gate of
    tests/test_gpu_interp.py)."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light import Interpolated
    from tests import test_gpu_interp as TI
    im_gate = 4 * max(TI._case(n)["im_yard"] for n in TI.CASES)
    c, _, _, _, _ = PC.data("A")
    sim, got = _run(gl, "A")
    params = _tensors(c["params"])
    ll = sim.simulate_lens_light(params).cpu().numpy()
    used = c["kw"]["mask"]
    for b in range(c["B"]):
        phys = PhysicalModel(list(c["phys"].lenses), [], [Interpolated(got["source"][b], order=1)])
        sim2 = gl.LensSimulator(phys, c["cfg"], bs=c["B"], supersampled_kernel=c["psf"])
        src = dict(center_x=torch.as_tensor(c["kw"]["center"][0]), center_y=torch.as_tensor(c["kw"]["center"][1]),
                   phi=torch.zeros(c["B"]), scale=torch.as_tensor(c["kw"]["pitch"]), amp=torch.ones(c["B"]))
        want = sim2.simulate_images({"lens_mass": params["lens_mass"], "source_light": [src]}).cpu().numpy()[b]
        diff = (got["model_image"][b] - ll[b]) - want
        e = np.abs(diff[used]).max() / np.abs(want).max()
        print(f"sample {b}: identity error {e:.3e}, gate {im_gate:.3e}")
        assert e <= im_gate
        assert np.array_equal(got["model_image"][b][~used], ll[b][~used])  # the lens light alone off the used pixels


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS + ("ok",))


@pytest.mark.parametrize("name", ["A", "B"])
def test_deterministic(gl, name):
    c, obs, err, _, _ = PC.data(name)
    sim, first = _run(gl, name)
    again = {k: v.cpu().numpy() for k, v in _call(sim, c, obs, err).items()}
    assert _same_bits(first, again)


def test_scan_columns_equal_single_calls(gl):
    c, obs, err, _, _ = PC.data("B")
    sim, scan = _run(gl, "B")
    for l in range(3):
        one = {k: v.cpu().numpy() for k, v in _call(sim, c, obs, err, strength=c["kw"]["strength"][:, l]).items()}
        assert _same_bits({k: scan[k][:, l] for k in scan}, one), l


def test_broken_pivot_is_flagged_not_raised(gl):
    """A sample whose ``err_map`` = 1e-25 and ``strength`` = 1e-30 (float32 overflows 1 / sigma^2 times the operator squared: the
    normal matrix is not finite; checked on the float32 restatement first) comes back ``ok == False`` with NaN outputs, no error;
    the healthy sample beside it has exactly the bits it has alone."""
    c, obs, err, _, _ = PC.data("C21")
    c2 = dict(c, B=2, params={g: [{k: np.repeat(v, 2) for k, v in d.items()} for d in lst] for g, lst in c["params"].items()})
    obs2 = np.repeat(obs, 2, axis=0)
    err2 = np.stack([np.full_like(err, 1e-25), err])
    lam2 = np.asarray([1e-30, c["kw"]["strength"][0]], dtype=np.float32)
    f32 = PC.reconstruct(c2["phys"], c2["cfg"], c2["psf"], c2["params"], obs2, err2, **{**c["kw"], "strength": lam2}, dtype=torch.float32)
    assert f32["ok"].tolist() == [False, True]
    sim2 = _sim(gl, c2)
    got = {k: v.cpu().numpy() for k, v in _call(sim2, c2, obs2, err2, strength=lam2).items()}
    assert got["ok"].tolist() == [False, True]
    assert all(np.isnan(got[k][0]).all() for k in KEYS)
    _, alone = _run(gl, "C21")
    assert all(np.array_equal(got[k][1], alone[k][0]) for k in KEYS)


def test_refusals(gl):
    c, obs, err, _, _ = PC.data("A")
    sim, _ = _run(gl, "A")
    with pytest.raises(ValueError, match="nodes"):
        _call(sim, c, obs, err, n_src=(33, 32))
    with pytest.raises(ValueError, match="strength"):
        _call(sim, c, obs, err, strength=0.0)
    with pytest.raises(ValueError, match="strength"):
        _call(sim, c, obs, err, strength=np.asarray([1.0, float("nan"), 1.0]))
    with pytest.raises(ValueError, match="pitch"):
        _call(sim, c, obs, err, pitch=-0.1)
    with pytest.raises(ValueError, match="regularization"):
        _call(sim, c, obs, err, regularization="laplace")
    bad = err.copy()
    bad[6, 6] = 0.0
    with pytest.raises(ValueError, match="err_map"):
        _call(sim, c, obs, bad)
    bad[6, 6], bad[0, 0] = err[6, 6], 0.0  # a masked pixel may hold anything
    assert _call(sim, c, obs, bad)["ok"].all()
    with pytest.raises(ValueError, match="observed_image"):
        _call(sim, c, obs[:, :5], err)
    with pytest.raises(ValueError, match="mask"):
        _call(sim, c, obs, err, mask=np.ones((3, 3), dtype=bool))
    with pytest.raises(ValueError, match="strength"):
        _call(sim, c, obs, err, strength=np.ones((2, 2), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        sim.reconstruct_source(_tensors(c["params"]), torch.as_tensor(obs).requires_grad_(True), err, **c["kw"])
    p = _tensors(c["params"])
    p["lens_mass"][0]["theta_E"] = p["lens_mass"][0]["theta_E"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        sim.reconstruct_source(p, obs, err, **c["kw"])
    # a series-expansion lens maps the simulator's own grid only: with a pix_region the full frame is another grid
    wl = gl.workloads.make("C6S", num_pix=16, batch=2, n_galaxies=4, n_sources=1)
    region = np.ones((16, 16))
    region[0, 0] = 0
    sim_s = gl.LensSimulator(wl.phys_model, dataclasses.replace(wl.sim_config, pix_region=region), bs=2)
    with pytest.raises(ValueError, match="series-expansion"):
        sim_s.reconstruct_source(H.sample_packed(wl, sim_s, seed=1), np.zeros((16, 16), np.float32), np.ones((16, 16), np.float32),
                                 n_src=(4, 4), pitch=0.1)
