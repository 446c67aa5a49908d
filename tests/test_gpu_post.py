"""Every PSF / pooling kernel of csrc/gl_post.hip.h against the float64 convolution of tests/post_cases.py.

Per case the GIGALENS_HIP_CORR_* environment is set before the model is created (the knobs are read there); then the model's own
post-processing is driven directly (gl_post_apply) in both directions on
  * random stacks, compared element by element under the derived bound gamma_n |scale| sum |s_i| |k_i| (post_cases docstring);
  * one impulse per sample at corners, tile edges and the last row / column: every output is float32(Keff) x amplitude x scale to
    two roundings where the reference puts a tap and exactly zero elsewhere -- swapped pair halves, a wrong second sample of an odd
    batch, a wrong workgroup remap or a misplaced class offset fail here at any tolerance;
and the adjoint identity, determinism, the NaN guards around the outputs and the name of the kernel that ran (the library is asked:
a case that moves to another kernel fails instead of losing its coverage) are checked.  Every case runs once."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import post_cases as PC
from tests.test_gpu_parity import gl  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernel_name():
    """mangled symbol (gl_model_last_post_kernel) -> the matrix's spelling"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_flops as isa
    cache = {}

    def name(sym):
        if sym not in cache:
            cache[sym] = PC.short_name(isa.demangle([sym])[0])
        return cache[sym]
    return name


def _set_env(monkeypatch, env):
    for k in PC.ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _simulator(gl, n, ss, psf, bs=2):
    """Any small model will do: the post plan depends on the grid and the PSF only."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.simulator import SimulatorConfig
    cfg = SimulatorConfig(delta_pix=0.08, num_pix=n, supersample=ss)
    return gl.LensSimulator(PhysicalModel([], [Sersic()], []), cfg, bs=bs, supersampled_kernel=psf)


def _apply(m, case, x, transpose):
    """gl_post_apply on `x` (numpy float32): the input view starts case.offset floats after an aligned address; the output is
    pre-filled with NaN and followed by a NaN guard of one image.  Returns the output (numpy) after checking both."""
    dev = m.device
    shape_out = PC.out_shape(case, transpose)
    per = shape_out[1] * shape_out[2]
    flat_in = torch.zeros(x.size + 8, dtype=torch.float32, device=dev)
    assert flat_in.data_ptr() % 16 == 0
    view = flat_in[case.offset:case.offset + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    flat_out = torch.full(((case.batch + 1) * per,), float("nan"), dtype=torch.float32, device=dev)
    out = flat_out[:case.batch * per].view(shape_out)
    m.post_apply(view, out=out, transpose=transpose, scale=case.scale)
    torch.cuda.synchronize()
    res = flat_out.cpu().numpy()
    assert np.isnan(res[case.batch * per:]).all(), "the guard image behind the output was written"
    assert not np.isnan(res[:case.batch * per]).any(), "an output element was not written"
    return res[:case.batch * per].reshape(shape_out)


@pytest.mark.parametrize("case", PC.CASES, ids=[c.id for c in PC.CASES])
def test_post_case(gl, case, kernel_name, monkeypatch):
    _set_env(monkeypatch, case.env)
    psf = PC.make_psf(case)
    m = _simulator(gl, case.n, case.ss, psf)._model
    figures, rand = {}, {}
    for transpose in (False, True):
        tag = "bwd" if transpose else "fwd"
        # ---- random input: element by element under the derived bound; which kernel ran; determinism
        x = PC.random_input(case, transpose)
        y = _apply(m, case, x, transpose)
        seen = kernel_name(m.last_post_kernel(transpose))
        declared = case.bwd if transpose else case.fwd
        assert seen == declared, f"{tag}: launched {seen}, declared {declared}"
        assert np.array_equal(y, _apply(m, case, x, transpose)), f"{tag}: two calls differ"
        ref = PC.post_f64(case, x, transpose, psf)
        bound = PC.error_bound(case, x, transpose, psf)
        err = np.abs(y.astype(np.float64) - ref)
        figures[tag] = float((err / np.maximum(bound, 1e-300)).max())
        rand[tag] = (x.astype(np.float64), y.astype(np.float64), bound)
        # ---- impulses: float32(Keff) x amplitude x scale to two roundings where a tap lands, exactly zero elsewhere
        xi = PC.impulse_input(case, transpose)
        yi = _apply(m, case, xi, transpose).astype(np.float64)
        figures[tag + "_imp"], figures[tag + "_imp_stray"] = PC.impulse_error_in_u(case, xi, yi, transpose, psf)
    print(f"{case.id}: " + " ".join(f"{k} {v:.3g}" for k, v in figures.items()) + "  (fwd / bwd: worst error in units of the bound;"
          " _imp: in units of u)")
    for tag in ("fwd", "bwd"):
        assert figures[tag] <= 1.0, (tag, figures)
        assert figures[tag + "_imp_stray"] == 0, (tag, figures)
        assert figures[tag + "_imp"] <= 2.0 + PC.U, (tag, figures)
    # ---- adjoint: <post(S), G> = <S, post^T(G)> from the GPU's own outputs, within the sum of the two bounds
    (S, yS, bS), (G, yG, bG) = rand["fwd"], rand["bwd"]
    lhs, rhs = float((yS * G).sum()), float((S * yG).sum())
    tol = float((bS * np.abs(G)).sum() + (np.abs(S) * bG).sum())
    print(f"{case.id}: adjoint |lhs - rhs| / tol = {abs(lhs - rhs) / tol:.3g}")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


@pytest.mark.parametrize("case_id", ["s2_13x13_demo", "s1_5x7", "s2_28x27_kh29", "s3_5x5"])
def test_public_paths_launch_the_tested_kernels(gl, case_id, kernel_name, monkeypatch):
    """simulate() and log_prob_and_grad on the case's grid launch the kernels test_post_case drove through gl_post_apply."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import SimulatorConfig
    from gigalens_amd._native import NativeLibraryError
    from tests import helpers as H
    from tests.test_prior_host import default_prior
    case = next(c for c in PC.CASES if c.id == case_id)
    _set_env(monkeypatch, case.env)
    phys = PhysicalModel([EPL(), Shear()], [SersicEllipse()], [SersicEllipse()])
    prior = default_prior()
    cfg = SimulatorConfig(delta_pix=0.08, num_pix=case.n, supersample=case.ss)
    B = 3
    names = lambda m: [kernel_name(m.last_post_kernel(t)) for t in (False, True)]
    sim = gl.LensSimulator(phys, cfg, bs=B, supersampled_kernel=PC.make_psf(case))
    wl = gl.workloads.Workload("POST", phys, prior, cfg, B)
    with pytest.raises(NativeLibraryError, match="no forward post-processing kernel"):
        sim._model.last_post_kernel(False)
    img = sim.simulate(H.sample_packed(wl, sim, seed=4))
    assert torch.isfinite(img).all()
    assert kernel_name(sim._model.last_post_kernel(False)) == case.fwd
    with pytest.raises(NativeLibraryError, match="no transposed post-processing kernel"):
        sim._model.last_post_kernel(True)
    sim2 = gl.LensSimulator(phys, cfg, bs=B, supersampled_kernel=PC.make_psf(case))
    obs = np.random.default_rng(1).normal(size=(case.n, case.n)).astype(np.float32)
    pm = gl.ForwardProbModel(prior, obs, 0.2, 100.0, include_positions=False)
    z = pm.bij.inverse(prior.sample(B, seed=9)).to("cuda")
    lp, _, gz = pm.log_prob_and_grad(sim2, z)
    assert torch.isfinite(lp).all() and torch.isfinite(gz).all()
    assert names(sim2._model) == [case.fwd, case.bwd]


def test_refusals(gl, monkeypatch):
    from gigalens_amd._native import NativeLibraryError
    _set_env(monkeypatch, {})
    # a PSF whose forward tap tile (15 + 113 rows of 129 floats) exceeds 64 KB of LDS: GL_EUNSUPPORTED (-2), nothing is launched
    n = 16
    psf = np.full((113, 113), 1.0 / 113 ** 2, dtype=np.float32)
    m = _simulator(gl, n, 1, psf)._model
    x = torch.zeros((1, n, n), dtype=torch.float32, device=m.device)
    with pytest.raises(NativeLibraryError, match=r"error -2: PSF too large"):
        m.post_apply(x)
    # no PSF, no supersampling: there is no post-processing; GL_EINVAL (-1)
    m = _simulator(gl, n, 1, None)._model
    with pytest.raises(NativeLibraryError, match=r"error -1: the model has no PSF"):
        m.post_apply(x)
    with pytest.raises(NativeLibraryError, match=r"error -1"):
        m.last_post_kernel(False)
    # null and non-positive arguments
    from gigalens_amd import _native
    m = _simulator(gl, n, 2, None)._model
    L, s = _native.lib(), _native._stream()
    out = torch.zeros((1, n, n), dtype=torch.float32, device=m.device)
    xin = torch.zeros((1, 2 * n, 2 * n), dtype=torch.float32, device=m.device)
    assert L.gl_post_apply(m._h, 0, _native._ptr(xin), _native._ptr(out), 0, 1.0, s) == -1
    assert L.gl_post_apply(m._h, -3, _native._ptr(xin), _native._ptr(out), 0, 1.0, s) == -1
    assert L.gl_post_apply(m._h, 1, None, _native._ptr(out), 0, 1.0, s) == -1
    assert L.gl_post_apply(m._h, 1, _native._ptr(xin), None, 0, 1.0, s) == -1
    assert L.gl_post_apply(None, 1, _native._ptr(xin), _native._ptr(out), 0, 1.0, s) == -1
    assert L.gl_post_apply(m._h, 1, _native._ptr(xin), _native._ptr(out), 2, 1.0, s) == -1
    assert L.gl_post_apply(m._h, 1, _native._ptr(xin), _native._ptr(out), 0, 1.0, s) == 0
    torch.cuda.synchronize()
