"""Every compile-time-specialised main-kernel instantiation against the float64 oracle (tests/dispatch_cases.py).

Per case: the GIGALENS_HIP_* environment is set before the model is created (the knobs are read there), then the four calls of
test_gpu_parity.py::test_dispatched_kernels_do_not_spill run -- simulate [IMG_FWD], its VJP [IMG_BWD], the log-likelihood
[LL_FWD] and the fused forward + gradient [LL_GRAD].  After each, the library is asked which kernel it launched, and that must
be the one the case declares: coverage that moves to another kernel fails here instead of vanishing.  Every mode is compared
with the oracle under the gates of test_gpu_parity.py::test_simulate_loglike_grad_vs_oracle (gradients: with the float32
conditioning allowance of test_psf_supersample_vs_oracle); the VJP against torch.autograd of the oracle image contracted with the
same cotangent."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import dispatch_cases as DC
from tests import helpers as H
from tests.test_gpu_parity import GRAD_RTOL_COL, IMG_RTOL, LL_RTOL, gl  # noqa: F401  (gl: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernel_name():
    """mangled symbol (gl_model_last_main_kernel) -> the matrix's demangled spelling"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_flops as isa
    cache = {}

    def name(sym):
        if sym not in cache:
            cache[sym] = DC.short_name(isa.demangle([sym])[0])
        return cache[sym]
    return name


def _oracle_vjp(wl, packed64, cot, grid_shift=None):
    """d <simulate(theta), cot> / d theta of the float64 oracle image (``grid_shift`` as in helpers.oracle_loglike_and_grad)."""
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, wl.batch, dtype=torch.float64)
    if grid_shift is not None:
        rs.img_X = rs.img_X + torch.as_tensor(grid_shift[0], dtype=torch.float64)
        rs.img_Y = rs.img_Y + torch.as_tensor(grid_shift[1], dtype=torch.float64)
    p = packed64.clone().requires_grad_(True)
    img = rs.simulate(H.struct_from_packed(wl.phys_model, p))
    (g,) = torch.autograd.grad((img * cot.reshape(img.shape)).sum(), p)
    return g.numpy()


def _vjp_conditioning_bound(wl, packed64, cot, g_o, S, seed=0):
    """helpers.float32_conditioning_bound for the VJP: the same displacements of the oracle's grid by one float32 ulp of the
    coordinates, applied to <simulate(theta), cot>."""
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, 1, dtype=torch.float64)
    d = float(np.spacing(np.float32(float(max(rs.img_X.abs().max(), rs.img_Y.abs().max())))))
    rng = np.random.default_rng(seed)
    n_pts = rs.img_X.shape[0]
    shifts = [(d, d), (d, -d), (d * rng.normal(size=(n_pts, 1)), d * rng.normal(size=(n_pts, 1))),
              (d * rng.normal(size=(n_pts, 1)), d * rng.normal(size=(n_pts, 1)))]
    out = np.zeros_like(g_o)
    for sh in shifts:
        out = np.maximum(out, np.abs(_oracle_vjp(wl, packed64, cot, sh) - g_o) / np.maximum(S, 1e-300))
    return out


def check_case_vs_oracle(gl, case, kernel_name, wl=None):
    """Run the four modes of `case` (environment already set) on its workload (default: DC.workload(case)), check the launched
    kernels and compare each mode with the oracle.  Returns the measured errors and the number of gradient elements that needed
    the conditioning allowance."""
    wl = DC.workload(case) if wl is None else wl
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=11)
    mask = sim.img_region if case.pix_region else None
    n_eff = float(torch.count_nonzero(sim.img_region))
    m = sim._model
    gen = torch.Generator(device="cpu")
    gen.manual_seed(5)

    seen = []
    img = m.simulate_fwd(packed)
    seen.append(kernel_name(m.last_main_kernel()))
    cot = (torch.rand(img.shape, generator=gen, dtype=torch.float64) + 0.5)  # fixed random cotangent of the VJP
    g_vjp = m.simulate_bwd(packed, cot.float().to(img.device))
    seen.append(kernel_name(m.last_main_kernel()))
    ll_f, chi2_f, _ = m.loglike(packed, obs, err, mask, wl.background_rms, wl.exp_time, False)
    seen.append(kernel_name(m.last_main_kernel()))
    ll_g, chi2_g, g = m.loglike(packed, obs, err, mask, wl.background_rms, wl.exp_time, True)
    seen.append(kernel_name(m.last_main_kernel()))
    assert seen == list(case.kernels), "\n".join(f"{mode}: launched {s}\n{' ' * len(mode)}  declared {k}"
                                                 for mode, s, k in zip(DC.MODES, seen, case.kernels) if s != k)

    obs_np = obs.cpu().numpy()
    err_np = None if err is None else err.cpu().numpy()
    p64 = packed.cpu().double()
    ll_o, red_o, g_o, img_o = H.oracle_loglike_and_grad(wl, p64, obs_np, err_np, wl.batch)
    assert np.isfinite(ll_o).all() and np.isfinite(g_o).all()
    g_vjp_o = _oracle_vjp(wl, p64, cot)

    img = img.cpu().numpy().reshape(img_o.shape)
    ll_f, ll_g = ll_f.cpu().numpy(), ll_g.cpu().numpy()
    red_f, red_g = chi2_f.cpu().numpy() / n_eff, chi2_g.cpu().numpy() / n_eff
    g, g_vjp = g.cpu().numpy(), g_vjp.cpu().numpy()
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    res = dict(img=float(np.abs(img - img_o).max() / np.abs(img_o).max()), ll_fwd=rel(ll_f, ll_o), ll_grad=rel(ll_g, ll_o),
               red_fwd=rel(red_f, red_o), red_grad=rel(red_g, red_o), grad=float(H.grad_col_err(g, g_o).max()),
               vjp=float(H.grad_col_err(g_vjp, g_vjp_o).max()))
    print(f"{case.id}: " + " ".join(f"{k} {v:.2e}" for k, v in res.items()))

    # IMG_FWD
    assert np.abs(img - img_o).max() <= IMG_RTOL * np.abs(img_o).max() + 1e-7, res
    if case.pix_region:
        outside = (sim.img_region == 0).cpu().numpy()
        assert np.all(img.reshape(-1, *outside.shape)[:, outside] == 0)
    # IMG_BWD and LL_GRAD gradients: the gate of test_gpu_parity.py::test_psf_supersample_vs_oracle -- every element within
    # GRAD_RTOL_COL of its column's scale, or, beyond it, within 4 x what one float32 rounding of beta = x - alpha does to that
    # element of the oracle's own gradient (helpers.grad_gate): a sample whose source maps next to a pixel or a shapelet table node
    # has gradient elements with condition numbers of 1e3-1e4 in that rounding, whatever the formulation (measured: four cases of
    # the matrix have elements beyond GRAD_RTOL_COL, at 0.7-1.1 x the bound; in the two shapelet ones the interpreter and the
    # tile kernels give those elements the same errors)
    ok, rep = H.grad_gate(g_vjp, g_vjp_o, GRAD_RTOL_COL, lambda S: _vjp_conditioning_bound(wl, p64, cot, g_vjp_o, S))
    assert ok, ("IMG_BWD", rep, res)
    res["vjp_conditioned"] = rep["conditioned"]
    # LL_FWD and LL_GRAD: value and reduced chi^2 against the oracle, and against each other
    for ll, red in ((ll_f, red_f), (ll_g, red_g)):
        assert np.allclose(ll, ll_o, rtol=LL_RTOL), res
        assert np.allclose(red, red_o, rtol=LL_RTOL), res
    assert np.allclose(ll_f, ll_g, rtol=LL_RTOL), res
    ok, rep = H.grad_gate(g, g_o, GRAD_RTOL_COL,
                          lambda S: H.float32_conditioning_bound(wl, p64, obs_np, err_np, wl.batch, g_o, S))
    assert ok, ("LL_GRAD", rep, res)
    res["grad_conditioned"] = rep["conditioned"]
    print(f"{case.id}: conditioned elements: vjp {res['vjp_conditioned']} grad {res['grad_conditioned']}")
    return res


def check_basis_vs_oracle(gl, case, kernel_name, wl=None):
    """The basis stack of lstsq (IMG_BASIS) of `case` against the oracle's, under the gate of
    test_gpu_lstsq.py::test_lstsq_simulate_vs_oracle; outside a pixel region the stack is exactly 0.  The stack is asked for with
    an observation and an error map, so the fused shapelet normal-matrix path (no stack) cannot take over.  Before the checked call
    every 32-bit word of the workspace the stack is rendered into is set to 1 (float 1.4e-45; harmless as any index or count the
    workspace holds): a stack pixel the call does not write -- outside the region, the zeroing gl_lstsq_fwd owes it -- is not 0."""
    from oracle import ref_torch as ref
    wl = DC.workload(case) if wl is None else wl
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=11)
    m = sim._model
    n = wl.sim_config.num_pix
    obs = torch.zeros((n, n), dtype=torch.float32, device=packed.device)
    err = torch.ones_like(obs)
    m.lstsq(packed, obs, err, 7, "stacked")  # sizes the workspace
    ws = m._lstsq_ws
    ws[:ws.numel() // 4 * 4].view(torch.int32).fill_(1)
    (st,) = m.lstsq(packed, obs, err, 7, "stacked")
    seen = kernel_name(m.last_main_kernel())
    assert [seen] == list(case.kernels), f"{DC.BASIS_MODE}: launched {seen}\n  declared {case.kernels[0]}"
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, wl.batch, dtype=torch.float64)
    st_o = ref.lstsq_simulate(rs, H.struct_from_packed(wl.phys_model, packed.cpu().double()), None, None, return_stacked=True)
    st_o = st_o.permute(0, 3, 1, 2)  # (bs, depth, H, W), the native layout
    st = st.cpu().double()
    assert st.shape == st_o.shape, (st.shape, st_o.shape)
    assert torch.isfinite(st_o).all()
    sc = st_o.abs().amax(dim=(2, 3), keepdim=True)
    err_st = float(((st - st_o).abs() / (5e-5 * sc + 1e-7)).max())
    print(f"{case.id}: stack error {err_st:.2f} x the gate")
    assert torch.all((st - st_o).abs() <= 5e-5 * sc + 1e-7), err_st
    if case.pix_region:
        outside = sim.img_region.cpu() == 0
        assert torch.all(st[:, :, outside] == 0)
    return dict(stack=err_st)


@pytest.mark.parametrize("case", DC.CASES, ids=[c.id for c in DC.CASES])
def test_dispatch_case_vs_oracle(gl, case, kernel_name, monkeypatch):
    for k in DC.ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    check_case_vs_oracle(gl, case, kernel_name)


@pytest.mark.parametrize("case", DC.GENERIC_CASES, ids=[c.id for c in DC.GENERIC_CASES])
def test_generic_dispatch_case_vs_oracle(gl, case, kernel_name, monkeypatch):
    """The interpreter, the cluster kernels and the basis stack (launch_generic) against the float64 oracle, one case per
    instantiation and edge (tests/dispatch_cases.py::GENERIC_CASES)."""
    for k in DC.ENV_KNOBS + DC.GENERIC_ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if case.basis:
        check_basis_vs_oracle(gl, case, kernel_name)
    else:
        check_case_vs_oracle(gl, case, kernel_name)
