"""Every linear-solve kernel of csrc/gl_lstsq.hip.h against the float64 normal-equation solve of tests/lstsq_cases.py.

Per case the product's own solve is driven on a synthetic basis stack (gl_lstsq_solve_stack: the function gl_lstsq_fwd runs after
rendering its stack), with the workspace pre-filled with NaN bits and a NaN guard behind the coefficients.  Checked:
  * the three launched kernels are the declared ones (the library is asked: a case that moves to another kernel fails);
  * every lower-triangle element of the summed augmented normal matrix against float64 under the derived bound
    gamma_m sum_p |X_ip| |X_jp| (lstsq_cases docstring; columns D + 1 .. Dp - 1 are not read);
  * where nothing is cut: the residual |A^ c - r^| against the GPU's own float32 matrix A^ at rounding level, and the forward error
    against float64 pinv(A^) within 30 cond 6e-8 + 1e-6 (the constants of tests/test_eigh_host.py);
  * gap systems: X c equals the float64 projection (2e-4), duplicates share their amplitude (1e-4 of it: test_eigh_host's
    rank-deficient case), every null direction -- the zero column, the difference of a duplicate pair -- carries at most
    u lambda_max / lambda_min max |c| (lstsq_cases.null_bound: rounding level for the body's condition), the attempt refused;
  * the Cholesky flags wherever float64 decides them; an empty sample is exactly 0; a NaN sample is all NaN and leaves its
    neighbours bitwise alone; masked pixels count for nothing; a second run is bitwise equal."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import lstsq_cases as LC
from tests.test_gpu_parity import gl  # noqa: F401  (the module fixture)
from tests.test_lstsq_solve_host import RESIDUAL_K, dispatch_rule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND = {LC.WELL1: 1e1, LC.WELL4: 1e4}


@pytest.fixture(scope="module")
def kernel_names():
    """gl_lstsq_last_kernels (mangled) -> the matrix's spelling"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_flops as isa
    from gigalens_amd import _native
    cache = {"": ""}

    def names():
        out = []
        for sym in _native.lstsq_last_kernels():
            if sym not in cache:
                cache[sym] = LC.short_name(isa.demangle([sym])[0])
            out.append(cache[sym])
        return tuple(out)
    return names


def _run(case, stack, obs, err):
    """One gl_lstsq_solve_stack call -> (coeffs [B, D], flags [B], normal [B, Dp, Dp]) as numpy, guards checked"""
    from gigalens_amd import _native
    dev = torch.device("cuda")
    B, D, HW, Dp = case.B, case.D, case.HW, case.Dp
    st = torch.from_numpy(stack).to(dev)
    bufs = []
    for a in (obs, err):  # views that start case.offset floats after an aligned address
        flat = torch.zeros(HW + 8, dtype=torch.float32, device=dev)
        assert flat.data_ptr() % 16 == 0
        v = flat[case.offset:case.offset + HW]
        v.copy_(torch.from_numpy(a))
        bufs.append(v)
    nbytes = _native.lstsq_solve_stack_workspace_bytes(B, D, HW, case.wgs)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)  # 0xFFFFFFFF: a NaN in every float
    flat_c = torch.full(((B + 1) * D,), float("nan"), dtype=torch.float32, device=dev)
    flags = torch.full((B,), -1, dtype=torch.int32, device=dev)
    normal = torch.full((B, Dp, Dp), float("nan"), dtype=torch.float32, device=dev)
    _native.lstsq_solve_stack(st, bufs[0], bufs[1], workgroups=case.wgs, cholesky=case.chol, coeffs=flat_c[:B * D].view(B, D),
                              flags=flags, normal=normal, workspace=ws)
    torch.cuda.synchronize()
    c = flat_c.cpu().numpy()
    assert np.isnan(c[B * D:]).all(), "the guard behind the coefficients was written"
    return c[:B * D].reshape(B, D), flags.cpu().numpy(), normal.cpu().numpy()


@pytest.mark.parametrize("case", LC.CASES, ids=[c.id for c in LC.CASES])
def test_lstsq_case(gl, case, kernel_names):
    stack, obs, err = LC.make_inputs(case)
    D, il = case.D, np.tril_indices(case.D + 1)
    co, flags, normal = _run(case, stack, obs, err)
    # (gl_lstsq_last_kernels has three slots: the launch of gl_partial_sum_kernel above eight chunks is not observed by name but
    # through the matrix it leaves.  With 2 .. 8 chunks the matrix read back is a re-sum of the partials after the solve, by the
    # additions the solve kernels made and in their order -- bitwise the values they consumed, not a copy of them.)
    seen = kernel_names()
    assert seen == case.kernels, f"launched {seen}, declared {case.kernels}"
    co2, flags2, normal2 = _run(case, stack, obs, err)
    same = lambda a, b: a.tobytes() == b.tobytes()
    assert same(co, co2) and same(flags, flags2), "two runs differ"
    assert all(same(normal[b][il], normal2[b][il]) for b in range(case.B)), "two runs differ in the normal matrix"
    if not case.cholk:
        assert np.all(flags == 1)
    fig = {"normal": 0.0, "residual": 0.0, "forward": 0.0, "proj": 0.0, "null": 0.0}
    for b in range(case.B):
        recipe = case.recipe(b)
        if recipe == LC.NAN:
            assert np.isnan(co[b]).all(), "a non-finite sample must come out all NaN"
            continue
        assert np.isfinite(co[b]).all(), b
        # ---- the normal matrix, element by element (rows 0 .. D, columns 0 .. row)
        M, absM = LC.augmented_reference(stack[b], obs, err)
        got = normal[b].astype(np.float64)[:D + 1, :D + 1]
        assert np.isfinite(got[il]).all(), (b, "an element of the lower triangle was not written")
        bound = LC.normal_bound(case, absM)
        over = np.abs(got - M)[il] > bound[il]
        fig["normal"] = max(fig["normal"], float((np.abs(got - M)[il] / np.maximum(bound[il], 1e-300)).max()))
        assert not over.any(), (b, "normal matrix outside the bound at", [(int(i), int(j)) for i, j in zip(il[0][over], il[1][over])][:8],
                                fig["normal"])
        if recipe == LC.EMPTY:
            assert not co[b].any() and same(co[b], np.zeros(D, np.float32)), "an empty system has coefficients exactly 0"
            continue
        A64, r64, c64 = LC.reference(stack[b], obs, err)
        w = np.linalg.eigvalsh(A64)
        if case.cholk:  # the flags where float64 decides them
            if w.min() > 16 * LC.RCOND * np.linalg.norm(A64):
                assert flags[b] == 0, (b, "the Cholesky attempt must solve this system")
            if w.min() < LC.RCOND * w.max():
                assert flags[b] == 1, (b, "the Cholesky attempt must refuse this system")
        X, _ = LC.weighted(stack[b], obs, err)
        c = co[b].astype(np.float64)
        if recipe in LC.WELL:
            # the GPU's own matrix A^ (lower triangle mirrored) and right-hand side (row D)
            Ah = np.tril(got[:D, :D]) + np.tril(got[:D, :D], -1).T
            rh = got[D, :D]
            res = np.abs(Ah @ c - rh).max() / (np.abs(Ah).sum(1).max() * np.abs(c).max())
            want = np.linalg.pinv(Ah, rcond=LC.RCOND, hermitian=True) @ rh
            fwd = np.abs(c - want).max() / np.abs(want).max()
            fig["residual"] = max(fig["residual"], float(res))
            fig["forward"] = max(fig["forward"], float(fwd / (30 * COND[recipe] * 6e-8 + 1e-6)))
            assert res <= RESIDUAL_K, (b, res)
            assert fwd <= 30 * COND[recipe] * 6e-8 + 1e-6, (b, fwd)
        else:  # rank deficient: the minimum-norm solution
            if case.cholk:
                assert flags[b] == 1, b
            proj = np.abs(X @ c - X @ c64).max() / np.abs(X @ c64).max()
            fig["proj"] = max(fig["proj"], float(proj))
            assert proj <= 2e-4, (b, proj)
            # the null directions (the zero column, each duplicate pair): |n . c| under the derived bound of LC.null_bound, which
            # the host twin meets on the same matrices (test_lstsq_solve_host), and test_eigh_host's form for the pairs
            for nv in LC.null_vectors(case, b):
                ratio = abs(nv @ c) / (LC.null_bound(w) * np.abs(c).max())
                fig["null"] = max(fig["null"], float(ratio))
                assert ratio <= 1.0, (b, "a null direction of the system carries", float(nv @ c), "bound ratio", ratio)
            for d, o in LC.gap_layout(case, b)[0]:
                assert abs(c[d] - c[o]) <= 1e-4 * abs(c[o]), (b, d, o, c[d], c[o])
    print(f"{case.id}: normal {fig['normal']:.3g} of the bound (m = {LC.rounding_count(case)}), residual {fig['residual'] / LC.U:.3g} u "
          f"(K = {RESIDUAL_K / LC.U:.0f} u), forward {fig['forward']:.3g} of its tolerance, projection {fig['proj']:.3g}, "
          f"null directions {fig['null']:.3g} of their bound")
    if LC.NAN in case.recipes:  # the neighbours of the NaN sample are bitwise what they are without the NaN (same B: same chunks)
        st2, obs2, err2 = LC.make_inputs(case, nan=False)
        assert same(obs, obs2) and same(err, err2)
        clean, _, _ = _run(case, st2, obs2, err2)
        assert np.isfinite(clean).all()
        for b in range(case.B):
            if case.recipe(b) != LC.NAN:
                assert same(co[b], clean[b]), (b, "a NaN in another sample changed this one")


@pytest.mark.parametrize("kind,num_pix,lens_light", [("sersic", 32, True), ("shapelets4", 36, True), ("shapelets11", 40, True),
                                                      ("shapelets16", 48, True), ("shapelets4", 36, False)])
def test_product_call_launches_the_tested_kernels(gl, kernel_names, kind, num_pix, lens_light):
    """lstsq_simulate on a model launches what the dispatch rule of the matrix gives for its (D, HW); the stack-free shapelet path
    (a shapelet source alone) reports its own normal-matrix kernel."""
    from tests.test_gpu_lstsq import _model, _observation
    B = 2
    wl = _model(kind, num_pix, B, lens_light=lens_light, interpolate=False)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=B)
    obs, err = _observation(wl)
    co = sim.lstsq_simulate(wl.prior.sample(B, seed=5), obs, err, return_coeffs=True)
    torch.cuda.synchronize()
    D = co.shape[1]
    assert torch.isfinite(co).all()
    rule, _ = dispatch_rule(LC.C("product", D, num_pix * num_pix, B, 1, "", "", ""))
    seen = kernel_names()
    if lens_light:
        assert seen == rule, (seen, rule)
    else:
        assert seen[0].startswith("gl_shp_normal_kernel<") and seen[1:] == rule[1:], (seen, rule)
