"""CPU half of the linear-solve matrix (tests/lstsq_cases.py): the float64 reference agrees with the oracle's own lines; the matrix
is well formed, covers what it claims and declares the kernels an independent restatement of gl_lstsq_fwd's dispatch ladder and of
the chunk arithmetic gives; the instantiations of the solve's kernel templates in the shipped library are exactly the declared
ones; the inputs meet the conditions the GPU assertions rest on (no eigenvalue near the cut, the host twin of the eigen solver
makes numpy's cut); and a float32 emulation of the plain accumulation order stays inside the derived bound of every case."""
import functools
import inspect
import math
import os
import sys
from collections import Counter
from ctypes import POINTER, c_float, c_int

import numpy as np
import pytest
import torch

from tests import lstsq_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

IDS = [c.id for c in LC.CASES]
RESIDUAL_K = 64 * LC.U  # |A c - r| <= K ||A||_inf ||c||_inf (the form of tests/test_eigh_host.py): 10 x the host twin's worst, 6.1 u
HOST_MAXN = 79      # what tests/hostmath serves (gle::EIG_MAXN - 1)


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    case = next(c for c in LC.CASES if c.id == case_id)
    return LC.make_inputs(case)


def samples(case, recipes=None):
    for b in range(case.B):
        if recipes is None or case.recipe(b) in recipes:
            yield b


# ---- the reference ----------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle():
    """LC.reference against the lines oracle.ref_torch.lstsq_simulate runs after its stack is rendered, in float64 on one small
    stack: the same quantities in another order of summation."""
    from oracle import ref_torch as ref
    src = inspect.getsource(ref.lstsq_simulate)
    for line in ("W = 1 / err", "Y = (obs * W).reshape(1, -1, 1)", "X = (ret * W).reshape(sim.bs, depth, -1).permute(0, 2, 1)",
                 "coeffs = (torch.linalg.pinv(Xt @ X, rcond=1e-6) @ Xt @ Y)[..., 0]"):
        assert line in src, line
    r = np.random.default_rng(5)
    bs, depth, H, Wd = 3, 6, 9, 7
    ret = torch.from_numpy(r.normal(size=(bs, depth, H, Wd)).astype(np.float32)).double()
    ret[1, 4] = ret[1, 1]  # a duplicate: the cut is in play
    err = torch.from_numpy(r.uniform(0.5, 2.0, size=(H, Wd)).astype(np.float32)).double()
    obs = torch.from_numpy(r.normal(size=(H, Wd)).astype(np.float32)).double()
    W = 1 / err
    Y = (obs * W).reshape(1, -1, 1)
    X = (ret * W).reshape(bs, depth, -1).permute(0, 2, 1)
    Xt = X.permute(0, 2, 1)
    coeffs = (torch.linalg.pinv(Xt @ X, rcond=1e-6) @ Xt @ Y)[..., 0].numpy()
    for b in range(bs):
        A, rr, c = LC.reference(ret[b].numpy().reshape(depth, -1).astype(np.float32), obs.numpy().ravel().astype(np.float32),
                                err.numpy().ravel().astype(np.float32))
        assert np.allclose(A, (Xt @ X)[b].numpy(), rtol=1e-13, atol=1e-13 * np.abs(A).max())
        assert np.abs(c - coeffs[b]).max() <= 1e-9 * np.abs(coeffs[b]).max()
    assert abs(coeffs[1, 4] - coeffs[1, 1]) <= 1e-9 * abs(coeffs[1, 1])


# ---- the matrix -------------------------------------------------------------------------------------------------------------
def carve_rule(HW, B, wgs):
    """carve_lstsq's chunk arithmetic restated: per-sample chunk target, pixels per chunk in whole 64-pixel groups"""
    target = max(1, math.ceil(wgs / B))
    px = math.ceil(HW / target)
    px = max(64, 64 * math.ceil(px / 64))
    return px, math.ceil(HW / px)


def dispatch_rule(case):
    """The ladder of the solve (csrc/gl_api_lstsq.hip) restated: (normal, Cholesky, eigen, partial sum?)"""
    C = case.D + 1
    vec = case.HW % 4 == 0 and case.offset % 4 == 0
    tf = "true" if vec else "false"
    if C <= 8:
        normal = "gl_normal_small_kernel<8>"
    elif C > 80:
        normal = f"gl_normal_pair_kernel<{tf}>"
    else:
        normal = f"gl_normal_mfma_kernel<{math.ceil(C / 16)}, {tf}>"
    chol = ""
    if case.D <= 127 and case.chol:
        chol = f"gl_chol_solve_kernel<{4 if C <= 64 else 5 if C <= 80 else 8}>"
    eigen = "gl_eigh_solve_kernel<2, false>" if case.D <= 127 else "gl_eigh_solve_kernel<4, true>"
    return (normal, chol, eigen), carve_rule(case.HW, case.B, case.wgs)[1] > 8


def test_matrix_is_well_formed():
    ids = Counter(IDS)
    assert not [i for i, k in ids.items() if k > 1], ids
    for c in LC.CASES:
        assert 1 <= c.D <= LC.LS_MAXN and 100 <= c.HW <= 2048 and c.B >= 1, c.id
        assert len(c.recipes) in (1, c.B), c.id
        assert (c.chunk, c.n_chunks) == carve_rule(c.HW, c.B, c.wgs), c.id
        names, psum = dispatch_rule(c)
        assert c.kernels == names, (c.id, names)
        assert psum == (c.n_chunks > 8), c.id
        live = int((~LC.mask_of(c)).sum())
        assert live >= 2 * c.D + 2, c.id  # the least-squares problem is overdetermined on the unmasked pixels
        stack, obs, err = inputs(c.id)
        assert stack.dtype == obs.dtype == err.dtype == np.float32 and stack.shape == (c.B, c.D, c.HW), c.id
        assert np.isinf(err).sum() == c.HW - live and np.all(err > 0), c.id
        for b in samples(c):
            if c.recipe(b) == LC.EMPTY:
                assert not stack[b].any(), c.id
            assert np.isnan(stack[b]).sum() == (c.recipe(b) == LC.NAN), c.id
            dups, zeros = LC.gap_layout(c, b)
            assert bool(dups or zeros) == (c.recipe(b) in LC.RANK_DEFICIENT), c.id
            for d, o in dups:
                assert stack[b, d].tobytes() == stack[b, o].tobytes() and stack[b, d].any(), c.id
            for z in zeros:
                assert not stack[b, z].any(), c.id
    assert sum(c.B > 5 for c in LC.CASES) == 1


def test_matrix_covers_the_ladder():
    """Every instantiation, both sides of every edge of the issue's list, every pixel-count class, every batch size."""
    names = LC.declared_names()
    every = {LC.SMALL, LC.PSUM, LC.E2, LC.E4, LC.PAIR(True), LC.PAIR(False), LC.CH(4), LC.CH(5), LC.CH(8)}
    every |= {LC.MFMA(nt, v) for nt in range(1, 6) for v in (True, False)}
    assert names == every and len(every) == 19
    Ds = {c.D for c in LC.CASES}
    # D + 1 = 8 | 9, 16 | 17, 32 | 33, 48 | 49, 64 | 65, 80 | 81, 128 | 129, 192 | 193;  D = 127 | 128;  D = 255 (256 is refused: GPU)
    assert Ds >= {7, 8, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 127, 128, 191, 192, 255}
    well = lambda c: any(c.recipe(b) in LC.WELL for b in samples(c))
    assert {c.cholk for c in LC.CASES if c.D in (63, 64, 79, 80) and well(c)} == {LC.CH(4), LC.CH(5), LC.CH(8)}
    assert {c.n_chunks for c in LC.CASES} >= {1, 8, 9}
    for nc in (8, 9):  # both summation routes with and without the Cholesky attempt's reader
        assert any(c.n_chunks == nc and c.cholk for c in LC.CASES), nc
    assert any(c.n_chunks == 9 and c.normal == LC.SMALL for c in LC.CASES) and any(c.n_chunks == 9 and c.eigen == LC.E4 for c in LC.CASES)
    assert {c.HW % 64 for c in LC.CASES} >= {0, 1, 15, 16, 17}
    assert any(c.HW % 4 and c.normal.startswith("gl_normal_mfma") for c in LC.CASES) and any(c.HW % 4 and c.normal.startswith("gl_normal_pair") for c in LC.CASES)
    assert any(c.HW < 256 and c.normal == LC.SMALL for c in LC.CASES)
    assert any(c.HW < c.chunk for c in LC.CASES)
    for fam in ("gl_normal_mfma", "gl_normal_pair"):
        assert any(c.offset % 4 and c.HW % 4 == 0 and c.normal.startswith(fam) for c in LC.CASES), fam
    assert {c.B for c in LC.CASES} >= {1, 2, 3, 33}
    # the wave context of the eigen solve on its eigenvector path: a rank-deficient sample at every listed n
    ql = {c.D: c.eigen for c in LC.CASES if any(c.recipe(b) in LC.RANK_DEFICIENT for b in samples(c))}
    assert {n: ql.get(n) for n in (63, 64, 65, 127)} == {n: LC.E2 for n in (63, 64, 65, 127)}
    assert {n: ql.get(n) for n in (128, 129, 192, 193, 255)} == {n: LC.E4 for n in (128, 129, 192, 193, 255)}
    # recipes: both conditions, gap, masked, mixed, NaN between two finite samples, Cholesky off on both eigen kernels' sizes
    rec = Counter(c.recipe(b) for c in LC.CASES for b in samples(c))
    assert all(rec[k] for k in (LC.WELL1, LC.WELL4, LC.GAP, LC.ZERO_FIRST, LC.EMPTY, LC.NAN))
    assert any(c.masked and c.normal == LC.SMALL for c in LC.CASES) and any(c.masked and "mfma" in c.normal for c in LC.CASES)
    assert any(c.masked and "pair" in c.normal for c in LC.CASES)
    assert any({LC.WELL1, LC.GAP, LC.EMPTY} <= {c.recipe(b) for b in samples(c)} for c in LC.CASES)
    assert any(c.B == 3 and len(c.recipes) == 3 and c.recipes[1] == LC.NAN and LC.NAN not in (c.recipes[0], c.recipes[2]) for c in LC.CASES)
    assert any(not c.chol and c.D <= 127 for c in LC.CASES)
    # the duplicate recipe stays where the host twin can confirm its cut; beyond, the zero-first recipe (ZERO_FIRST)
    assert all(c.D <= HOST_MAXN for c in LC.CASES for b in samples(c, (LC.GAP,)))
    assert all(any(c.recipe(b) == LC.GAP for b in samples(c)) for c in LC.CASES if c.D in (63, 64, 65))
    for c in LC.CASES:  # generic positions: neither the first nor the last column only by chance, and distinct
        for b in samples(c, (LC.GAP,)):
            dups, zeros = LC.gap_layout(c, b)
            idx = [i for p in dups for i in p] + zeros
            assert len(set(idx)) == len(idx) and all(0 <= i < c.D for i in idx), c.id


# ---- the library ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library_names():
    import isa_flops as isa
    if not os.path.exists(isa.LIB):
        pytest.skip("library not built")
    return {LC.short_name(k) for k in isa.kernel_metadata(isa.code_object())}


def test_instantiations_equal_the_declared_matrix(library_names):
    shipped = {k for k in library_names if k.split("<")[0] in LC.FAMILIES}
    declared = LC.declared_names()
    assert shipped - declared == set(), f"instantiations without a case in tests/lstsq_cases.py: {sorted(shipped - declared)}"
    assert declared - shipped == set(), f"declared but not in the library: {sorted(declared - shipped)}"
    assert len(shipped) == 19


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spectrum(case_id, b):
    case = next(c for c in LC.CASES if c.id == case_id)
    stack, obs, err = inputs(case_id)
    A, r, c = LC.reference(stack[b], obs, err)
    return A, r, c, np.linalg.eigvalsh(A)


@pytest.mark.parametrize("case", LC.CASES, ids=IDS)
def test_no_eigenvalue_near_the_cut(case):
    """The float64 spectrum of the float32 inputs keeps a factor 30 clear of rcond lambda_max on both sides; well-posed samples
    satisfy the condition under which the Cholesky flag is asserted 0, rank-deficient ones that for 1, and at most one sample of
    a case lies between."""
    between = 0
    for b in samples(case):
        if case.recipe(b) in (LC.EMPTY, LC.NAN):
            continue
        A, _, _, w = spectrum(case.id, b)
        lmax = w.max()
        near = (np.abs(w) > LC.RCOND * lmax / 30) & (np.abs(w) < LC.RCOND * lmax * 30)
        assert not near.any(), (b, w[near] / lmax)
        cut = int((np.abs(w) <= LC.RCOND * lmax).sum())
        dups, zeros = LC.gap_layout(case, b)
        assert cut == len(dups) + len(zeros), (b, cut)
        must0 = w.min() > 16 * LC.RCOND * np.linalg.norm(A)
        must1 = w.min() < LC.RCOND * lmax
        assert must0 == (case.recipe(b) in LC.WELL) or not (must0 or must1), b
        between += not (must0 or must1)
    assert between <= 1


def _fp(a):
    return a.ctypes.data_as(POINTER(c_float))


def _host_solve(hostmath, A64, r64, shortcut):
    n = A64.shape[0]
    A32 = np.ascontiguousarray(A64, dtype=np.float32)
    r32 = np.ascontiguousarray(r64, dtype=np.float32)
    co, ev = np.zeros(n, np.float32), np.zeros(n, np.float32)
    took = hostmath.hm_eigh_pinv_f32(_fp(A32), c_int(n), _fp(r32), c_float(LC.RCOND), c_int(int(shortcut)), _fp(co), _fp(ev))
    return co, ev, took, A32, r32


def test_host_twin_makes_the_same_cut_on_gap_systems(hostmath):
    """gle::pinv_solve in float32 (serial context) on the float64-accumulated, float32-rounded matrix of every rank-deficient
    sample the harness serves: refuses the short cut, cuts as many eigenvalues as numpy, lands on numpy's solution."""
    seen, worst_null = 0, 0.0
    for case in LC.CASES:
        for b in samples(case, LC.RANK_DEFICIENT):
            if case.D > HOST_MAXN:
                continue
            A, r, c64, w = spectrum(case.id, b)
            co, ev, took, A32, r32 = _host_solve(hostmath, A, r, shortcut=True)
            assert took == 0, case.id
            assert int((np.abs(ev) <= LC.RCOND * np.abs(ev).max()).sum()) == int((np.abs(w) <= LC.RCOND * w.max()).sum()), case.id
            assert np.abs(co - c64).max() <= 2e-4 * np.abs(c64).max(), case.id
            # the null directions, held as on the GPU: the derived bound (LC.null_bound) for the zero column and for each duplicate
            # pair, and test_eigh_host's own form for the pair (the recipe makes the shared amplitude comparable to max |c|)
            for nv in LC.null_vectors(case, b):
                ratio = abs(nv @ co.astype(np.float64)) / (LC.null_bound(w) * np.abs(co).max())
                worst_null = max(worst_null, ratio)
                assert ratio <= 1.0, (case.id, b, ratio)
            for d, o in LC.gap_layout(case, b)[0]:
                assert abs(c64[o]) >= 0.4 * np.abs(c64).max(), (case.id, b, "the duplicated column must carry a large amplitude")
                assert abs(co[d] - co[o]) <= 1e-4 * abs(co[o]), (case.id, b, d, o)
            seen += 1
    print(f"host twin: worst |n . c| = {worst_null:.3g} of the null bound")
    assert seen >= 6


def test_host_twin_residual_leaves_a_margin(hostmath):
    """The constant of the GPU's residual check: the host twin's worst |A c - r| / (||A||_inf ||c||_inf) over the well-posed samples
    it serves, both paths, is at least eight times under RESIDUAL_K (measured: 6.1 u)."""
    worst = 0.0
    for case in LC.CASES:
        for b in samples(case, LC.WELL):
            if case.D > HOST_MAXN:
                continue
            A, r, _, _ = spectrum(case.id, b)
            for shortcut in (True, False):
                co, _, _, A32, r32 = _host_solve(hostmath, A, r, shortcut)
                A64 = A32.astype(np.float64)
                res = np.abs(A64 @ co.astype(np.float64) - r32).max() / (np.abs(A64).sum(1).max() * np.abs(co).max())
                worst = max(worst, res)
    print(f"host twin: worst residual ratio {worst:.3g} ({worst / LC.U:.1f} u), K = {RESIDUAL_K / LC.U:.0f} u")
    assert 0 < worst <= RESIDUAL_K / 8


# ---- the bound --------------------------------------------------------------------------------------------------------------
def emulate_normal_f32(stack_b, obs, err):
    """The plain order in float32: w = 1 / err (IEEE division), x = s w, every product rounded, added pixel after pixel"""
    w = (np.float32(1.0) / err).astype(np.float32)
    Z = np.concatenate([stack_b * w, (obs * w)[None]], axis=0).astype(np.float32)  # [D + 1, HW]
    n = Z.shape[0]
    M = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        M[i, :i + 1] = np.cumsum(Z[:i + 1] * Z[i], axis=1, dtype=np.float32)[:, -1]
    return M


@pytest.mark.parametrize("case", LC.CASES, ids=IDS)
def test_float32_plain_order_stays_inside_the_bound(case):
    stack, obs, err = inputs(case.id)
    # (the first three eligible samples of a case: every recipe of every case but the B = 33 one, whose samples repeat recipes)
    for b in list(samples(case, LC.WELL + LC.RANK_DEFICIENT))[:3]:
        M, absM = LC.augmented_reference(stack[b], obs, err)
        got = emulate_normal_f32(stack[b], obs, err).astype(np.float64)
        il = np.tril_indices(case.D + 1)
        ratio = np.abs(got - M)[il] / np.maximum(LC.normal_bound(case, absM)[il], 1e-300)
        assert ratio.max() <= 1.0, (b, float(ratio.max()))
