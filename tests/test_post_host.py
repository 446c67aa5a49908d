"""CPU half of the post-processing matrix (tests/post_cases.py): the float64 reference agrees with the oracle's own PSF / pooling
lines and its transpose is the adjoint; the matrix is well formed, covers what it claims and declares the kernels the dispatch
rule of launch_corr gives; the gl_corr_pair_kernel instantiations in the shipped library are exactly the declared ones; and a
float32 emulation of the plain tap order stays inside the derived bound of every case."""
import os
import re
import sys
import zlib
from collections import Counter

import numpy as np
import pytest
import torch

from tests import post_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

IDS = [c.id for c in PC.CASES]


def _geometries():
    """every distinct (psf shape, supersample) of the matrix"""
    return sorted({(c.psf, c.ss) for c in PC.CASES}, key=str)


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("psf_shape,ss", _geometries(), ids=[f"{p}-ss{s}" for p, s in _geometries()])
def test_reference_agrees_with_the_oracle(psf_shape, ss):
    """post_fwd_f64 against the pad -> conv2d -> avg_pool2d lines RefSimulator.simulate runs (oracle.ref_torch.psf_pool), in
    float64 on random inputs: two orders of the same sum of at most kh kw ss^2 terms."""
    from oracle import ref_torch as ref
    r = np.random.default_rng(zlib.crc32(f"{psf_shape}/{ss}".encode()))
    n = 13 if ss == 3 else 14
    S = r.normal(size=(3, n * ss, n * ss))
    psf = None if psf_shape is None else r.uniform(0.1, 1.0, size=psf_shape)
    flat = None if psf is None else torch.from_numpy(psf[::-1, ::-1].copy())
    want = ref.psf_pool(torch.from_numpy(S)[:, None], flat, ss)[:, 0].numpy() * 0.37
    got = PC.post_fwd_f64(S, psf, ss, 0.37)
    assert got.shape == want.shape == (3, n, n)
    terms = (1 if psf is None else psf.size) * ss * ss
    mag = PC.post_fwd_f64(np.abs(S), None if psf is None else np.abs(psf), ss, 0.37)
    assert np.all(np.abs(got - want) <= 2 * (terms + 2) * 2.0 ** -53 * mag)


def test_simulate_uses_psf_pool():
    """RefSimulator.simulate goes through psf_pool: the function the test above compares with is the oracle's own code."""
    import inspect
    from oracle import ref_torch as ref
    src = inspect.getsource(ref.RefSimulator.simulate)
    assert "psf_pool(" in src and "conv2d" not in src and "avg_pool2d" not in src


@pytest.mark.parametrize("case", PC.CASES, ids=IDS)
def test_reference_transpose_is_the_adjoint(case):
    """<post_fwd(S), G> = <S, post_bwd(G)> to float64 rounding, on the case's own geometry"""
    r = np.random.default_rng(7)
    psf = PC.make_psf(case)
    B = min(case.batch, 2)
    S = r.normal(size=(B, case.hs, case.hs))
    G = r.normal(size=(B, case.n, case.n))
    lhs = float((PC.post_fwd_f64(S, psf, case.ss, case.scale) * G).sum())
    rhs = float((S * PC.post_bwd_f64(G, psf, case.ss, case.scale, case.hs, case.hs)).sum())
    apsf = None if psf is None else np.abs(psf)
    mag = float((PC.post_fwd_f64(np.abs(S), apsf, case.ss, abs(case.scale)) * np.abs(G)).sum())
    n_add = S.size + case.kh * case.kw * case.ss ** 2 + 4  # additions behind either inner product, an upper count
    assert abs(lhs - rhs) <= 2 * n_add * 2.0 ** -53 * mag, (lhs, rhs, mag)


# ---- the matrix -------------------------------------------------------------------------------------------------------------
def _pad4(n):
    return max(4, (n + 3) & ~3)


def _tile_width(tc):
    return ((tc + 3 + 3) // 4) * 4


def dispatch_rule(case):
    """launch_corr / post_fwd / post_bwd (csrc/gigalens_hip.hip) restated: the kernels that serve the case's two directions"""
    ss, KH, KW = case.ss, case.KH, case.KW
    if case.env.get("GIGALENS_HIP_CORR_PAIR", "1") == "0" or ss > 2 or KW > 32 or KH > 64:
        return PC.TAP_F, PC.TAP_B
    kwp = _pad4(KW)
    if ss == 1:
        return PC.S1(kwp), PC.S1(kwp)
    wide = kwp <= 28 and KH <= 28 and case.env.get("GIGALENS_HIP_CORR_WIDE", "1") != "0"
    if wide:
        fwd = PC.WIDE(kwp)
    else:  # the input tile: (15 ss + KH) rows of (31 ss + KWP, widened to whole float4 groups, odd) float2 within 64 KB
        lds = (15 * ss + KH) * (_tile_width(31 * ss + kwp) | 1) * 8
        fwd = PC.S2(kwp) if lds <= 64 * 1024 else PC.TAP_F
    # transpose plan (gl_model_create): per column class pj the decimated sub-kernel has Cn taps; the classes' left paddings are
    # levelled to the largest by shifting
    pad_l = (case.kw - 1) // 2
    Cn, pln = [], []
    for pj in range(ss):
        C = (KW - pj + ss - 1) // ss if KW > pj else 0
        rj = (pj - pad_l) % ss
        Cn.append(C)
        pln.append((C - 1) - (rj + pad_l - pj) // ss)
    width = max([1] + [Cn[pj] + max(pln) - pln[pj] for pj in range(ss)])
    return fwd, PC.T2(_pad4(width))


def test_matrix_is_well_formed():
    ids = Counter(IDS)
    assert not [i for i, k in ids.items() if k > 1], ids
    for c in PC.CASES:
        assert set(c.env) <= set(PC.ENV_KNOBS), c.id
        assert c.ss in (1, 2, 3) and (c.psf is not None or c.ss > 1), c.id
        assert 1 <= c.hs <= PC.MAX_SIDE and c.batch >= 1, c.id
        assert c.batch * c.hs * c.hs * c.kh * c.kw <= 2 ** 28, c.id  # keeps the float64 reference to seconds
        assert (c.fwd, c.bwd) == dispatch_rule(c), (c.id, dispatch_rule(c))
        for transpose in (False, True):
            x = PC.impulse_input(c, transpose)
            assert np.all((x != 0).sum(axis=(1, 2)) == 1), c.id
            assert len({float(v) for v in x[x != 0]}) == c.batch, c.id  # amplitudes differ per sample


def test_matrix_covers_the_dispatch():
    """Every boundary the launch code branches on has a case on each side (the issue's list)."""
    by = {c.id: c for c in PC.CASES}
    names = PC.declared_names()
    assert {PC.TAP_F, PC.TAP_B} <= names
    assert {c.batch for c in PC.CASES} >= {1, 2, 3, 15, 16, 17, 33}
    assert {(c.batch + 1) // 2 for c in PC.CASES} >= {8, 9, 17}
    # every KWP of each reachable family
    assert {PC.S1(k) for k in range(4, 33, 4)} <= names
    assert {PC.WIDE(k) for k in range(4, 29, 4)} <= names
    assert {PC.S2(k) for k in range(4, 33, 4)} <= names
    assert {PC.T2(k) for k in range(4, 21, 4)} <= names
    pair = lambda c: PC.pair_args(c.fwd) is not None
    # KW 32 / 33, KH 64 / 65, ss 2 / 3
    assert any(c.KW == 32 and pair(c) for c in PC.CASES) and any(c.KW == 33 and c.KH <= 64 and c.ss <= 2 for c in PC.CASES)
    assert any(c.KH == 64 and pair(c) for c in PC.CASES) and any(c.KH == 65 and c.KW <= 32 and c.ss <= 2 for c in PC.CASES)
    assert any(c.ss == 3 for c in PC.CASES) and any(c.ss == 3 and c.psf is None for c in PC.CASES)
    # the wide rule: KWP 28 / 32 and KH 28 / 29 without the knob
    plain = [c for c in PC.CASES if not c.env and c.ss == 2]
    assert any(c.fwd == PC.WIDE(28) and c.KH == 28 for c in plain)
    assert any(c.fwd == PC.S2(32) and c.KH <= 28 for c in plain) and any(c.fwd == PC.S2(28) and c.KH == 29 for c in plain)
    # the LDS limit at KWP = 32
    assert any(c.fwd == PC.S2(32) and c.KH == 51 for c in plain)
    assert any(c.fwd == PC.TAP_F and c.KH == 52 and c.KW <= 32 and PC.pair_args(c.bwd) for c in plain)
    # 1 x 1, pooling only at ss = 2, rectangular, even and odd sides
    assert any(c.psf == (1, 1) for c in PC.CASES) and any(c.psf is None and c.ss == 2 and c.KW == 2 for c in PC.CASES)
    assert any(c.psf and c.psf[0] != c.psf[1] for c in PC.CASES)
    assert {s % 2 for c in PC.CASES if c.psf for s in c.psf} == {0, 1}
    # image sizes: widths 0..3 mod 4, both values of `vec`, smaller than a tile, whole tiles
    assert {c.n % 4 for c in PC.CASES if pair(c)} == {0, 1, 2, 3}
    vec = lambda c: c.offset == 0 and c.n % 4 == 0 and c.hs % 4 == 0
    assert any(vec(c) and pair(c) for c in PC.CASES) and any(not vec(c) and pair(c) for c in PC.CASES)
    assert any(c.n < 16 and pair(c) for c in PC.CASES) and any(c.n % 32 == 0 and pair(c) for c in PC.CASES)
    assert any(c.n > 32 and c.n % 16 for c in PC.CASES)  # several tiles, the last one partial
    # the scalar path forced by alignment alone
    assert any(c.offset % 4 and c.n % 4 == 0 and c.hs % 4 == 0 and pair(c) for c in PC.CASES)
    # slicing: 1 and 3 pairs a slice on odd batches
    sl = {c.env["GIGALENS_HIP_CORR_MAXPAIRS"]: c for c in PC.CASES if "GIGALENS_HIP_CORR_MAXPAIRS" in c.env}
    assert set(sl) == {"1", "3"} and all(c.batch % 2 == 1 and (c.batch + 1) // 2 > int(k) for k, c in sl.items())
    assert any(c.scale == 1.0 and c.batch >= 12 for c in PC.CASES)  # the basis stack
    assert by["s2_narrow_kwp24"].env == {}  # the narrow family is also reached without its knob


# ---- the library ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library_names():
    import isa_flops as isa
    if not os.path.exists(isa.LIB):
        pytest.skip("library not built")
    return {PC.short_name(k) for k in isa.kernel_metadata(isa.code_object())}


def test_pair_instantiations_equal_the_declared_matrix(library_names):
    shipped = {k for k in library_names if k.startswith("gl_corr_pair_kernel<")}
    declared = {k for k in PC.declared_names() if k.startswith("gl_corr_pair_kernel<")}
    assert shipped - declared == set(), f"instantiations without a case in tests/post_cases.py: {sorted(shipped - declared)}"
    assert declared - shipped == set(), f"declared but not in the library: {sorted(declared - shipped)}"
    assert len(shipped) == 28  # 8 + 7 + 8 + 5: the four that no plan can reach are not built (launch_corr: corr_reachable)


def test_every_declared_name_is_in_the_library(library_names):
    assert not sorted(PC.declared_names() - library_names)


def test_unreachable_instantiations_are_unreachable():
    """The dispatch code itself: `wide` requires KWP <= 28, and the supersample-2 transpose plan is at most 17 taps wide (KW <= 32
    -> ceil(32 / 2) taps a class, one more when the classes' paddings are levelled), so KWP <= 20."""
    src = open(os.path.join(ROOT, "gigalens_amd", "csrc", "gigalens_hip.hip")).read()
    assert re.search(r"const bool wide = pl\.ST == 2 && a\.ncj == 1 && pl\.KWP <= 28 && pl\.max_KH <= 28 && corr_wide;", src)
    assert re.search(r"ss <= 2 && m->KW <= 32 && m->KH <= 64", src)
    widths = set()
    for kw in range(1, 32):  # every PSF width the pair plan accepts at supersample 2
        c = PC.Case("w", (3, kw), 2, 8, 1, "", "")
        widths.add(int(PC.pair_args(dispatch_rule(c)[1])[0]))
    assert max(widths) == 20 and widths == {4, 8, 12, 16, 20}


# ---- the bound --------------------------------------------------------------------------------------------------------------
def _emulate_f32(case, x, transpose, psf):
    """The plain tap order in float32: one fused multiply-add per tap of the float32 effective kernel, then x scale"""
    ss, KH, KW = case.ss, case.KH, case.KW
    pt, pl = (case.kh - 1) // 2, (case.kw - 1) // 2
    keff = np.zeros((KH, KW))
    k = np.ones((1, 1)) if psf is None else np.asarray(psf, dtype=np.float64)[::-1, ::-1]
    for a in range(ss):
        for b in range(ss):
            keff[a:a + case.kh, b:b + case.kw] += k / (ss * ss)
    keff = keff.astype(np.float32).astype(np.float64)
    B, n, hs = case.batch, case.n, case.hs
    fma = lambda acc, prod: (acc.astype(np.float64) + prod).astype(np.float32)  # products of two float32 are exact in float64
    x = np.asarray(x, dtype=np.float64)
    if not transpose:  # out[I, J] = sum_uv S[I ss + u - pt, J ss + v - pl] Keff[u, v]
        xp = np.pad(x, ((0, 0), (pt, KH), (pl, KW)))
        acc = np.zeros((B, n, n), dtype=np.float32)
        for u in range(KH):
            for v in range(KW):
                acc = fma(acc, xp[:, u:u + n * ss:ss, v:v + n * ss:ss] * keff[u, v])
    else:  # gS[i, j] = sum_IJ gP[I, J] Keff[i + pt - I ss, j + pl - J ss]
        accp = np.zeros((B, hs + KH + ss, hs + KW + ss), dtype=np.float32)
        for u in range(KH):
            for v in range(KW):
                sl = accp[:, u:u + n * ss:ss, v:v + n * ss:ss]
                accp[:, u:u + n * ss:ss, v:v + n * ss:ss] = fma(sl, x * keff[u, v])
        acc = accp[:, pt:pt + hs, pl:pl + hs]
    return (acc * np.float32(case.scale)).astype(np.float32)


@pytest.mark.parametrize("case", PC.CASES, ids=IDS)
def test_float32_tap_order_stays_inside_the_bound(case):
    """The derived bound is loose enough for a correct float32 kernel (and the reference and its adjoint place every tap where
    the kernels' formula does): a numpy emulation of the tap-by-tap order, both directions, random and impulse inputs."""
    psf = PC.make_psf(case)
    for transpose in (False, True):
        tap = PC.TAP_B if transpose else PC.TAP_F  # the emulation is the tap kernels' count of multiply-adds: the smallest n
        x = PC.random_input(case, transpose)
        ref = PC.post_f64(case, x, transpose, psf)
        bound = PC.error_bound(case, x, transpose, psf, kernel=tap)
        err = np.abs(_emulate_f32(case, x, transpose, psf).astype(np.float64) - ref)
        assert np.all(err <= bound), (transpose, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(bound <= PC.error_bound(case, x, transpose, psf))  # the declared kernel's n is no smaller
        xi = PC.impulse_input(case, transpose)
        emu = _emulate_f32(case, xi, transpose, psf).astype(np.float64)
        worst, stray = PC.impulse_error_in_u(case, xi, emu, transpose, psf)
        assert stray == 0 and worst <= 2.0 + PC.U, (transpose, worst, stray)
