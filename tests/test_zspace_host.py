"""CPU half of the z-space matrix (tests/zspace_cases.py): the float64 restatement is held to scipy.stats and
torch.distributions.transforms, its derivatives to float64 autograd, gigalens_amd/prior.py to it at prior-typical draws; the matrix
names every (bijector, prior) pair and every front-end variant; the inputs of every case meet the conditions the GPU tests
(tests/test_gpu_zspace.py) rely on."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import zspace_cases as Z

SPECS = [Z.Spec(Z.ID, Z.NORMAL, 0.3, 0.7), Z.Spec(Z.ID, Z.LOGNORMAL, -0.2, 0.6), Z.Spec(Z.ID, Z.UNIFORM, 0, 1, -5.0, 4.0),
         Z.Spec(Z.ID, Z.TRUNC, 0.5, 1.2, -5.0, 4.0),
         Z.Spec(Z.EXP, Z.NORMAL, 1.0, 2.0), Z.Spec(Z.EXP, Z.LOGNORMAL, 0.1, 0.4), Z.Spec(Z.EXP, Z.UNIFORM, 0, 1, 0.01, 60.0),
         Z.Spec(Z.EXP, Z.TRUNC, 2.0, 3.0, 0.01, 60.0),
         Z.Spec(Z.SIG, Z.NORMAL, -0.3, 0.2, *Z.SIG_A), Z.Spec(Z.SIG, Z.LOGNORMAL, 0.7, 0.2, *Z.SIG_B),
         Z.Spec(Z.SIG, Z.UNIFORM, 0, 1, *Z.SIG_A), Z.Spec(Z.SIG, Z.TRUNC, 2.0, 0.25, *Z.SIG_B), Z.Spec(Z.SIG, Z.TRUNC, -0.3, 0.2, *Z.SIG_A)]
Z_MODERATE = np.asarray([-3.5, -2.0, -1.0, -1e-3, 0.0, 1e-3, 0.4, 1.0, 2.0, 3.5], dtype=np.float32)


def _z_for(s):
    return np.abs(Z_MODERATE) + np.float32(0.01) if (s.bij == Z.ID and s.prior == Z.LOGNORMAL) else Z_MODERATE


def _torch_forward(s, z):
    """x(z) and log|dx/dz| by torch.distributions.transforms, float64."""
    from torch.distributions import transforms as T
    t = {Z.ID: T.identity_transform, Z.EXP: T.ExpTransform(),
         Z.SIG: T.ComposeTransform([T.SigmoidTransform(), T.AffineTransform(s.lo, s.hi - s.lo)])}[s.bij]
    x = t(z)
    return x, t.log_abs_det_jacobian(z, x) + torch.zeros_like(z)


def _torch_logp(s, x):
    from torch import distributions as D
    a, b, lo, hi = (torch.tensor(v, dtype=torch.float64) for v in (s.a, s.b, s.lo, s.hi))
    if s.prior == Z.NORMAL:
        return D.Normal(a, b).log_prob(x)
    if s.prior == Z.LOGNORMAL:
        return D.LogNormal(a, b).log_prob(x)
    if s.prior == Z.UNIFORM:
        return D.Uniform(lo, hi).log_prob(x)
    return D.Normal(a, b).log_prob(x) - Z.log_norm(s)  # the derivative of a TruncatedNormal inside its support is the Normal's


@pytest.mark.parametrize("s", SPECS, ids=lambda s: "-".join(s.pair))
def test_reference_matches_scipy_and_torch_transforms(s):
    from scipy import stats
    z = _z_for(s)
    ev = Z.eval_column(s, z)
    x_t, ldj_t = _torch_forward(s, torch.from_numpy(z).double())
    assert np.allclose(ev["x"], x_t.numpy(), rtol=1e-13, atol=1e-15)
    assert np.allclose(ev["fldj"], ldj_t.numpy(), rtol=1e-12, atol=1e-13)
    x = ev["x"]
    want = {Z.NORMAL: lambda: stats.norm.logpdf(x, s.a, s.b),
            Z.LOGNORMAL: lambda: stats.lognorm.logpdf(x, s=s.b, scale=math.exp(s.a)),
            Z.UNIFORM: lambda: stats.uniform.logpdf(x, s.lo, s.hi - s.lo),
            Z.TRUNC: lambda: stats.truncnorm.logpdf(x, (s.lo - s.a) / s.b, (s.hi - s.a) / s.b, loc=s.a, scale=s.b)}[s.prior]()
    assert np.all(np.isfinite(want))
    assert np.allclose(ev["logp"], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("s", SPECS, ids=lambda s: "-".join(s.pair))
def test_reference_derivatives_match_float64_autograd(s):
    z = torch.from_numpy(_z_for(s)).double().requires_grad_(True)
    x, ldj = _torch_forward(s, z)
    def grad(y, v):  # a constant (Identity's log|J|, Uniform's density) has no graph: its derivative is 0
        return torch.autograd.grad(y.sum(), v, retain_graph=True)[0] if y.requires_grad else None
    dxdz, dfldj = grad(x, z), grad(ldj, z)
    xl = x.detach().clone().requires_grad_(True)
    dlogp = grad(_torch_logp(s, xl), xl)
    ev = Z.eval_column(s, z.detach().numpy().astype(np.float32))
    zero = torch.zeros_like(z)
    assert np.allclose(ev["dxdz"], (dxdz if dxdz is not None else zero).numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(ev["dfldj"], (dfldj if dfldj is not None else zero).numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(ev["dlogp"], (dlogp if dlogp is not None else zero).numpy(), rtol=1e-12, atol=1e-13)


def test_stable_forms_where_the_plain_ones_cancel():
    """|z| up to 80: dx/dz against the closed form w e / (1 + e)^2 in float64 and the float32 restatement against that -- it stays
    at a few units of roundoff where the plain float32 product sg (1 - sg) has lost its digits (1e-3 at |z| = 10, 0.17 at 15);
    x stays inside [lo, hi] and every term finite in both formats."""
    s = Z.Spec(Z.SIG, Z.UNIFORM, 0, 1, *Z.SIG_A)
    z = np.asarray([v * sgn for v in (1e-3, 1, 4, 8, 10, 12, 15, 17, 20, 40, 80) for sgn in (1, -1)], dtype=np.float32)
    ref, f32 = Z.eval_column(s, z), Z.eval_column(s, z, Z.F32)
    w = s.hi - s.lo
    exact = w * np.exp(-np.abs(z.astype(np.float64))) / (1 + np.exp(-np.abs(z.astype(np.float64)))) ** 2
    assert np.allclose(ref["dxdz"], exact, rtol=1e-14, atol=0)
    assert np.all(np.abs(f32["dxdz"] - ref["dxdz"]) <= 8 * Z.U * ref["dxdz"])
    sg = np.float32(1) / (np.float32(1) + np.exp(-z))
    plain = np.float32(w) * sg * (np.float32(1) - sg)
    err = np.abs(plain - ref["dxdz"]) / ref["dxdz"]
    assert err[np.abs(z) == 10].max() > 1e-4 and err[np.abs(z) == 15].max() > 1e-2  # what the kernels used to compute
    assert np.all((ref["x"] >= s.lo) & (ref["x"] <= s.hi)) and np.all((f32["x"] >= np.float32(s.lo)) & (f32["x"] <= np.float32(s.hi)))
    assert np.all(np.isfinite(ref["t"])) and np.all(np.isfinite(f32["t"]))
    assert np.allclose(ref["dfldj"], 1 - 2 / (1 + np.exp(-z.astype(np.float64))), rtol=0, atol=1e-15)


def test_prior_module_matches_the_reference_at_typical_draws():
    """gigalens_amd/prior.py (float32 torch) against the float64 restatement: forward, log|J| and log-density per column."""
    from gigalens_amd import prior as tfd
    leaves, specs = [], []
    for s in SPECS:
        if (s.bij, s.prior) not in ((Z.ID, Z.NORMAL), (Z.EXP, Z.LOGNORMAL), (Z.SIG, Z.UNIFORM), (Z.SIG, Z.TRUNC)):
            continue  # the pairs a Python class produces
        leaves.append({Z.NORMAL: lambda: tfd.Normal(s.a, s.b), Z.LOGNORMAL: lambda: tfd.LogNormal(s.a, s.b),
                       Z.UNIFORM: lambda: tfd.Uniform(s.lo, s.hi), Z.TRUNC: lambda: tfd.TruncatedNormal(s.a, s.b, s.lo, s.hi)}[s.prior]())
        specs.append(s)
    flat = tfd.FlatPrior(leaves)
    assert flat.bij.tolist() == [s.bij for s in specs] and flat.kind.tolist() == [s.prior for s in specs]
    assert np.allclose(flat.logz.numpy(), [Z.log_norm(s) for s in specs], rtol=1e-6, atol=1e-7)
    x = flat.sample(64, seed=5)
    z = flat.inverse(x)
    ev = Z.evaluate(specs, z.numpy())
    assert np.allclose(flat.forward(z).numpy(), ev["x"], rtol=2e-6, atol=2e-7)
    assert np.allclose(flat.fldj_columns(z).numpy(), ev["fldj"], rtol=2e-6, atol=2e-6)
    assert np.allclose(flat.log_prob_columns(flat.forward(z)).numpy(), ev["logp"], rtol=1e-5, atol=1e-5)


def test_epl_table_reference_forms_agree():
    """The table from the definition (float64) against the recurrence (float32) and, where a factor vanishes, the division-free
    sums against the limit of the definition."""
    for e1, e2, g, cap in ((0.3, 0.2, 2.0, 50), (0.6, -0.5, 1.7, 300), (0.0, 0.0, 2.0, 50), (0.3, -0.4, 1.0, 50)):
        f, s, _, K = Z.epl_head(e1, e2, g, cap)
        ref, rec = Z.epl_table_ref(f, s, K), Z.epl_table_f32(f, s, K)
        assert ref.shape == rec.shape == (K + 4, 4) and not ref[K + 1:].any() and not rec[K + 1:].any()
        err = Z.table_row_errors(rec, ref)
        assert np.all(err <= 8 * (np.arange(K + 4) + 2) * Z.U), (e1, e2, g, err.max())
    f, s, _, K = Z.epl_head(0.3, -0.4, 1.0, 50)
    near = Z.epl_table_ref(f, s - 1e-9, K)  # gamma -> 1: the definition's quotient form converges to the division-free sum
    assert np.allclose(Z.epl_table_ref(f, s, K)[:, 3], near[:, 3], rtol=1e-6, atol=1e-12)


# ---- the matrix ------------------------------------------------------------------------------------------------------
def test_matrix_names_every_pair_and_every_front_end_variant():
    ids = [c.id for c in Z.CASES]
    assert len(set(ids)) == len(ids)
    all_pairs = {(b, p) for b in Z.BIJECTORS for p in Z.PRIORS}
    assert len(all_pairs) == 12
    for cid in ("isolated-basic", "isolated-full"):
        built = Z.reference(cid)[0]
        assert {s.pair for s in built.specs} == all_pairs, cid
        ranges = {(s.lo, s.hi) for s in built.specs if s.bij == Z.SIG}
        assert ranges == {(Z.f32(Z.SIG_A[0]), Z.f32(Z.SIG_A[1])), (Z.f32(Z.SIG_B[0]), Z.f32(Z.SIG_B[1]))}, cid
    assert {c.variant for c in Z.of_kind("forward")} == set(Z.VARIANTS) == {"wave_lds", "wave_global", "thread", "sie", "epl65"}
    assert {c.B for c in Z.of_kind("shape") if c.model_name == "epl"} == {1, 3, 5, 45}
    assert {c.d_z for c in Z.of_kind("shape") if c.model_name == "wide"} == {1, 13, 63, 64, 65, 130}
    assert {(c.niter, c.variant) for c in Z.of_kind("table")} == {(n, v) for n in (50, 61, 64, 65, 130, 300) for v in ("wave_lds", "thread")}
    assert {(bool(c.consts), dict(c.env)["GIGALENS_HIP_ORDER_FUSED"]) for c in Z.of_kind("order")} == {(a, f) for a in (True, False) for f in "01"}
    assert all(c.B == 257 for c in Z.of_kind("order"))
    for c in Z.CASES:
        assert c.environment.keys() <= {"GIGALENS_HIP_PREP_LDS", "GIGALENS_HIP_WAVE_PREP", "GIGALENS_HIP_ORDER_FUSED"}, c.id
        assert c.model_name in Z.MODELS, c.id


def test_matrix_models_and_columns():
    for c in Z.CASES:
        b = Z.reference(c.id)[0]
        P = len(b.slots)
        assert len(set(b.param_cols)) == len(b.param_cols) and all(0 <= p < P for p in b.param_cols), c.id
        assert b.z.shape == (c.B, len(b.specs)) and b.z.dtype == np.float32
        n_comp = len(b.phys.lenses) + len(b.phys.lens_light) + len(b.phys.source_light)
        if c.variant == "epl65":
            assert n_comp == 65
        if c.model_name == "wide":
            assert P == 134 and len(b.specs) == c.d_z < P  # P > 64 with constants
    chain = Z.reference("chain-epl")[0]
    assert chain.param_cols != sorted(chain.param_cols)  # priors listed in another order than the packed one
    consts = sorted(set(range(len(chain.slots))) - set(chain.param_cols))
    assert consts == [4, 10]  # in the middle of the EPL's and of the source's columns


def test_z_grid_of_the_isolated_and_forward_cases():
    want = {0.0} | {sgn * v for v in (1e-3, 1, 4, 8, 12, 15, 17, 20, 40, 80) for sgn in (1, -1)}
    assert {np.float32(v) for v in Z.SIG_GRID} == {np.float32(v) for v in want}
    for c in Z.of_kind("isolated") + [Z.BY_ID["forward-wave_lds"]]:
        b = Z.reference(c.id)[0]
        for k, s in enumerate(b.specs):
            if s.bij == Z.SIG:
                assert set(b.z[:, k].tolist()) == {float(np.float32(v)) for v in want}, (c.id, k)
        amp = b.specs[[b.slots[p] for p in b.param_cols].index(("source_light", 0, "Ie"))]
        assert amp.bij == Z.EXP and {20.0, -20.0} <= set(amp.edge)
        cen = b.specs[[b.slots[p] for p in b.param_cols].index(("lens_mass", 0, "center_x"))]
        assert cen.bij == Z.ID and {500.0, -500.0} <= set(cen.edge)


@pytest.mark.parametrize("cid", [c.id for c in Z.CASES if c.kind != "table"])
def test_reference_is_finite_and_inside_the_supports(cid):
    """Every row: lo <= x <= hi on the Sigmoid columns, finite log-prior terms and gradients in float64 and in float32 (so the
    saturated rows have finite float64 values to hold the kernels to), x > 0 where a LogNormal meets a non-Exp bijector."""
    b, ref, f32 = Z.reference(cid)
    for ev, dt in ((ref, np.float64), (f32, np.float32)):
        for key in ("x", "t", "dxdz", "dlogp", "dfldj"):
            assert np.all(np.isfinite(ev[key])), (cid, key, dt)
        for k, s in enumerate(b.specs):
            if s.bij == Z.SIG:
                assert np.all((ev["x"][:, k] >= dt(s.lo)) & (ev["x"][:, k] <= dt(s.hi))), (cid, k)
            if s.prior == Z.LOGNORMAL and s.bij != Z.EXP:
                assert np.all(ev["x"][:, k] > 0), (cid, k)


def _oracle_images(b, dtype):
    from oracle import ref_torch as ref
    rows = torch.from_numpy(b.rows(Z.reference(b.case.id)[1]["x"].astype(np.float32))).to(dtype)
    rs = ref.RefSimulator(b.phys, Z.sim_config(), rows.shape[0], dtype=dtype)
    return rs, rows, rs.simulate(H.struct_from_packed(b.phys, rows)).detach().numpy()


@pytest.mark.parametrize("cid", [c.id for c in Z.CASES if c.kind in ("forward", "isolated", "chain", "shape", "table")])
def test_oracle_image_is_finite_on_every_row(cid):
    """With an all-zero mask the likelihood sums are 0 only if the image is finite: the oracle's image of every row, in float64
    and in float32."""
    b = Z.reference(cid)[0]
    for dtype in (torch.float64, torch.float32):
        img = _oracle_images(b, dtype)[2]
        assert np.all(np.isfinite(img)), (cid, dtype, np.argwhere(~np.isfinite(img))[:3])


def test_chain_case_has_one_nan_likelihood_row():
    from oracle import ref_torch as ref
    b = Z.reference("chain-epl")[0]
    rs, rows, img = _oracle_images(b, torch.float64)
    obs = chain_observation(img)
    ll, _ = ref.stats_pixels(rs, H.struct_from_packed(b.phys, rows), obs, CHAIN_BG, CHAIN_T)
    ll = ll.detach().numpy()
    assert np.isnan(ll[Z.NAN_ROW]) and np.all(np.isfinite(np.delete(ll, Z.NAN_ROW)))
    sig = [k for k, s in enumerate(b.specs) if s.bij == Z.SIG]
    assert {8.0, 12.0, 15.0} <= set(np.abs(b.z[:, sig]).reshape(-1).tolist())  # the chain-rule factor where sg (1 - sg) cancels


CHAIN_BG, CHAIN_T = 0.05, 100.0


def chain_observation(img):
    """The observed image of the chain case: the mean image of the rows with a finite likelihood (a deterministic stand-in for data)."""
    keep = [r for r in range(img.shape[0]) if r != Z.NAN_ROW]
    return np.asarray(img, dtype=np.float64)[keep].mean(axis=0).astype(np.float32)


def test_epl_cases_sit_away_from_the_series_length_thresholds():
    """niter = log(tol) / log(f) + 2 of every EPL sample, in float64, is at least 0.05 from an integer (so float32 and float64 agree
    on K) -- e = 0 alone is exempt: log f = -inf makes niter exactly 2 in both formats.  The table cases land K where they say."""
    for c in Z.CASES:
        if c.model_name == "sie":
            continue
        b, ref, _ = Z.reference(c.id)
        rows = b.rows(ref["x"].astype(np.float32))
        off = b.slots.index(("lens_mass", 0, "e1"))
        Ks = []
        for r in rows:
            f, _, niter, K = Z.epl_head(r[off], r[off + 1], r[off - 1], c.niter)
            f32_K = Z.epl_head(r[off], r[off + 1], r[off - 1], c.niter, Z.F32)[3]
            assert f32_K == K, (c.id, niter)
            Ks.append(K)
            if f == 0:
                assert niter == 2.0 and K == 1
                continue
            if c.kind == "order" and abs(niter - round(niter)) < 0.05:
                continue  # 257 random draws: the GPU test compares the trip count of the other rows only
            assert abs(niter - round(niter)) >= 0.05, (c.id, niter)
        if c.kind == "table":
            natural = [12, 49, 60, 61, 64, 65, 127, 128, 129, 400]
            assert Ks[:10] == [min(k, c.niter) for k in natural], (c.id, Ks)
            assert Ks[10] == 1 and rows[11][off - 1] == 1.0 and rows[12][off - 1] == 1.0
            if c.niter == 300:
                assert max(Ks) == 300 > 255  # beyond the clamp of the counting sort
        if c.kind == "order":
            assert len(set(Ks)) > 4


def test_workspace_layout_refuses_a_null_model():
    """gl_model_workspace_layout launches nothing and validates its arguments without a GPU."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    out = _native.gl_workspace_layout()
    assert _native.lib().gl_model_workspace_layout(None, 4, -1, ctypes.byref(out)) == -1  # GL_EINVAL
    assert b"null argument" in _native.lib().gl_last_error()
