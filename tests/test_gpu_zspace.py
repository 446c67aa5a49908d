"""The unconstrained-space front end (gl_prep_kernel / gl_prep_wave_kernel: z -> constrained rows, derived constants, the EPL
coefficient table, the dispatch order) and back end (gl_finalize_kernel: log-prior + log|J| and the gradient carried back to z)
against the float64 restatement of tests/zspace_cases.py, case by case (tests/test_zspace_host.py pins the restatement and the
inputs).  The models take their prior as raw column tuples (Model.set_prior), so all twelve (bijector, prior) pairs run; the rows
and tables are read back from the workspace (Model.workspace_rows).  Gates: four times the float32 yardstick of the case, never below
the floor of the number format (zspace_cases.gate); every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import zspace_cases as Z
from tests.test_gpu_parity import GRAD_RTOL_COL, IMG_RTOL, LL_RTOL, gl  # noqa: F401

pytestmark = pytest.mark.gpu
U = Z.U


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _launch(gl, monkeypatch, built, z=None, mask_zero=True, obs=None, err=True, bg=0.2, t=100.0):
    """gl_logprob_fwd_bwd on the case's z, the workspace read back, then gl_loglike_fwd_bwd on the read-back rows."""
    for k, v in built.case.environment.items():
        monkeypatch.setenv(k, v)  # read at model creation
    B, n = built.case.B, Z.NUM_PIX
    sim = gl.LensSimulator(built.phys, Z.sim_config(), bs=B)
    m = sim._model
    m.set_prior(built.columns, built.const_row)
    dev = m.device
    obs_t = (torch.zeros((n, n)) if obs is None else torch.from_numpy(np.asarray(obs, dtype=np.float32))).to(dev).contiguous()
    err_t = torch.ones((n, n), device=dev) if err else None
    mask = torch.zeros((n, n), device=dev) if mask_zero else None
    zt = torch.from_numpy(np.ascontiguousarray(built.z if z is None else z)).to(dev)
    lp, ll, _, gz = m.logprob(zt, obs_t, err_t, mask, bg, t, True)
    torch.cuda.synchronize()
    rows = {k: v.clone() for k, v in m.workspace_rows(B).items()}
    ll_p, _, G = m.loglike(rows["params"], obs_t, err_t, mask, bg, t, True)
    torch.cuda.synchronize()
    derived_p = m.workspace_rows(B)["derived"].clone()
    lay = m.workspace_layout(B, 0)
    assert (lay.P, lay.p_off) == (len(built.slots), 0) and lay.params_count == B * lay.P and lay.order_count == lay.cost_count == B
    cpu = lambda v: v.cpu().numpy()
    return dict(lp=cpu(lp), ll=cpu(ll), gz=cpu(gz), x=cpu(rows["params"]), derived=cpu(rows["derived"]), order=cpu(rows["order"]),
                cost=cpu(rows["cost"]), ll_p=cpu(ll_p), G=cpu(G), derived_p=cpu(derived_p), d_off=lay.d_off, D=lay.D)


def _check_forward(built, ref, f32, out):
    """The read-back constrained rows against float64; constants and Identity columns bitwise; Sigmoid columns inside [lo, hi]; the
    derived rows of the z entry bitwise those of the row entry on the read-back rows."""
    cid, x = built.case.id, out["x"]
    assert not np.isnan(x).any()
    consts = sorted(set(range(x.shape[1])) - set(built.param_cols))
    assert np.array_equal(_bits(x[:, consts]), _bits(np.broadcast_to(built.const_row[consts], (x.shape[0], len(consts)))))
    xz = x[:, built.param_cols]
    for k, s in enumerate(built.specs):
        if s.bij == Z.ID:
            assert np.array_equal(_bits(xz[:, k]), _bits(built.z[:, k])), (cid, k)
        if s.bij == Z.SIG:
            assert np.all((xz[:, k] >= np.float32(s.lo)) & (xz[:, k] <= np.float32(s.hi))), (cid, k, xz[:, k])
    yard = Z.worst(f32["x"] - ref["x"], ref["xs"])
    g = Z.gate(yard, 4 * U)
    err = Z.worst(xz - ref["x"], ref["xs"])
    print(f"ZSPACE {cid}: x yardstick {yard:.3g} gate {g:.3g} kernel {err:.3g} ratio {err / g:.3f}")
    assert np.all(np.abs(xz - ref["x"]) <= g * ref["xs"]), cid
    assert np.array_equal(_bits(out["derived"]), _bits(out["derived_p"])), cid


def _check_prior_terms(built, ref, f32, out, G=None, rows=None):
    """lp = loglike + sum_k (logp_k + fldj_k) and grad_z = (G[param_col] + dlogp/dx) dx/dz + dfldj/dz against float64.  ``G`` None: the
    all-zero mask, where the likelihood sums -- and the kernel's own likelihood gradient -- are exactly 0."""
    cid, d = built.case.id, len(built.specs)
    rows = np.arange(out["lp"].shape[0]) if rows is None else np.asarray(rows)
    if G is None:
        assert np.all(out["ll"] == 0) and np.all(out["ll_p"] == 0) and np.all(out["G"] == 0), cid
        G = np.zeros_like(out["G"])
    assert np.array_equal(_bits(out["ll"][rows]), _bits(out["ll_p"][rows])), cid
    ll = out["ll"].astype(np.float64)
    (lp64, S), (lp32, _) = Z.log_prior(ref), Z.log_prior(f32)
    assert np.all(np.isfinite(lp64))
    S = S + np.abs(ll)  # (the log-likelihood is one more term of the sum; 0 under the all-zero mask)
    yard = Z.worst(((out["ll"] + lp32).astype(np.float64) - (ll + lp64))[rows], S[rows])
    g = Z.gate(yard, (d + 8) * U)
    e = np.abs(out["lp"].astype(np.float64) - (ll + lp64))[rows]
    print(f"ZSPACE {cid}: lp yardstick {yard:.3g} gate {g:.3g} kernel {Z.worst(e, S[rows]):.3g} ratio {Z.worst(e, S[rows]) / g:.3f}")
    (g64, sc), (g32, _) = Z.grad_z(ref, G, built.param_cols), Z.grad_z(f32, G, built.param_cols)
    assert np.all(np.isfinite(g64[rows]))
    yard_g = Z.worst((g32 - g64)[rows], sc[rows])
    gg = Z.gate(yard_g, 4 * U)
    eg = np.abs(out["gz"].astype(np.float64) - g64)[rows]
    print(f"ZSPACE {cid}: grad_z yardstick {yard_g:.3g} gate {gg:.3g} kernel {Z.worst(eg, sc[rows]):.3g} "
          f"ratio {Z.worst(eg, sc[rows]) / gg:.3f}")
    assert np.all(np.isfinite(out["lp"][rows])) and np.all(np.isfinite(out["gz"][rows])), cid
    assert np.all(e <= g * S[rows]), (cid, np.argmax(e / S[rows]))
    bad = eg > gg * sc[rows]
    assert not bad.any(), (cid, np.argwhere(bad)[:5], out["gz"][rows][bad][:5], g64[rows][bad][:5])


@pytest.mark.parametrize("cid", [c.id for c in Z.of_kind("forward", "isolated", "shape")])
def test_bijectors_prior_and_gradient_in_isolation(gl, monkeypatch, cid):
    """Every front-end variant, all twelve (bijector, prior) pairs under both finalize instantiations, the batch sizes and column
    counts at which the kernels change path, over the z grid up to saturation: the constrained rows, and -- with an all-zero mask,
    where ``chi2_terms`` multiplies every pixel by 0 -- lp = sum (logp + fldj) and grad_z = dlogp/dx dx/dz + dfldj/dz alone."""
    from gigalens_amd import _native
    built, ref, f32 = Z.reference(cid)
    try:
        out = _launch(gl, monkeypatch, built)
    except _native.NativeLibraryError as e:  # an EPL model of 65 components may be beyond the model limits: the typed refusal
        print(f"ZSPACE {cid}: refused: {e}")
        assert built.case.variant == "epl65" and "gigalens_hip error -2" in str(e), e
        return
    _check_forward(built, ref, f32, out)
    _check_prior_terms(built, ref, f32, out)


def test_chain_rule_column_map_and_nan_row(gl, monkeypatch):
    """With the mask off: grad_z[k] = (G[param_col_k] + dlogp/dx) dx/dz + dfldj/dz, formed in float64 from G, the kernel's own loglike
    gradient on the read-back rows; the priors are listed in another order than the packed one with constants in the middle of a
    component; Sigmoid columns sit at |z| = 8, 12, 15 where dx/dz carries the whole likelihood gradient.  The NaN-likelihood row
    is all NaN and its neighbours are bitwise what they are beside a finite row."""
    from tests.test_zspace_host import CHAIN_BG, CHAIN_T, _oracle_images, chain_observation
    built, ref, f32 = Z.reference("chain-epl")
    obs = chain_observation(_oracle_images(built, torch.float64)[2])
    out = _launch(gl, monkeypatch, built, mask_zero=False, obs=obs, err=False, bg=CHAIN_BG, t=CHAIN_T)
    keep = [r for r in range(built.case.B) if r != Z.NAN_ROW]
    assert np.isnan(out["lp"][Z.NAN_ROW]) and np.isnan(out["ll"][Z.NAN_ROW]) and np.isnan(out["gz"][Z.NAN_ROW]).all()
    assert np.isnan(out["G"][Z.NAN_ROW]).all() and np.isfinite(out["G"][keep]).all() and np.abs(out["G"][keep]).max() > 1
    _check_forward(built, ref, f32, out)
    _check_prior_terms(built, ref, f32, out, G=out["G"], rows=keep)
    z2 = built.z.copy()
    amp = [built.slots[p] for p in built.param_cols].index(("source_light", 0, "Ie"))
    assert z2[Z.NAN_ROW, amp] < 0
    z2[Z.NAN_ROW, amp] = 50.0
    out2 = _launch(gl, monkeypatch, built, z=z2, mask_zero=False, obs=obs, err=False, bg=CHAIN_BG, t=CHAIN_T)
    assert np.isfinite(out2["lp"]).all() and np.isfinite(out2["gz"]).all()
    for key in ("lp", "ll", "gz"):
        assert np.array_equal(_bits(out[key][keep]), _bits(out2[key][keep])), key


@pytest.mark.parametrize("cid", [c.id for c in Z.of_kind("table")])
def test_epl_table_vs_float64(gl, monkeypatch, cid):
    """Rows 0 .. K + 3 of the EPL coefficient table of the z entry, by the wavefront's scan (more than one 64-row round from
    K = 61) and by the sequential form, K up to 300: every entry relative to its own value; zero rows and K exact."""
    built, ref, f32 = Z.reference(cid)
    out = _launch(gl, monkeypatch, built)
    _check_forward(built, ref, f32, out)
    _check_prior_terms(built, ref, f32, out)
    cap, off = built.case.niter, built.slots.index(("lens_mass", 0, "e1"))
    blocks = out["derived"][:, out["d_off"]:]
    errs, yards = [], []
    for r, row in enumerate(out["x"]):
        f, s, _, K = Z.epl_head(row[off], row[off + 1], row[off - 1], cap)
        f_32, s_32, _, K32 = Z.epl_head(row[off], row[off + 1], row[off - 1], cap, Z.F32)
        assert K32 == K and blocks[r, Z.EPL_K] == K and _bits(blocks[r])[Z.EPL_KI] == K and out["cost"][r] == K, (cid, r, K)
        tab = blocks[r, Z.EPL_TAB:Z.EPL_TAB + 4 * (K + 4)].reshape(K + 4, 4)
        want = Z.epl_table_ref(f, s, K)
        errs.append(Z.table_row_errors(tab, want))
        yards.append(Z.table_row_errors(Z.epl_table_f32(f_32, s_32, K), want))
    yard = max(float(y.max()) for y in yards)
    assert np.isfinite(yard)
    worst_ratio = 0.0
    for r, e in enumerate(errs):
        g = Z.gate(yard, (np.arange(e.size) + 2) * U)
        worst_ratio = max(worst_ratio, float((e / g).max()))
    print(f"ZSPACE {cid}: table yardstick {yard:.3g} (4x: {4 * yard:.3g}) kernel {max(float(e.max()) for e in errs):.3g} "
          f"worst error / gate {worst_ratio:.3f} K {[e.size - 4 for e in errs]}")
    for r, e in enumerate(errs):
        g = Z.gate(yard, (np.arange(e.size) + 2) * U)
        assert np.all(e <= g), (cid, r, int(np.argmax(e / g)), float(e.max()))


@pytest.mark.parametrize("cid", [c.id for c in Z.of_kind("order")])
def test_order_on_the_z_path(gl, monkeypatch, cid):
    """B = 257 with e1 / e2 under TruncatedNormal columns (and e1 a constant): the order is a permutation sorted by the cost the
    sample wavefronts wrote, which is the trip count of the float64 head wherever niter is not within 0.05 of an integer."""
    built, ref, f32 = Z.reference(cid)
    out = _launch(gl, monkeypatch, built)
    order, cost, B = out["order"], out["cost"], built.case.B
    print(f"ZSPACE {cid}: cost min {cost.min()} max {cost.max()} distinct {len(set(cost.tolist()))}")
    assert sorted(order.tolist()) == list(range(B))
    assert np.all(np.diff(cost[order]) <= 0), "not sorted heaviest first"
    assert cost.min() >= 0 and cost.max() > cost.min()
    off, n_held = built.slots.index(("lens_mass", 0, "e1")), 0
    for r, row in enumerate(out["x"]):
        _, _, niter, K = Z.epl_head(row[off], row[off + 1], row[off - 1], built.case.niter)
        if abs(niter - round(niter)) >= 0.05:
            assert cost[r] == K, (cid, r, niter, cost[r])
            n_held += 1
    assert n_held > B // 2
    _check_forward(built, ref, f32, out)


def test_long_series_end_to_end(gl):
    """EPL(niter=140) at |e| ~ 0.8 on 16 x 16, B = 3: a series of ~95 rows (two scan rounds in the front end, twice the rows of
    any other pixel-likelihood case) -- image, log-likelihood and gradient against the oracle at the tolerances of
    test_simulate_loglike_grad_vs_oracle."""
    wl = Z.long_workload()
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=11)
    ee = np.hypot(*packed[:, 2:4].cpu().numpy().T)
    K = [Z.epl_head(r[2], r[3], r[1], Z.LONG_NITER)[3] for r in packed.cpu().numpy()]
    print(f"ZSPACE long: |e| {ee} K {K}")
    assert np.all(np.abs(ee - 0.8) < 0.05) and min(K) > 64 and max(K) < Z.LONG_NITER
    obs_np = obs.cpu().numpy()
    ll_o, red_o, g_o, img_o = H.oracle_loglike_and_grad(wl, packed.cpu().double(), obs_np, None, wl.batch)
    img = sim.simulate(packed).cpu().numpy().reshape(img_o.shape)
    print(f"ZSPACE long: image error {np.abs(img - img_o).max() / np.abs(img_o).max():.3g} (gate {IMG_RTOL})")
    assert np.abs(img - img_o).max() <= IMG_RTOL * np.abs(img_o).max() + 1e-7
    pm = gl.ForwardProbModel(wl.prior, obs_np, wl.background_rms, wl.exp_time, include_positions=False)
    p = packed.clone().requires_grad_(True)
    ll, red = pm._pixel_stats_packed(sim, p)
    ll.sum().backward()
    g = p.grad.cpu().numpy()
    print(f"ZSPACE long: loglike error {H.relerr(ll.detach().cpu().numpy(), ll_o):.3g} (gate {LL_RTOL}) "
          f"gradient error {H.grad_col_err(g, g_o).max():.3g} (gate {GRAD_RTOL_COL})")
    assert np.allclose(ll.detach().cpu().numpy(), ll_o, rtol=LL_RTOL)
    assert np.allclose(red.detach().cpu().numpy(), red_o, rtol=LL_RTOL)
    bad = H.grad_col_err(g, g_o) > GRAD_RTOL_COL
    assert not bad.any(), (np.argwhere(bad)[:5], g[bad][:5], g_o[bad][:5], H.grad_col_err(g, g_o).max())
    # the z entry of the same model: log_prob through the front end's scan and the fused prior
    z = pm.bij.inverse(wl.prior.sample(wl.batch, seed=11)).to("cuda")
    lp, _, gz = pm.log_prob_and_grad(sim, z)
    assert torch.isfinite(lp).all() and torch.isfinite(gz).all()
