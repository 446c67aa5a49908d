"""The five kernels of csrc/gl_updates.hip.h (Adam, the SVI surrogate's sample and gradient, the HMC kick+drift and Metropolis
step), called through ``_native`` and held to the float64 restatements of tests/inference_cases.py at their launch and reduction
edges: 256-thread blocks, 64-lane waves, HMC_WG = 128, the d <= 4096 limit of the C entry points.  Every gate is a derived bound
(``inference_cases``: gamma_n sum |terms|, n read off the kernel), bit equality, or 4 x a float32 CPU yardstick computed here."""
import numpy as np
import pytest
import torch

from tests import inference_cases as IC

pytestmark = pytest.mark.gpu
SHIFTS = (0.0, 1e-6, 0.5)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


def over(what, got, want, bound):
    """worst |got - want| / bound, printed (the figures DESIGN section 5 quotes)"""
    r = float((np.abs(np.asarray(got, dtype=np.float64) - want) / bound).max())
    print(f"RATIO {what} {r:.3f}")
    return r


# ---- gl_adam_kernel ---------------------------------------------------------------------------------------------------------------
def _adam_once(x, m, v, g, hyper, t):
    from gigalens_amd import _native
    xd, md, vd, gd = dev(x), dev(m), dev(v), dev(g)
    _native.adam_update(xd, gd, md, vd, hyper["scale"], hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], t)
    return xd, md, vd


@pytest.mark.parametrize("scale", [1.0, -0.25])
@pytest.mark.parametrize("t", [1, 2, 5000])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_adam_one_step_against_float64(n, t, scale):
    x, m, v, g = IC.adam_case(n, seed=n)
    hyper = dict(IC.HYPER, scale=scale)
    got = _adam_once(x, m, v, g, hyper, t)
    want, bound = IC.adam64(x, m, v, g, hyper, t), IC.adam_bound(x, m, v, g, hyper, t)
    for name, a, w, b in zip("xmv", got, want, bound):
        assert over(f"adam-{name}-n{n}-t{t}-s{scale}", host(a), w, b) <= 1


def test_adam_200_steps_against_float64():
    """The optimiser's own loop (host step count) over 200 given gradients.  Gate: 4 x the worst deviation from float64 of the same
    recurrence in float32 on the CPU, in the kernel's operation order."""
    from gigalens_amd.inference import Adam
    n, steps, hyper = 1000, 200, dict(IC.HYPER, scale=-0.25)
    r = np.random.default_rng(5)
    x0 = r.standard_normal(n).astype(np.float32)
    grads = (r.standard_normal((steps, n)) * 10.0 ** r.uniform(-3, 3, (steps, 1))).astype(np.float32)
    s64, s32 = (x0, np.zeros(n), np.zeros(n)), (x0, np.zeros(n), np.zeros(n))
    for t in range(1, steps + 1):
        s64 = IC.adam64(*s64, grads[t - 1], hyper, t)
        s32 = IC.adam64(*s32, grads[t - 1], hyper, t, dtype=np.float32)
    opt = Adam(hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"])
    xd, gd = dev(x0), dev(grads)
    for t in range(steps):
        opt.step(xd, gd[t], hyper["scale"])
    assert opt.t == steps
    for name, a, w32, w64 in zip("xmv", (xd, opt.m, opt.v), s32, s64):
        yard = float(np.abs(w32.astype(np.float64) - w64).max())
        err = float(np.abs(host(a).astype(np.float64) - w64).max())
        print(f"YARDSTICK adam200-{name} float32 {yard:.3e} kernel {err:.3e} ratio-to-gate {err / (4 * yard):.3f}")
        assert err <= 4 * yard


def test_adam_zero_learning_rate_keeps_the_bits_of_x():
    x, m, v, g = IC.adam_case(600, seed=2)
    x[:6] = [-0.0, -0.0, 0.0, 0.0, 3.0e38, -3.0e38]
    g[:4] = [2.0, -2.0, 2.0, -2.0]  # the zero update comes with either sign: x - (-0.0) would turn -0.0 into +0.0
    m[:4] = 0.0
    hyper = dict(IC.HYPER, lr=0.0)
    xd, md, vd = _adam_once(x, m, v, g, hyper, 3)
    assert np.array_equal(bits(xd), x.view(np.int32))
    want, bound = IC.adam64(x, m, v, g, hyper, 3), IC.adam_bound(x, m, v, g, hyper, 3)
    assert over("adam-lr0-m", host(md), want[1], bound[1]) <= 1 and over("adam-lr0-v", host(vd), want[2], bound[2]) <= 1
    assert not np.array_equal(host(md), m) and not np.array_equal(host(vd), v)


def test_adam_isolates_zero_and_non_finite_gradients():
    n = 600
    x, _, _, g = IC.adam_case(n, seed=3)
    zero = np.zeros(n, dtype=np.float32)
    xd, md, vd = _adam_once(x, zero, zero, zero, IC.HYPER, 1)  # 0 / (sqrt(0) + eps): a zero update, not 0 / 0
    assert np.array_equal(bits(xd), x.view(np.int32)) and not host(md).any() and not host(vd).any()
    _, m, v, _ = IC.adam_case(n, seed=3)
    bad = g.copy()
    bad[5], bad[300] = np.nan, np.inf
    clean, dirty = _adam_once(x, m, v, g, IC.HYPER, 4), _adam_once(x, m, v, bad, IC.HYPER, 4)
    others = np.ones(n, dtype=bool)
    others[[5, 300]] = False
    for a, b in zip(clean, dirty):
        assert np.array_equal(bits(a)[others], bits(b)[others])
    assert not np.isfinite(host(dirty[0])[[5, 300]]).any()


def test_adam_device_counter_in_a_graph_on_257_blocks():
    """``step_captured`` inside a real HIP graph on a multi-block grid: the last block to take a ticket advances the counter, once
    per replay, and leaves the ticket word at zero."""
    from gigalens_amd.inference import Adam
    n, K, hyper = 65537, 5, dict(IC.HYPER, scale=-0.25)
    x, m, v, g = IC.adam_case(n, seed=11)

    def fresh():
        opt = Adam(hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"])
        opt.t, opt.m, opt.v = 7, dev(m), dev(v)
        return opt, dev(x)

    gd = dev(g)
    opt, xd = fresh()
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):  # the warm-up of ``MAP``: three steps off the default stream
        for _ in range(3):
            opt.step_captured(xd, gd, hyper["scale"])
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step_captured(xd, gd, hyper["scale"])
    worst = 0.0
    for k in range(K):
        before = tuple(host(a) for a in (xd, opt.m, opt.v))
        graph.replay()
        t = 7 + 3 + k + 1
        want, bound = IC.adam64(*before, g, hyper, t), IC.adam_bound(*before, g, hyper, t)
        worst = max([worst] + [float((np.abs(host(a).astype(np.float64) - w) / b).max()) for a, w, b in zip((xd, opt.m, opt.v), want, bound)])
    print(f"RATIO adam-graph-replays {worst:.3f}")
    assert worst <= 1
    torch.cuda.synchronize()
    assert not host(opt._t_dev[1:2].view(torch.int32)).any()  # the ticket word, before the sync drops the buffer
    opt.sync_from_device()
    assert opt.t == 7 + 3 + K
    del graph
    plain, xp = fresh()
    for _ in range(3 + K):
        plain.step_captured(xp, gd, hyper["scale"])
    plain.sync_from_device()
    assert plain.t == opt.t
    for a, b in zip((xd, opt.m, opt.v), (xp, plain.m, plain.v)):
        assert np.array_equal(bits(a), bits(b))


# ---- gl_svi_sample_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_rank", [True, False])
@pytest.mark.parametrize("d", [1, 2, 13, 64, 65, 132])
def test_svi_sample_against_float64(d, full_rank):
    from gigalens_amd import _native
    worst = 0.0
    for n in (1, 63, 64, 65, 257):
        mu, lp, eps, _, _ = IC.svi_case(n, d, full_rank, seed=100 * d + n)
        for shift in SHIFTS:
            z = host(_native.svi_sample(dev(mu), dev(lp), dev(eps), full_rank, shift))
            want, bound = IC.svi_sample64(mu, lp, eps, full_rank, shift), IC.svi_sample_bound(mu, lp, eps, full_rank, shift)
            worst = max(worst, float((np.abs(z - want) / bound).max()))
    print(f"RATIO svi_sample-d{d}-{'full' if full_rank else 'diag'} {worst:.3f}")
    assert worst <= 1


def test_svi_sample_d1_gives_the_two_documented_formulas():
    """At d = 1 the packed length does not tell the surrogates apart: ``full_rank`` does.  Full rank: mu + (exp(p) + shift) eps;
    mean field: mu + exp(p) eps.  With exp(p) = shift = 1e-6 the two differ by a factor of two in the scale."""
    from gigalens_amd import _native
    mu, p = np.float32([0.0]), np.float32([IC.SMALL_P])  # (mu = 0: the bound is relative to the scale, and tells 1e-6 from 2e-6)
    eps = np.random.default_rng(0).standard_normal((65, 1)).astype(np.float32)
    e = np.exp(np.float64(p[0]))
    for full_rank, scale in ((True, e + IC.f32(1e-6)), (False, e)):
        z = host(_native.svi_sample(dev(mu), dev(p), dev(eps), full_rank, 1e-6))
        want = scale * eps.astype(np.float64)
        assert (np.abs(z - want) <= IC.svi_sample_bound(mu, p, eps, full_rank, 1e-6)).all()


# ---- gl_svi_grad_kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_rank", [True, False])
@pytest.mark.parametrize("d", [1, 2, 3, 13, 132])
def test_svi_grad_against_float64(d, full_rank):
    """Given eps, log p ~ 1e5 and G over five decades: no log-prob function, so no float32 evaluation noise enters."""
    from gigalens_amd import _native
    worst = np.zeros(3)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 777):
        mu, lp, eps, logp, G = IC.svi_case(n, d, full_rank, seed=1000 * d + n)
        for shift in SHIFTS:
            buf = host(_native.svi_grad(dev(lp), dev(eps), dev(logp), dev(G), full_rank, shift))
            want = IC.svi_buffer64(lp, eps, logp, G, full_rank, shift)
            r = np.abs(buf - want) / IC.svi_buffer_bound(lp, eps, logp, G, full_rank, shift)
            worst = np.maximum(worst, [r[0], r[1:1 + d].max(), r[1 + d:].max()])
    print(f"RATIO svi_grad-d{d}-{'full' if full_rank else 'diag'} elbo {worst[0]:.3f} dmu {worst[1]:.3f} dp {worst[2]:.3f}")
    assert worst.max() <= 1


def test_svi_grad_index_map_is_exact():
    """d = 300, full rank: 45 150 packed outputs, one workgroup each, every one placed by ``tril_jk``.  The off-diagonal values
    -(j + 1)(k + 1) / 1024 are exact in float32, so a wrong (j, k) at any t is a wrong bit pattern."""
    from gigalens_amd import _native
    d = 300
    lp, eps, logp, G, jj, kk, exact = IC.index_map_case(d)
    assert lp.size == 45150
    buf = host(_native.svi_grad(dev(lp), dev(eps), dev(logp), dev(G), True, 1e-6))
    got, off = buf[1 + d:], jj != kk
    wrong = np.flatnonzero(got[off].view(np.int32) != exact[off].view(np.int32))
    assert wrong.size == 0, (wrong[:8], got[off][wrong[:8]], exact[off][wrong[:8]])
    assert np.array_equal(buf[1:1 + d], -G[0])
    want, bound = IC.svi_buffer64(lp, eps, logp, G, True, 1e-6), IC.svi_buffer_bound(lp, eps, logp, G, True, 1e-6)
    assert over("svi_grad-index-map-diagonal", got[~off], want[1 + d:][~off], bound[1 + d:][~off]) <= 1


@pytest.mark.parametrize("full_rank", [True, False])
def test_svi_grad_diagonal_terms(full_rank):
    """The Exp diagonal written out: full rank v e - e / (e + shift), mean field v e - 1, v = -mean G_j eps_j, at p_jj = log(1e-6)
    (the shift is half of L_jj) among ordinary ones."""
    from gigalens_amd import _native
    n, d = 64, 13
    mu, lp, eps, logp, G = IC.svi_case(n, d, full_rank, seed=7)
    jj, kk = IC.tril_rows(d)
    diag = np.flatnonzero(jj == kk) if full_rank else np.arange(d)
    p = lp[diag].astype(np.float64)
    assert (lp[diag][::3] == np.float32(IC.SMALL_P)).all()
    v = -(G.astype(np.float64) * eps.astype(np.float64)).mean(0)
    for shift in SHIFTS:
        e = np.exp(p)
        want = v * e - e / (e + IC.f32(shift)) if full_rank else v * e - 1.0
        buf = host(_native.svi_grad(dev(lp), dev(eps), dev(logp), dev(G), full_rank, shift))
        bound = IC.svi_buffer_bound(lp, eps, logp, G, full_rank, shift)[1 + d:][diag]
        assert over(f"svi_grad-diagonal-{'full' if full_rank else 'diag'}-shift{shift}", buf[1 + d:][diag], want, bound) <= 1


# ---- gl_hmc_kick_drift_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("d", [1, 2, 127, 128, 129, 300, 4096])
def test_hmc_kick_drift_against_float64(d, n):
    from gigalens_amd import _native
    p, g, kick, z, sigma, eps = IC.kick_case(n, d, seed=10 * d + n)
    pd, gd, zd, sd = dev(p), dev(g), dev(z), dev(sigma)
    p_out, z_out = torch.empty_like(pd), torch.empty_like(zd)
    _native.hmc_kick_drift(pd, gd, kick, zd, sd, eps, p_out, z_out)
    want, bound = IC.kick_drift64(p, g, kick, z, sigma, eps), IC.kick_drift_bound(p, g, kick, z, sigma, eps)
    assert over(f"kick_drift-p-d{d}-n{n}", host(p_out), want[0], bound[0]) <= 1
    assert over(f"kick_drift-z-d{d}-n{n}", host(z_out), want[1], bound[1]) <= 1
    assert np.array_equal(host(pd), p) and np.array_equal(host(zd), z)
    # every output element is read and written by one thread: the aliased forms give the bits of the out-of-place call
    for alias_p, alias_z in ((True, True), (True, False), (False, True)):
        pi, zi = pd.clone(), zd.clone()
        po, zo = (pi if alias_p else torch.empty_like(pi)), (zi if alias_z else torch.empty_like(zi))
        _native.hmc_kick_drift(pi, gd, kick, zi, sd, eps, po, zo)
        assert np.array_equal(bits(po), bits(p_out)) and np.array_equal(bits(zo), bits(z_out))


@pytest.mark.parametrize("d", [4097, 0])
def test_hmc_kick_drift_refuses_d_outside_1_4096(d):
    from gigalens_amd import _native
    n = 2
    p, g, z = (torch.zeros(n, d, device="cuda") for _ in range(3))
    sigma = torch.zeros(max(d, 1), max(d, 1), device="cuda")
    p_out, z_out = (torch.full((n, max(d, 1)), 7.0, device="cuda") for _ in range(2))
    with pytest.raises(_native.NativeLibraryError):
        _native.hmc_kick_drift(p, g, 0.1, z, sigma, 0.1, p_out, z_out)
    torch.cuda.synchronize()
    assert bool((p_out == 7.0).all()) and bool((z_out == 7.0).all())  # nothing was launched


# ---- gl_hmc_accept_kernel ---------------------------------------------------------------------------------------------------------
def _accept(c, L=None):
    """run the kernel on a case; returns numpy (z, g, lp, acc_prob, moved)"""
    from gigalens_amd import _native
    z, g, lp = dev(c["z"]), dev(c["g"]), dev(c["lp"])
    acc = torch.full((c["z"].shape[0],), -1.0, device="cuda")
    _native.hmc_accept(z, g, lp, dev(c["zn"]), dev(c["gn"]), dev(c["lpn"]), dev(c["p0"]), dev(c["pn"]), c["kick"],
                       dev(c["L"] if L is None else L), dev(c["u"]), acc)
    z, g, lp, acc = host(z), host(g), host(lp), host(acc)
    return z, g, lp, acc, (z.view(np.int32) == c["zn"].view(np.int32)).all(-1)


def _selected(c, out):
    z, g, lp, _, moved = out
    sel = moved[:, None]
    return (np.array_equal(z.view(np.int32), np.where(sel, c["zn"], c["z"]).view(np.int32))
            and np.array_equal(g.view(np.int32), np.where(sel, c["gn"], c["g"]).view(np.int32))
            and np.array_equal(lp.view(np.int32), np.where(moved, c["lpn"], c["lp"]).view(np.int32)))


@pytest.mark.parametrize("d,n", [(d, n) for d in (1, 2, 64, 127, 128, 129, 300) for n in (1, 2, 300)] + [(4096, 2)])
def test_hmc_accept_against_float64(d, n):
    c = IC.accept_case(n, d, seed=10 * d + n)
    want = IC.accept64(**c)
    b_la, b_acc, b_dec = IC.accept_bound(c["lp"], c["gn"], c["lpn"], c["p0"], c["pn"], c["kick"], c["L"], c["u"])
    called = want["margin"] > b_dec
    assert called.mean() >= 0.98  # float64 alone: the draw keeps the cap
    out = _accept(c)
    assert over(f"accept-prob-d{d}-n{n}", out[3], want["acc_prob"], b_acc) <= 1
    print(f"RATIO accept-closest-decision-d{d}-n{n} {float((b_dec / want['margin'])[called].max()):.3f} accepted {want['take'].mean():.2f}")
    assert np.array_equal(out[4][called], want["take"][called])
    assert _selected(c, out)


@pytest.mark.parametrize("d", [2, 129, 300])
def test_hmc_accept_never_reads_above_the_diagonal(d):
    c = IC.accept_case(3, d, seed=d)
    nan_up = np.where(np.triu(np.ones((d, d), dtype=bool), 1), np.float32(np.nan), c["L"]).astype(np.float32)
    assert np.isnan(nan_up).sum() == d * (d - 1) // 2
    for a, b in zip(_accept(c), _accept(c, nan_up)):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)


def test_hmc_accept_designed_rows_equal_the_torch_branch():
    """Today's behaviour at the edges of the Metropolis test, equal to the loop's torch branch: a NaN, +inf or -inf proposal is
    rejected with probability 0; a current log p of -inf with a finite proposal gives log_acc = +inf, which the non-finite guard
    turns into a rejection (such a chain never moves: DESIGN section 7); u = 0 accepts any finite log_acc; u = 1 accepts only
    log_acc > 0."""
    n, d = 8, 13
    c = IC.accept_case(n, d, seed=1)
    c["pn"][7], c["gn"][7] = c["p0"][7], 0.0                   # row 7: ke1 == ke0 and lpn == lp below, log_acc = 0 exactly
    lp, lpn, u = c["lp"], c["lpn"], c["u"]
    lpn[0], lpn[1], lpn[2] = np.nan, np.inf, -np.inf
    lp[3] = -np.inf
    lpn[3] = 1.0
    lpn[4], u[4] = lp[4] - 60.0, 0.0
    lpn[5], u[5] = lp[5] + 60.0, 1.0
    lpn[6], u[6] = lp[6] - 60.0, 1.0
    lpn[7], u[7] = lp[7], 1.0
    out = _accept(c)
    moved, acc = out[4], out[3]
    assert moved.tolist() == [False, False, False, False, True, True, False, False]
    assert (acc[:4] == 0).all() and 0 < acc[4] < 1e-10 and acc[5] == 1 and 0 < acc[6] < 1e-10 and acc[7] == 1
    assert _selected(c, out)
    # the loop's torch branch (ModellingSequence.HMC, ``native`` false) on the same rows
    t = {k: dev(v) for k, v in c.items() if k != "kick"}
    p1 = t["pn"] + IC.f32(c["kick"]) * t["gn"]
    ke0, ke1 = 0.5 * ((t["p0"] @ t["L"]) ** 2).sum(-1), 0.5 * ((p1 @ t["L"]) ** 2).sum(-1)
    log_acc = (t["lpn"] - ke1) - (t["lp"] - ke0)
    log_acc = torch.where(torch.isfinite(log_acc), log_acc, torch.full_like(log_acc, -float("inf")))
    assert host(torch.log(t["u"]) < log_acc).tolist() == moved.tolist()
    acc_t = host(torch.exp(torch.clamp(log_acc, max=0.0)))
    assert (acc_t[:4] == 0).all() and acc_t[5] == 1 and acc_t[7] == 1
