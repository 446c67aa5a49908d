"""Host logic of the inference drivers (no GPU): the written-out reparameterisation gradient of ``svi_step`` against
autograd through the surrogate's sampling path -- what tf/inference.py:85-91 obtains from ``tf.GradientTape``; the HMC and SMC
drivers on targets with known answers; the float64 restatements of tests/inference_cases.py against the torch branches."""
import math

import numpy as np
import pytest
import torch

from gigalens_amd import inference as inf
from tests import inference_cases as IC


def _toy_log_prob(z):
    a = torch.linspace(0.5, 2.0, z.shape[-1], dtype=z.dtype)
    return -0.5 * ((z - 0.3) ** 2 * a).sum(-1) - 0.1 * torch.sin(z).sum(-1) + 0.05 * (z[..., 0] * z[..., -1])


def _taped(mu, lp, n, gen, full_rank):
    d = mu.numel()
    mu_ = mu.clone().requires_grad_(True)
    lp_ = lp.clone().requires_grad_(True)
    L = inf.tril_unpack(lp_, d) if full_rank else torch.diag(torch.exp(lp_))
    eps = torch.randn((n, d), generator=gen, dtype=mu.dtype)
    z = mu_ + eps @ L.T
    log_q = -0.5 * (eps * eps).sum(-1) - torch.log(torch.diagonal(L)).sum() - 0.5 * d * math.log(2 * math.pi)
    elbo = (log_q - _toy_log_prob(z)).mean()
    g_mu, g_lp = torch.autograd.grad(elbo, (mu_, lp_))
    return elbo.detach(), g_mu, g_lp


@pytest.mark.parametrize("full_rank", [True, False])
@pytest.mark.parametrize("use_vg", [False, True])
def test_svi_step_gradient_equals_the_taped_one(full_rank, use_vg):
    torch.manual_seed(0)
    d, n = 6, 64
    mu = torch.randn(d, dtype=torch.float64) * 0.2
    scale = torch.tril(torch.randn(d, d, dtype=torch.float64) * 0.1) + torch.diag(torch.rand(d, dtype=torch.float64) + 0.2)
    lp = inf.tril_pack(scale) if full_rank else torch.log(torch.diagonal(scale))
    want = _taped(mu, lp, n, torch.Generator().manual_seed(5), full_rank)

    def vg(z):
        zz = z.clone().requires_grad_(True)
        v = _toy_log_prob(zz)
        (g,) = torch.autograd.grad(v.sum(), zz)
        return v.detach(), g

    got = inf.svi_step(mu, lp, None if use_vg else _toy_log_prob, n, torch.Generator().manual_seed(5),
                       value_and_grad_fn=vg if use_vg else None)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12)


def test_adam_scale_argument_on_cpu():
    """CPU tensors take the torch formula (the gloo tests of the sharding logic); ``scale`` multiplies the gradient."""
    x1, x2 = torch.ones(5), torch.ones(5)
    g = torch.tensor([0.1, -0.2, 0.3, 0.0, 1.0])
    o1, o2 = inf.Adam(1e-2), inf.Adam(1e-2)
    for _ in range(3):
        o1.step(x1, g * -0.5)
        o2.step(x2, g, -0.5)
    assert torch.allclose(x1, x2) and o1.t == o2.t == 3


# ---- HMC driver: trajectory-length adaptation (tfe.mcmc.GradientBasedTrajectoryLengthAdaptation, tf/inference.py:150-154) ----
class _ToyModel:
    """A closed-form log-density behind the ForwardProbModel surface the drivers use (the lens likelihood needs a GPU)."""
    device = torch.device("cpu")
    include_pixels, include_positions, n_position = True, False, 0.0

    def __init__(self, sigma):
        self.sigma = torch.as_tensor(sigma, dtype=torch.float32)

    def init_centroids(self, bs):
        return None

    def log_prob_and_grad(self, simulator, z):
        lp = -0.5 * ((z / self.sigma) ** 2).sum(-1)
        return lp, torch.zeros_like(lp), -z / self.sigma ** 2


def _hmc(monkeypatch, sigma, **kw):
    monkeypatch.setattr(inf, "LensSimulator", lambda *a, **k: None)
    d = len(sigma)
    seq = inf.ModellingSequence(None, _ToyModel(sigma), None)
    return seq.HMC((torch.zeros(d), torch.diag(torch.as_tensor(sigma, dtype=torch.float32))), **kw)


def test_halton_sequence():
    assert [inf._halton2(i) for i in range(1, 8)] == [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875]


def test_hmc_trajectory_length_adapts_to_the_known_optimum(monkeypatch):
    """Standard normal in the preconditioned coordinates: ChEES per unit mass is d sin^2(t), so with lengths h T, h uniform on
    (0, 1), the criterion is maximal where tan 2T = 2T, T = 2.2467 -- in the limit of small steps; the integration time is a
    whole number of steps, ceil(h T / eps) eps, so the adapted T approaches that value from below as eps shrinks (measured:
    1.47 at eps = 0.92, 1.90 at 0.61, 2.00 at 0.36, 2.17 at 0.18).  Starting from T = eps * L = 0.2 the adaptation must get
    there (the step-size adaptation runs beside it), keep the acceptance at the target, and the chain must sample the target."""
    sigma = [0.5, 1.0, 2.0, 4.0, 1.0, 1.0, 3.0, 0.7, 1.5, 1.0]
    samples, st = _hmc(monkeypatch, sigma, init_eps=0.1, init_l=2, n_hmc=256, num_burnin_steps=600, num_results=200,
                       max_leapfrog_steps=200, seed=11, target_accept=0.97)
    T = st["max_trajectory_length"]
    assert 1.8 < T < 2.4, T
    assert 0.93 < sum(st["accept"][-200:]) / 200 < 0.995
    assert samples.shape == (200, 256, 10)
    sd = samples.reshape(-1, 10).std(0)
    assert torch.allclose(sd, torch.tensor(sigma), rtol=0.1)
    # the jitter spreads the number of leapfrog steps between 1 and ceil(T / eps)
    late = st["num_leapfrog_steps"][-200:]
    assert min(late) >= 1 and max(late) <= math.ceil(T / st["step_size"]) and len(set(late)) > 3


def test_hmc_honours_max_leapfrog_steps(monkeypatch):
    sigma = [1.0] * 6
    samples, st = _hmc(monkeypatch, sigma, init_eps=0.05, init_l=9, n_hmc=64, num_burnin_steps=60, num_results=10,
                       max_leapfrog_steps=4, seed=2)
    assert max(st["num_leapfrog_steps"]) <= 4 and min(st["num_leapfrog_steps"]) >= 1
    assert st["max_trajectory_length"] <= 4 * st["step_size"] * 1.5  # kept near the cap eps * max_leapfrog_steps
    # adaptation stops after int(0.8 * burn-in) transitions (tf/inference.py:140): the step size is frozen afterwards
    s2, st2 = _hmc(monkeypatch, sigma, init_eps=0.05, init_l=2, n_hmc=64, num_burnin_steps=0, num_results=5, seed=2)
    assert st2["step_size"] == pytest.approx(0.05) and set(st2["num_leapfrog_steps"]) <= {1, 2}


# ---- SMC on a conjugate problem: the evidence and the posterior are known ----------------------------------------------------------
class _ConjugateModel:
    """Prior N(0, 2^2 I_4), likelihood N(y | z, 0.3^2 I) (normalised: the evidence is log N(y; 0, (4 + 0.09) I)), behind the two
    entry points ``SMC`` uses."""
    device = torch.device("cpu")
    include_pixels, include_positions, n_position = True, False, 0.0
    s0, s = 2.0, 0.3
    y = torch.tensor([1.0, -0.5, 2.5, 0.2])

    def init_centroids(self, bs):
        return None

    def log_prior(self, z):
        return -0.5 * (z / self.s0).pow(2).sum(-1) - 4 * math.log(self.s0) - 2 * math.log(2 * math.pi)

    def term_log_prob_and_grad(self, simulator, z, name):
        assert name == "pixels"
        like = -0.5 * ((self.y - z) / self.s).pow(2).sum(-1) - 4 * math.log(self.s) - 2 * math.log(2 * math.pi)
        return self.log_prior(z) + like, like, -z / self.s0 ** 2 + (self.y - z) / self.s ** 2


def test_smc_evidence_and_posterior_on_a_conjugate_problem(monkeypatch):
    """The adaptive tempered SMC against the closed form: mean log-evidence of 8 ensembles within 5 standard errors of
    log N(y; 0, 4.09 I), posterior means within 5 sd / sqrt(N E), posterior sd within 5 %."""
    monkeypatch.setattr(inf, "LensSimulator", lambda *a, **k: None)
    pm = _ConjugateModel()
    N, E = 512, 8
    start = pm.s0 * torch.randn(4 * N * E, 4, generator=torch.Generator().manual_seed(21))
    samples, info = inf.ModellingSequence(None, pm, None).SMC(
        start=start, num_particles=N, num_ensembles=E, num_leapfrog_steps=5, post_sampling_steps=0, max_sampling_per_stage=4,
        target="pixels", auxiliar="none")
    assert samples.shape == (N, E, 4) and info["stages"][-1]["beta"] == [1.0] * E
    var = pm.s0 ** 2 + pm.s ** 2
    want = float(-0.5 * (pm.y ** 2).sum() / var - 2 * math.log(2 * math.pi * var))
    lz = info["log_evidence"].double()
    se = float(lz.std() / math.sqrt(E))
    print(f"log evidence {float(lz.mean()):.4f} vs {want:.4f}: {abs(float(lz.mean()) - want) / se:.2f} se, ensemble sd {float(lz.std()):.3f}")
    assert abs(float(lz.mean()) - want) <= 5 * se
    post_sd = math.sqrt(pm.s0 ** 2 * pm.s ** 2 / var)
    post_mean = pm.y * pm.s0 ** 2 / var
    flat = samples.reshape(-1, 4).double()
    assert float((flat.mean(0) - post_mean).abs().max()) <= 5 * post_sd / math.sqrt(N * E)
    assert float((flat.std(0) / post_sd - 1).abs().max()) <= 0.05


# ---- the float64 restatements of tests/inference_cases.py against the loops' torch branches, and what their gates reject -----------
def _transition_runs(d, init_eps, seed, mutate=None):
    """the restatement in float64 and float32 on the draws of a CPU generator, for q off the target"""
    m, C = IC.gaussian_target(d)
    pm = IC.GaussModel(m, C)
    mean = torch.as_tensor(m + 0.5, dtype=torch.float32)
    L = torch.as_tensor(0.8 * np.linalg.cholesky(C), dtype=torch.float32)
    n, K = 512, 4
    gen = inf.gdist.rank_generator(seed, 0)
    draws = [torch.randn(n, d, generator=gen).numpy()]
    for _ in range(K):
        draws += [torch.randn(n, d, generator=gen).numpy(), torch.rand(n, generator=gen).numpy()]
    run = lambda T, mut=None: IC.hmc_transitions64(pm.vg(T), mean.numpy(), L.numpy(), init_eps, 3, n, K, 10, draws, dtype=T, mutate=mut)
    return pm, (mean, L), run(np.float64), run(np.float32), (run(np.float32, mutate) if mutate else None)


@pytest.mark.parametrize("d,init_eps", [(5, 1.1), (132, 0.55)])
def test_hmc_restatement_equals_the_torch_branch(monkeypatch, d, init_eps):
    """``hmc_transitions64`` in float32 and the loop's torch branch on the same CPU generator walk the same chains: to 4 x the
    float32 restatement's own deviation from float64, over the chains whose decisions float32 can call."""
    monkeypatch.setattr(inf, "LensSimulator", lambda *a, **k: None)
    pm, q, r64, r32, _ = _transition_runs(d, init_eps, 9)
    samples, st = inf.ModellingSequence(None, pm, None).HMC(q, init_eps=init_eps, init_l=3, n_hmc=512, num_burnin_steps=0, num_results=4,
                                                             max_leapfrog_steps=10, seed=9)
    rep = IC.transitions_gate(samples.numpy(), r64, r32)
    print(d, rep, "accept", st["accept"])
    assert 0.5 < sum(st["accept"]) / 4 < 0.95  # rejections are exercised
    assert rep["err"] <= 4 * rep["yard_z"] and rep["left_out"] <= 0.01
    assert st["num_leapfrog_steps"] == [2, 1, 3, 1]


@pytest.mark.parametrize("full_rank", [True, False])
def test_svi_buffer64_equals_svi_step_in_float64(full_rank):
    mu, lp, eps, logp, G = (torch.as_tensor(a).double() for a in IC.svi_case(65, 13, full_rank, seed=3))
    got = inf.svi_step_buffer(mu, lp, None, 65, value_and_grad_fn=lambda z: (logp, G), full_rank=full_rank, eps=eps, reduce=False)
    want = IC.svi_buffer64(lp.numpy(), eps.numpy(), logp.numpy(), G.numpy(), full_rank, 1e-6)
    assert np.allclose(got.numpy(), want, rtol=1e-12, atol=1e-9 * np.abs(want).max())
    z = IC.svi_sample64(mu.numpy(), lp.numpy(), eps.numpy(), full_rank, 1e-6)
    L = inf.tril_unpack(lp, 13) if full_rank else torch.diag(torch.exp(lp))
    assert np.allclose(z, (mu + eps @ L.T).numpy(), rtol=1e-13, atol=1e-13)


def _over(a, b, bound):
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / bound).max())


@pytest.mark.parametrize("mutation", ["no_c2", "no_shift", "row_start", "upper", "no_last_kick", "kick_sign"])
def test_gates_hold_the_float32_restatement_and_reject_a_mutant(mutation):
    """Each gate of the GPU tests, applied on the CPU: the float32 restatement passes it, and one plausible wrong variant of that
    restatement does not.  (No wrong kernel is put on a GPU.)"""
    f = np.float32
    if mutation == "no_c2":
        x, m, v, g = IC.adam_case(257)
        for t in (1, 2, 5000):
            want, b = IC.adam64(x, m, v, g, IC.HYPER, t), IC.adam_bound(x, m, v, g, IC.HYPER, t)
            assert _over(IC.adam64(x, m, v, g, IC.HYPER, t, f)[0], want[0], b[0]) <= 1
            assert _over(IC.adam64(x, m, v, g, IC.HYPER, t, f, mutation)[0], want[0], b[0]) > 1
    elif mutation == "no_shift":
        mu, lp, eps, logp, G = IC.svi_case(65, 13, True)
        want, b = IC.svi_buffer64(lp, eps, logp, G, True, 1e-6), IC.svi_buffer_bound(lp, eps, logp, G, True, 1e-6)
        assert _over(IC.svi_buffer64(lp, eps, logp, G, True, 1e-6, f), want, b) <= 1
        assert _over(IC.svi_buffer64(lp, eps, logp, G, True, 1e-6, f, mutation), want, b) > 1
    elif mutation == "row_start":
        lp, eps, logp, G, jj, kk, exact = IC.index_map_case(300)
        off = jj != kk
        assert all(IC.tril_jk32(t) == (j, k) for t, (j, k) in enumerate(zip(jj.tolist(), kk.tolist())))
        assert np.array_equal(IC.svi_buffer64(lp, eps, logp, G, True, 1e-6, f)[301:][off], exact[off])
        assert not np.array_equal(IC.svi_buffer64(lp, eps, logp, G, True, 1e-6, f, mutation)[301:][off], exact[off])
    elif mutation == "upper":
        c = IC.accept_case(8, 13)
        nan_up = np.where(np.triu(np.ones((13, 13), dtype=bool), 1), np.nan, c["L"]).astype(f)
        want = IC.accept64(**c, dtype=f)
        got, bad = IC.accept64(**{**c, "L": nan_up}, dtype=f), IC.accept64(**{**c, "L": nan_up}, dtype=f, mutate=mutation)
        assert all(np.array_equal(got[k], want[k]) for k in ("acc_prob", "take", "z", "g", "lp"))
        assert not np.array_equal(bad["acc_prob"], want["acc_prob"])
    elif mutation == "no_last_kick":
        _, _, r64, r32, bad = _transition_runs(5, 1.1, 9, mutation)
        ok = IC.transitions_gate(r32[0], r64, r32)
        rep = IC.transitions_gate(bad[0], r64, r32)
        assert ok["err"] <= 4 * ok["yard_z"] and ok["left_out"] <= 0.01
        assert rep["err"] > 4 * rep["yard_z"]
    else:
        p, g, k, z, S, e = IC.kick_case(3, 129)
        want, b = IC.kick_drift64(p, g, k, z, S, e), IC.kick_drift_bound(p, g, k, z, S, e)
        assert max(_over(a, w, bb) for a, w, bb in zip(IC.kick_drift64(p, g, k, z, S, e, f), want, b)) <= 1
        assert min(_over(a, w, bb) for a, w, bb in zip(IC.kick_drift64(p, g, k, z, S, e, f, mutation), want, b)) > 1
