"""The native MAP / SVI / HMC loops of ``gigalens_amd/inference.py`` on a target with known answers: a correlated Gaussian N(m, C)
in closed form behind the surface the loops use, float32 on the GPU, so that every launch the loops issue -- first half kick, the
order of kick and drift, the last half kick inside the accept kernel, the in-place selection, the surrogate's two kernels around
the gradient call, the fused Adam update -- is the one under test."""
import math

import numpy as np
import pytest
import torch

from gigalens_amd import _native
from gigalens_amd import inference as inf
from tests import inference_cases as IC

pytestmark = pytest.mark.gpu


def _sequence(monkeypatch, d):
    monkeypatch.setattr(inf, "LensSimulator", lambda *a, **k: None)
    m, C = IC.gaussian_target(d)
    pm = IC.GaussModel(m, C, "cuda")
    calls = {"accept": 0, "kick_drift": 0, "svi_grad": 0, "adam": 0}
    for name, key in (("hmc_accept", "accept"), ("hmc_kick_drift", "kick_drift"), ("svi_grad", "svi_grad"), ("adam_update", "adam")):
        def counted(*a, _f=getattr(_native, name), _k=key, **k):
            calls[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(_native, name, counted)
    return pm, inf.ModellingSequence(None, pm, None), m, C, calls


@pytest.mark.parametrize("d,init_eps", [(5, 1.1), (132, 0.55)])
def test_hmc_transitions_against_float64_on_identical_draws(monkeypatch, d, init_eps):
    """Four transitions of 512 chains from a surrogate off the target (mean + 0.5, 0.8 chol C), adaptation off, against
    ``hmc_transitions64`` fed the draws of the same device generator.  Gate: every chain not left out agrees to 4 x the float32 run
    of the restatement on those draws; a chain is left out from the first transition where its float64 margin |log u - log_acc| is
    below 4 x the float32 run's log_acc deviation, at most 1 % of them."""
    pm, seq, m, C, calls = _sequence(monkeypatch, d)
    n, K = 512, 4
    mean = torch.as_tensor(m + 0.5, dtype=torch.float32)
    L = torch.as_tensor(0.8 * np.linalg.cholesky(C), dtype=torch.float32)
    samples, st = seq.HMC((mean, L), num_burnin_steps=0, num_results=K, init_eps=init_eps, init_l=3, max_leapfrog_steps=10, n_hmc=n,
                          seed=9)
    assert calls["accept"] == K and calls["kick_drift"] == sum(st["num_leapfrog_steps"])  # the native path, one launch per drift
    assert st["num_leapfrog_steps"] == [2, 1, 3, 1]
    gen = inf.gdist.rank_generator(9, 0, device="cuda")
    draws = [torch.randn(n, d, generator=gen, device="cuda").cpu().numpy()]
    for _ in range(K):
        draws += [torch.randn(n, d, generator=gen, device="cuda").cpu().numpy(), torch.rand(n, generator=gen, device="cuda").cpu().numpy()]
    run = lambda T: IC.hmc_transitions64(pm.vg(T), mean.numpy(), L.numpy(), init_eps, 3, n, K, 10, draws, dtype=T)
    r64, r32 = run(np.float64), run(np.float32)
    rep = IC.transitions_gate(samples.cpu().numpy(), r64, r32)
    print(f"LOOP hmc-transitions-d{d} {rep} ratio-to-gate {rep['err'] / (4 * rep['yard_z']):.3f} accept {np.mean(st['accept']):.3f}")
    assert 0.5 < np.mean(st["accept"]) < 0.95  # rejections are exercised
    assert rep["left_out"] <= 0.01
    assert rep["err"] <= 4 * rep["yard_z"]


def test_hmc_reaches_the_stationary_distribution_from_a_wrong_start(monkeypatch):
    """1024 chains started 3 sigma off with half the scale, 100 adapted transitions: the last state of each chain is one
    independent draw of N(m, C).  Every coordinate mean within 5 sigma_j / sqrt(n), every covariance entry within 5 of its own
    standard errors sqrt((C_jk^2 + C_jj C_kk) / (n - 1)).  A loop that never moves leaves the mean 96 standard errors off."""
    d, n = 5, 1024
    pm, seq, m, C, calls = _sequence(monkeypatch, d)
    sd = np.sqrt(np.diagonal(C))
    q = (torch.as_tensor(m + 3 * sd, dtype=torch.float32), torch.as_tensor(0.5 * np.diag(sd), dtype=torch.float32))
    samples, st = seq.HMC(q, n_hmc=n, num_burnin_steps=100, num_results=1, max_leapfrog_steps=10)
    assert samples.shape == (1, n, d) and calls["accept"] == 101
    z_mean, z_cov = IC.moment_z_scores(samples[0].cpu().numpy(), m, C)
    print(f"LOOP hmc-stationary worst z-score mean {z_mean:.2f} covariance {z_cov:.2f} accept {np.mean(st['accept'][-20:]):.3f}")
    assert z_mean <= 5 and z_cov <= 5


@pytest.mark.parametrize("full_rank", [True, False])
def test_svi_reaches_the_target(monkeypatch, full_rank):
    """800 steps of the native SVI loop from m + sigma, scale 0.3.  Full rank: the optimum is q = N(m, C), loss -log Z; mean field:
    the optimum has mean m and variances 1 / (C^-1)_jj."""
    d = 5
    pm, seq, m, C, calls = _sequence(monkeypatch, d)
    sd = np.sqrt(np.diagonal(C))
    (mean, L), losses = seq.SVI(inf.Adam(lambda t: 0.05 * min(1.0, 200.0 / t)), torch.as_tensor(m + sd, dtype=torch.float32),
                                n_vi=256, init_scales=0.3, num_steps=800, full_rank=full_rank)
    assert calls["svi_grad"] == 800 and calls["adam"] == 800
    mean, L = mean.cpu().double().numpy(), L.cpu().double().numpy()
    e_mean = float((np.abs(mean - m) / sd).max())
    if full_rank:
        e_cov = float(np.abs(L @ L.T - C).max() / np.abs(C).max())
        e_loss = abs(float(np.mean(losses[-50:])) + pm.log_Z)
        print(f"LOOP svi-full mean {e_mean:.4f} sigma, covariance {e_cov:.4f} of max|C|, loss - (-log Z) {e_loss:.4f}")
        assert e_mean <= 0.1 and e_cov <= 0.1 and e_loss <= 0.05
    else:
        want = 1.0 / np.diagonal(np.linalg.inv(C))
        e_var = float((np.abs(np.diagonal(L) ** 2 - want) / want).max())
        print(f"LOOP svi-diag mean {e_mean:.4f} sigma, variances {e_var:.4f}")
        assert np.array_equal(L, np.diag(np.diagonal(L)))
        assert e_mean <= 0.1 and e_var <= 0.1
