"""``log_prob_and_grad(..., graph=True)`` when the simulator's native model is used for other things between two replays: the
graph's entry owns the workspace it captured and is captured again once anything was handed to the native model since (another
``ForwardProbModel``'s prior or image positions).  Every result is compared bit for bit with stream launches on a simulator of its
own, and ``simulator._lp_captures`` says how often a capture happened."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _clone(outs):
    return [t.clone() for t in outs]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def c1():
    """BASELINE configs[0]'s model (one SIE + Sersic) on a 32 x 32 grid: the workload, an observation, and a second prior of the
    same structure with other parameters."""
    from gigalens_amd import prior as tfd
    from gigalens_amd import workloads
    from gigalens_amd.simulator import LensSimulator
    wl = workloads.make("C1", num_pix=32, batch=3)
    obs = workloads.synthetic_observation(wl, LensSimulator)[0].cpu().numpy()
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    other = J(dict(
        lens_mass=S([J(dict(theta_E=tfd.LogNormal(math.log(1.1), 0.3), e1=tfd.Normal(0.05, 0.15), e2=tfd.Normal(-0.05, 0.15),
                            center_x=tfd.Normal(0.02, 0.08), center_y=tfd.Normal(-0.02, 0.08)))]),
        source_light=S([J(dict(R_sersic=tfd.LogNormal(math.log(0.3), 0.2), n_sersic=tfd.Uniform(0.5, 4), center_x=tfd.Normal(0, 0.3),
                               center_y=tfd.Normal(0, 0.3), Ie=tfd.LogNormal(math.log(120.0), 0.4)))])))
    return wl, obs, other


def test_two_shapes_and_calls_between_them_replay_without_a_new_capture(c1):
    """Graphs at B = 3 and B = 2, then a stream-launch call and a render at B = 1 (each takes the native model's one workspace slot),
    then both graphs again: every replay equals the stream launches, and nothing was captured a second time -- the entries hold
    their workspaces, and nothing was handed to the native model."""
    from gigalens_amd.model import ForwardProbModel
    from gigalens_amd.simulator import LensSimulator
    wl, obs, _ = c1
    pm = ForwardProbModel(wl.prior, obs, wl.background_rms, wl.exp_time, include_positions=False)
    fresh = LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    z = {(B, seed): pm.bij.inverse(wl.prior.sample(B, seed=seed)).to("cuda").contiguous() for B in (3, 2, 1) for seed in (1, 2)}
    want = {k: _clone(pm.log_prob_and_grad(fresh, v)) for k, v in z.items()}
    packed = fresh.pack(wl.prior.sample(wl.batch, seed=3))[:1].contiguous()
    image = fresh.simulate(packed).clone()

    sim = LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    assert sim._lp_captures == 0
    assert _same(pm.log_prob_and_grad(sim, z[3, 1], graph=True), want[3, 1])
    assert _same(pm.log_prob_and_grad(sim, z[2, 1], graph=True), want[2, 1])
    assert sim._lp_captures == 2
    assert _same(pm.log_prob_and_grad(sim, z[1, 1]), want[1, 1])
    assert torch.equal(sim.simulate(packed), image)
    for seed in (2, 1):
        assert _same(pm.log_prob_and_grad(sim, z[3, seed], graph=True), want[3, seed])
        assert _same(pm.log_prob_and_grad(sim, z[2, seed], graph=True), want[2, seed])
    assert _same(pm.log_prob_and_grad(sim, z[1, 2]), want[1, 2])
    assert sim._lp_captures == 2


def _a_second_model_between_two_replays(a, b, phys, cfg, z):
    """Model ``a`` with ``graph=True``, model ``b`` with stream launches on the same simulator, ``a`` with ``graph=True`` again."""
    from gigalens_amd.simulator import LensSimulator
    fresh_a, fresh_b = LensSimulator(phys, cfg, bs=z[0].shape[0]), LensSimulator(phys, cfg, bs=z[0].shape[0])
    want_a = [_clone(a.log_prob_and_grad(fresh_a, v)) for v in z]
    want_b = _clone(b.log_prob_and_grad(fresh_b, z[1]))
    assert not torch.equal(want_a[1][0], want_b[0])  # (the two models do differ)

    sim = LensSimulator(phys, cfg, bs=z[0].shape[0])
    assert _same(a.log_prob_and_grad(sim, z[0], graph=True), want_a[0])
    assert sim._lp_captures == 1
    assert _same(b.log_prob_and_grad(sim, z[1]), want_b)
    assert _same(a.log_prob_and_grad(sim, z[1], graph=True), want_a[1])  # a's, not b's: captured again on a's own tables
    assert sim._lp_captures == 2
    assert _same(a.log_prob_and_grad(sim, z[0], graph=True), want_a[0])  # and replayed from then on
    assert sim._lp_captures == 2


def test_a_second_prior_on_the_simulator_makes_the_graph_capture_again(c1):
    from gigalens_amd.model import ForwardProbModel
    wl, obs, other = c1
    a = ForwardProbModel(wl.prior, obs, wl.background_rms, wl.exp_time, include_positions=False)
    b = ForwardProbModel(other, obs, wl.background_rms, wl.exp_time, include_positions=False)
    z = [a.bij.inverse(wl.prior.sample(wl.batch, seed=seed)).to("cuda").contiguous() for seed in (1, 2)]
    _a_second_model_between_two_replays(a, b, wl.phys_model, wl.sim_config, z)


def test_a_second_set_of_image_positions_makes_the_graph_capture_again():
    """Pixels and image positions (the families of tests/test_gpu_positions.py); the second model has other ``centroids_x``."""
    from gigalens_amd import workloads
    from gigalens_amd.model import ForwardProbModel
    from gigalens_amd.simulator import LensSimulator
    from tests import test_gpu_positions as TP
    phys, prior, cfg, B = TP._setup("epl")
    obs = workloads.synthetic_observation(workloads.Workload("POS", phys, prior, cfg, B), LensSimulator)[0].cpu().numpy()
    kw = dict(centroids_y=TP.CY, centroids_errors_x=TP.EX, centroids_errors_y=TP.EY)
    a = ForwardProbModel(prior, obs, 0.2, 100.0, centroids_x=TP.CX, **kw)
    b = ForwardProbModel(prior, obs, 0.2, 100.0, centroids_x=[x + 0.02 for x in TP.CX], **kw)
    assert a._terms() == b._terms() == 3
    z = [a.bij.inverse(prior.sample(B, seed=seed)).to("cuda").contiguous() for seed in (2, 3)]
    _a_second_model_between_two_replays(a, b, phys, cfg, z)
