#!/usr/bin/env python3
"""Event-timed cost of the fused ``log_prob_and_grad`` of the point-image term (no pixels): an EPL + Shear lens with one quad of
observed images, the image positions alone and, where the build has the term, with the time delays of the quad added.

    python3 tools/point_term_step_time.py                 # batch 1024, stream launches and graph replay
    python3 tools/point_term_step_time.py --batch 4096
    python3 tools/point_term_step_time.py --planes        # K = 2: an SIS at z = 1 behind the lens at z = 0.5, the quad at z = 2

Method: per variant 20 warm-up calls, then ``--calls`` back-to-back calls between two HIP events; ``--runs`` such runs, the
variants alternating; the median, minimum and maximum of the runs in microseconds per call.  The script needs nothing but the
package, so the same file times an older build from that build's checkout (a build without ``centroids_time_delays`` reports the
positions alone): the figures of INTEGRATION.md, "time delays as a likelihood", come from running it in turn on the parent
commit's build and on this one.  ``--planes``: the same on two lens planes (``centroids_redshifts``; the delays through
``time_delay_h0`` where the build has it): the figures of "time delays on lens planes"."""
import argparse
import inspect
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--planes", action="store_true", help="two lens planes: an SIS on a plane of its own behind the EPL + Shear")
    args = ap.parse_args()
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import ForwardProbModel, PhysicalModel
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.simulator import LensSimulator, SimulatorConfig
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([
        J(dict(theta_E=tfd.LogNormal(float(np.log(1.1)), 0.03), gamma=tfd.LogNormal(float(np.log(2.1)), 0.03), e1=tfd.Normal(0.1, 0.01),
               e2=tfd.Normal(-0.05, 0.01), center_x=tfd.Normal(0.037, 0.01), center_y=tfd.Normal(-0.063, 0.01))),
        J(dict(gamma1=tfd.Normal(0.03, 0.01), gamma2=tfd.Normal(-0.02, 0.01)))])))
    f32 = lambda *v: np.asarray(v, dtype=np.float32)
    quad = dict(centroids_x=[f32(1.2, -1.0, 0.2, -0.3)], centroids_y=[f32(0.2, 0.3, -1.1, 1.0)], centroids_errors_x=[np.float32(0.01)],
                centroids_errors_y=[np.float32(0.0125)])
    delays = dict(centroids_time_delays=[f32(-210.0, -228.0, -215.0, -219.0)], centroids_time_delays_errors=[np.float32(1.0)])
    keywords = inspect.signature(ForwardProbModel.__init__).parameters
    if args.planes:
        from gigalens_amd.cosmology import MultiPlane
        from gigalens_amd.profiles.mass.sis import SIS
        prior = J(dict(lens_mass=S(list(prior.model["lens_mass"].model) + [
            J(dict(theta_E=tfd.LogNormal(float(np.log(0.05)), 0.03), center_x=tfd.Normal(0.937, 0.01), center_y=tfd.Normal(-0.663, 0.01)))])))
        quad = dict(quad, centroids_redshifts=[2.0])
        variants = {"positions": quad}
        if "time_delay_h0" in keywords:
            variants["positions+delays"] = dict(quad, **delays, time_delay_h0="profile")
        phys = PhysicalModel([EPL(), Shear(), SIS()], [], [], multiplane=MultiPlane([0.5, 0.5, 1.0], [], 3.0))
    else:
        variants = {"positions": quad}
        if "centroids_time_delays" in keywords:
            variants["positions+delays"] = dict(quad, **delays)
        phys = PhysicalModel([EPL(), Shear()], [], [])
    runs = {}
    for name, kw in variants.items():
        sim = LensSimulator(phys, SimulatorConfig(delta_pix=0.1, num_pix=8), bs=args.batch)
        pm = ForwardProbModel(prior, include_pixels=False, **kw)
        z = pm.bij.inverse(pm.prior.sample(args.batch, seed=1)).to(sim.device).contiguous()
        runs[name] = (sim, pm, z)

    def timed(sim, pm, z, graph):
        for _ in range(20):
            pm.log_prob_and_grad(sim, z, graph=graph)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            pm.log_prob_and_grad(sim, z, graph=graph)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3

    for graph in (False, True):
        res = {k: [] for k in runs}
        for _ in range(args.runs):
            for k, (sim, pm, z) in runs.items():
                res[k].append(timed(sim, pm, z, graph))
        for k, v in res.items():
            v = np.asarray(v)
            print(f"batch {args.batch}, {'graph replay' if graph else 'stream launches'}, {k}: median {np.median(v):.2f} us per call "
                  f"(min {v.min():.2f}, max {v.max():.2f}; {args.runs} runs of {args.calls} calls)", flush=True)


if __name__ == "__main__":
    main()
