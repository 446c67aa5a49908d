"""Select-free whole tiles of the pair kernels (csrc/gl_pair.hip.h, csrc/gl_vec.hip.h FAST).

Whole unmasked tiles run the profile bodies without the selects, clamps and floors that only act on singular inputs, behind one
wave-uniform guard; a wave whose guard fires hands the tile to the careful body.  For every input the results must be BITWISE
those of the careful body on every tile, which GIGALENS_HIP_CAREFUL_TILES=1 (read at model creation) forces:

  * regular prior draws, with and without an error map, over the compositions the pair kernels serve;
  * inputs that are singular by construction -- a pixel exactly on the EPL's centre, a pixel exactly on a lens light's centre,
    a Sersic whose (R / R_sersic)^(1/n) overflows -- where the select-free body alone would produce inf x 0 = NaN: equality with
    the careful path, finite where it is finite, proves that the fallback ran.  The log-likelihood is held to the float64 oracle
    there too (at the overflowing Sersic the oracle's own log-likelihood is NaN: agreement there is NaN on both sides);
    gradients at these points only to the careful path (the reference's own gradient is NaN at some of them).

Sizes: batch 8 (the cost-ordered dispatch runs), 32 x 32 (1 024 pixels: whole pair tiles only) and 40 x 40 (1 600 pixels: whole
tiles and a ragged 64-pixel one)."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_parity import LL_RTOL, gl  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH = 8
KNOB = "GIGALENS_HIP_CAREFUL_TILES"


def _models(gl):
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    W = gl.workloads
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    sie = lambda: J(dict(theta_E=tfd.LogNormal(math.log(1.0), 0.2), e1=tfd.Normal(0, 0.1), e2=tfd.Normal(0, 0.1),
                         center_x=tfd.Normal(0, 0.05), center_y=tfd.Normal(0, 0.05)))
    src_ell = lambda: J(dict(R_sersic=tfd.LogNormal(math.log(0.25), 0.15), n_sersic=tfd.Uniform(0.5, 4), e1=tfd.Normal(0, 0.1),
                             e2=tfd.Normal(0, 0.1), center_x=tfd.Normal(0, 0.25), center_y=tfd.Normal(0, 0.25),
                             Ie=tfd.LogNormal(math.log(150.0), 0.5)))
    lens_light = lambda: J(dict(R_sersic=tfd.LogNormal(math.log(0.8), 0.1), n_sersic=tfd.Uniform(2, 4), center_x=tfd.Normal(0, 0.05),
                                center_y=tfd.Normal(0, 0.05), Ie=tfd.LogNormal(math.log(30.0), 0.3)))
    return {
        "EPL+Shear|Sersic": (PhysicalModel([EPL(), Shear()], [], [Sersic()]),
                             J(dict(lens_mass=S([W._epl_prior(), W._shear_prior()]), source_light=S([W._sersic_src_prior()])))),
        "EPL+Shear|SersicEllipse": (PhysicalModel([EPL(), Shear()], [], [SersicEllipse()]),
                                    J(dict(lens_mass=S([W._epl_prior(), W._shear_prior()]), source_light=S([src_ell()])))),
        "EPL+Shear|Sersic|Sersic": (PhysicalModel([EPL(), Shear()], [Sersic()], [Sersic()]),
                                    J(dict(lens_mass=S([W._epl_prior(), W._shear_prior()]), lens_light=S([lens_light()]),
                                           source_light=S([W._sersic_src_prior()])))),
        "SIE|Sersic": (PhysicalModel([SIE()], [], [Sersic()]),
                       J(dict(lens_mass=S([sie()]), source_light=S([W._sersic_src_prior()])))),
        "SIE+Shear|Sersic|Sersic": (PhysicalModel([SIE(), Shear()], [Sersic()], [Sersic()]),
                                    J(dict(lens_mass=S([sie(), W._shear_prior()]), lens_light=S([lens_light()]),
                                           source_light=S([W._sersic_src_prior()])))),
    }


def _workload(gl, name, num_pix):
    from gigalens_amd.simulator import SimulatorConfig
    phys, prior = _models(gl)[name]
    return gl.workloads.Workload(name, phys, prior, SimulatorConfig(delta_pix=0.065, num_pix=num_pix), BATCH)


def _column(phys, group, index, name):
    """Column of a parameter in the packed rows (the walk of helpers.struct_from_packed)."""
    k = 0
    for g, profs in zip(H.GROUPS, (phys.lenses, phys.lens_light, phys.source_light)):
        for i, p in enumerate(profs):
            for n in (p._native_params() if hasattr(p, "_native_params") else p.params):
                if (g, i, n) == (group, index, name):
                    return k
                k += 1
    raise KeyError((group, index, name))


def _outputs(gl, wl, obs, err, packed, cot, z=None):
    """Everything the pair kernels produce, from a FRESH simulator (the knob is read when its native model is created):
    log-likelihood, chi^2 and gradient from packed rows; the image and its VJP; and, with `z`, the fused log_prob_and_grad."""
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    out = [t.clone() for t in sim._model.loglike(packed, obs, err, None, wl.background_rms, wl.exp_time, True)]
    assert "gl_pair_kernel" in sim._model.last_main_kernel(), sim._model.last_main_kernel()
    out.append(sim.simulate(packed).clone())
    out.append(sim.simulate_vjp(packed, cot).clone())
    if z is not None:
        pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time,
                                 error_map=None if err is None else err.cpu().numpy(), include_positions=False)
        out += [t.clone() for t in pm.log_prob_and_grad(sim, z)]
    torch.cuda.synchronize()
    return out


def _both(gl, monkeypatch, wl, obs, err, packed, cot, z=None):
    monkeypatch.delenv(KNOB, raising=False)
    default = _outputs(gl, wl, obs, err, packed, cot, z)
    monkeypatch.setenv(KNOB, "1")
    careful = _outputs(gl, wl, obs, err, packed, cot, z)
    monkeypatch.delenv(KNOB)
    return default, careful


def _equal_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))  # NaNs included, signed zeros told apart


def _cotangent(n, seed=5):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn((BATCH, n, n), generator=g, dtype=torch.float32).to("cuda")


@pytest.mark.parametrize("with_err", [False, True])
@pytest.mark.parametrize("num_pix", [32, 40])
@pytest.mark.parametrize("name", ["EPL+Shear|Sersic", "EPL+Shear|SersicEllipse", "EPL+Shear|Sersic|Sersic", "SIE|Sersic",
                                  "SIE+Shear|Sersic|Sersic"])
def test_default_equals_careful_bitwise_on_regular_draws(gl, monkeypatch, name, num_pix, with_err):
    wl = _workload(gl, name, num_pix)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    err = (0.2 + 0.05 * obs.abs()).contiguous() if with_err else None
    x = wl.prior.sample(BATCH, seed=3)
    sim0 = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=BATCH)
    packed = sim0.pack(x)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    z = pm.bij.inverse(x).to("cuda")
    default, careful = _both(gl, monkeypatch, wl, obs, err, packed, _cotangent(num_pix), z)
    assert len(default) == len(careful) == 8
    for a, b in zip(default, careful):
        assert torch.isfinite(a).all()
        assert _equal_bits(a, b)


def _singular_case(gl, case, num_pix):
    """(workload, packed rows, host-side proof that the input is singular) for one of the three constructions."""
    name = {"epl_centre_on_pixel": "EPL+Shear|Sersic", "lens_light_centre_on_pixel": "EPL+Shear|Sersic|Sersic",
            "sersic_overflow": "EPL+Shear|Sersic"}[case]
    wl = _workload(gl, name, num_pix)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=BATCH)
    packed = H.sample_packed(wl, sim, seed=4)
    phys = wl.phys_model
    gx, gy = sim.img_X.cpu().numpy(), sim.img_Y.cpu().numpy()
    assert gx.dtype == np.float32 and gx.shape == (num_pix * num_pix,)
    if case in ("epl_centre_on_pixel", "lens_light_centre_on_pixel"):
        j = (num_pix // 2) * num_pix + num_pix // 2 + 3  # a pixel of the tile [512, 1024): whole at both sizes
        assert 512 <= j < 1024
        group = ("lens_mass", 0) if case == "epl_centre_on_pixel" else ("lens_light", 0)
        cx, cy = _column(phys, *group, "center_x"), _column(phys, *group, "center_y")
        packed[:, cx] = float(gx[j])
        packed[:, cy] = float(gy[j])
        p = packed.cpu().numpy()
        # singular by construction: the float32 parameter IS the float32 grid coordinate, so x - cx and y - cy are exact zeros
        assert p.dtype == np.float32 and np.all(p[:, cx] == gx[j]) and np.all(p[:, cy] == gy[j])
        assert np.all((gx[j] - p[:, cx]) == 0) and np.all((gy[j] - p[:, cy]) == 0)
    else:
        col = lambda n: _column(phys, "source_light", 0, n)
        packed[:, col("n_sersic")] = 0.05
        packed[:, col("R_sersic")] = 0.01
        packed[:, col("center_x")] = 0.7  # (a corner of the source plane: most of the field maps further than 0.85 arcsec from it)
        packed[:, col("center_y")] = 0.7
        # singular by construction: (R / R_sersic)^(1/n) = (R / 0.01)^20 is beyond float32 for R > 0.85 arcsec.  The reference's
        # ray-shoot, evaluated in float32 on the host, says so for pixels of the first two (whole) tiles of every sample.
        from oracle import ref_torch as ref
        rs = ref.RefSimulator(phys, wl.sim_config, BATCH, dtype=torch.float32)
        params = H.struct_from_packed(phys, packed.cpu())
        bx, by = rs.beta(rs.img_X, rs.img_Y, params["lens_mass"])
        R = torch.hypot(bx - 0.7, by - 0.7)
        u = torch.pow(R / np.float32(0.01), np.float32(1.0 / 0.05))
        assert u.dtype == torch.float32 and bool(torch.isinf(u[:1024]).any(0).all())
    return wl, packed


@pytest.mark.parametrize("num_pix", [32, 40])
@pytest.mark.parametrize("case", ["epl_centre_on_pixel", "lens_light_centre_on_pixel", "sersic_overflow"])
def test_the_fallback_fires_and_is_right(gl, monkeypatch, case, num_pix):
    wl, packed = _singular_case(gl, case, num_pix)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    default, careful = _both(gl, monkeypatch, wl, obs, None, packed, _cotangent(num_pix))
    assert len(default) == len(careful) == 5
    for a, b in zip(default, careful):
        assert _equal_bits(a, b)
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))
    ll, img = default[0].cpu().numpy().reshape(-1), default[3].cpu().numpy()
    ll_o, _, _, img_o = H.oracle_loglike_and_grad(wl, packed.cpu().double(), obs.cpu().numpy(), None, BATCH)
    ll_o = ll_o.reshape(-1)
    if case == "sersic_overflow":
        # b_n = 1.9992 n - 0.3271 is negative at n = 0.05, so the profile GROWS outwards: the overflowed pixels are NaN -> 0 in float32
        # (the image stays free of NaN: the select-free body alone would have left them in), the pixels short of the overflow
        # are +inf in float32 and float64 alike, and the log-likelihood of every sample is NaN on both sides
        assert not np.isnan(img).any() and (img == 0).any() and np.isinf(img_o).any()
        assert np.isnan(ll_o).all()
    else:
        assert np.isfinite(ll_o).all() and np.isfinite(img).all()
        for t in default:
            assert torch.isfinite(t).all()
    assert np.array_equal(np.isnan(ll), np.isnan(ll_o))
    assert np.allclose(ll, ll_o, rtol=LL_RTOL, equal_nan=True), (ll, ll_o)
