"""Host side of the multi-source-plane feature (no GPU): the distance ratios of gigalens_amd/cosmology.py, validation and storage
of the scales in PhysicalModel / ForwardProbModel, the exports of the built library and the register budgets of the new kernels."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_einstein_de_sitter_closed_form():
    from gigalens_amd.cosmology import deflection_scale
    dc = lambda z: 2.0 * (1.0 - 1.0 / np.sqrt(1.0 + z))  # D_C H0 / c for omega_m = 1
    z_lens, z_ref = 0.4, 2.0
    zs = np.array([0.45, 0.7, 1.0, 2.0, 4.0, 9.0])
    want = (1 - dc(z_lens) / dc(zs)) / (1 - dc(z_lens) / dc(z_ref))
    got = deflection_scale(z_lens, zs, z_ref, omega_m=1.0)
    assert got.dtype == np.float64 and got.shape == zs.shape
    assert np.max(np.abs(got / want - 1)) <= 1e-9
    assert abs(deflection_scale(z_lens, 1.0, z_ref, omega_m=1.0) / want[2] - 1) <= 1e-9  # a scalar for a scalar


def test_identity_and_monotonicity():
    from gigalens_amd.cosmology import deflection_scale
    for om in (0.3, 0.27, 1.0):
        assert abs(deflection_scale(0.5, 2.0, 2.0, omega_m=om) - 1.0) <= 1e-12
        c = deflection_scale(0.5, np.linspace(0.55, 8.0, 60), 2.0, omega_m=om)
        assert np.all(np.diff(c) > 0) and c[0] > 0
    assert deflection_scale(0.5, 1.0, 2.0) < 1.0 < deflection_scale(0.5, 4.0, 2.0)


def test_cosmology_validation():
    from gigalens_amd.cosmology import deflection_scale
    for zs in (0.4, 0.3, [1.0, 0.4], float("nan")):
        with pytest.raises(ValueError):
            deflection_scale(0.4, zs, 2.0)
    with pytest.raises(ValueError):
        deflection_scale(0.4, 1.0, 0.4)


def _profiles():
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.sis import SIS
    return [SIS()], [Sersic(), Sersic()]


def test_physical_model_stores_and_validates_scales():
    from gigalens_amd.model import PhysicalModel
    lenses, sources = _profiles()
    pm = PhysicalModel(lenses, [], sources)
    assert pm.source_light_scales.dtype == np.float32 and pm.source_light_scales.tolist() == [1.0, 1.0]
    pm = PhysicalModel(lenses, [], sources, source_light_scales=[0.6, 1.3])
    assert pm.source_light_scales.dtype == np.float32 and np.allclose(pm.source_light_scales, [0.6, 1.3])
    for bad in ([1.0], [1.0, 1.0, 1.0], [1.0, 0.0], [1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0]):
        with pytest.raises(ValueError):
            PhysicalModel(lenses, [], sources, source_light_scales=bad)


def test_forward_prob_model_stores_and_validates_scales():
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import ForwardProbModel
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J(dict(theta_E=tfd.LogNormal(0.0, 0.1), center_x=tfd.Normal(0, 0.1), center_y=tfd.Normal(0, 0.1)))])))
    xy = [np.array([1.0, -1.0], np.float32), np.array([0.5, -0.6, 0.1], np.float32)]
    kw = dict(include_pixels=False, centroids_x=xy, centroids_y=xy, centroids_errors_x=xy, centroids_errors_y=xy)
    pm = ForwardProbModel(prior, **kw)
    assert pm.centroids_scales.dtype == np.float32 and pm.centroids_scales.tolist() == [1.0, 1.0]
    pm = ForwardProbModel(prior, centroids_scales=[1.0, 0.55], **kw)
    assert pm.centroids_scales.dtype == np.float32 and np.allclose(pm.centroids_scales, [1.0, 0.55])
    for bad in ([1.0], [1.0, 0.0], [1.0, float("nan")], [-1.0, 1.0]):
        with pytest.raises(ValueError):
            ForwardProbModel(prior, centroids_scales=bad, **kw)
    with pytest.raises(ValueError):
        ForwardProbModel(prior, np.zeros((4, 4), np.float32), 0.1, 100.0, include_positions=False, centroids_scales=[1.0])


NEW_SYMBOLS = ["gl_model_set_source_scales", "gl_model_set_position_scales", "gl_image_positions_scaled", "gl_critical_curves_scaled"]


def test_new_abi_symbols_are_exported_and_bound():
    from gigalens_amd import _native
    assert os.path.exists(_native.lib_path()), "library not built (__graft_entry__.build())"
    h = ctypes.CDLL(_native.lib_path())
    header = open(os.path.join(ROOT, "include", "gigalens_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(h, name), name
        assert name in _native.SYMBOLS and f"int {name}(" in header, name
    # argument checks that need no device: null model, and (through the bound library) the error text
    L = _native.lib()
    assert L.gl_model_set_source_scales(None, None, 0) != 0 and b"model is null" in L.gl_last_error()
    assert L.gl_model_set_position_scales(None, None, 0) != 0


# the scaled form of every gl_clusterw_kernel instantiation the launcher can pick (gl_launch_generic.hip.h)
SCALED_CLUSTER = [f"gl_clusterw_scaled_kernel<{m}, glk::CwLensNfw<{h}>, {s}, {e}, {w}>"
                  for m in (1, 3) for h, s, e, w in ((1, 2, "true", 4), (2, 3, "true", 3), (2, 5, "true", 2),
                                                     (1, 2, "false", 4), (2, 3, "false", 4), (2, 5, "false", 3))]
# the point kernels that take a scale now.  (They index per-lens constant arrays dynamically and have used their private segment
# since before the scales -- 55 to 120 scratch instructions each -- so only the spill count is held for them.)
POINT_KERNELS = ["gl_pos_p1_kernel", "gl_pos_p3_kernel", "gl_img_scan_kernel", "gl_img_newton_kernel", "gl_crit_map_kernel<false>",
                 "gl_crit_refine_kernel<false>"]


@pytest.fixture(scope="module")
def metadata():
    import isa_flops as isa
    assert os.path.exists(isa.LIB), "library not built (__graft_entry__.build())"
    return isa.kernel_metadata(isa.code_object())


@pytest.mark.parametrize("pat", SCALED_CLUSTER + POINT_KERNELS)
def test_new_and_changed_kernels_do_not_spill(metadata, pat):
    import isa_flops as isa
    hits = [k for k in metadata if pat in k]
    assert len(hits) == 1, (pat, hits)
    md = metadata[hits[0]]
    assert md["vgpr_spill_count"] == 0, (hits[0], md)
    if pat in SCALED_CLUSTER:
        assert md["vgpr_count"] <= 512 // int(pat.rsplit(", ", 1)[1].rstrip(">")), (hits[0], md["vgpr_count"])  # the declared waves per SIMD fit
        if md["scratch_bytes"]:
            ins = isa.disassemble(md["co"], md["symbol"])
            assert not [i for i in ins if i[1].startswith("scratch_")], (hits[0], md["scratch_bytes"])
