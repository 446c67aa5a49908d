"""The float64 restatement of the multi-plane image-position likelihood (tests/mp_positions_cases.py) and the host side of
``ForwardProbModel(centroids_redshifts=...)``, without a GPU: the restatement on one plane against
``multiplane_cases.expected_stats_positions``, its A against ``multilens_cases.maps_hessian`` / ``maps``, its autograd gradient against
central differences, the closed form on two Shear planes, the conditions every case must meet, and the validation of the redshifts
with the ``[F, K]`` table of couplings."""
import numpy as np
import pytest
import torch

from tests import multilens_cases as MC
from tests import multiplane_cases as SC
from tests import mp_positions_cases as PC

F64 = torch.float64


def _A_of(c, maps_fn):
    """``A [J, 4, B]`` of every image of case ``c`` from ``maps_fn`` (``MC.maps_hessian`` / ``MC.maps``)."""
    lp = c["params"]["lens_mass"]
    return np.concatenate([np.moveaxis(maps_fn(c["phys"], c["mp"], lp, fm["x"], fm["y"], fm["T"], F64)[2:], 0, 1) for fm in c["fams"]])


def test_one_plane_equals_the_scaled_single_plane_restatement():
    """K = 1 with target coupling c: ``beta = theta - c sum alpha``, ``A = I - c H`` -- ``expected_stats_positions`` to 1e-12."""
    from oracle import ref_torch as ref
    m = MC.map_case("epl_shear|sie")
    mp = MC._mp([0.5, 0.5, 0.5])
    assert mp.K == 1
    fams = [PC.family(mp, z, kx, ky, s) for z, kx, ky, s in PC._RING["k2"]]
    scales = [float(np.float32(fm["T"][0])) for fm in fams]
    assert len(set(scales)) == 2 and all(s > 0 for s in scales)
    c = dict(phys=m["phys"], mp=mp, params={"lens_mass": m["lens_params"], "lens_light": [], "source_light": []}, B=3, fams=fams)
    ll, red, _, _ = PC.loglike_grad(c)
    rs = ref.RefSimulator(m["phys"], _cfg(), 3, dtype=F64)
    pt = MC._tensors(c["params"], F64)
    ll_e, red_e, _ = SC.expected_stats_positions(rs, pt, [fm["x"] for fm in fams], [fm["y"] for fm in fams], [fm["ex"] for fm in fams],
                                                 [fm["ey"] for fm in fams], scales)
    assert MC.rel_err(ll, ll_e.detach().numpy()) <= 1e-12 and MC.rel_err(red, red_e.detach().numpy()) <= 1e-12


def _cfg():
    from gigalens_amd.simulator import SimulatorConfig
    return SimulatorConfig(delta_pix=MC.PIX, num_pix=8)


@pytest.mark.parametrize("name", PC.CASES)
def test_A_is_the_recursion_of_maps_hessian(name):
    c, ref, _ = PC.data(name)
    A = _A_of(c, MC.maps_hessian)
    assert A.shape == ref["A"].shape
    assert np.abs(ref["A"] - A).max() <= 1e-12 * np.abs(A).max()
    kinds = {type(l).__name__ for l in c["phys"].lenses}
    if "DPIS" not in kinds:  # no override that differs from the derivative of the deflection: autograd on the composition
        A2 = _A_of(c, MC.maps)
        assert np.abs(ref["A"] - A2).max() <= 1e-9 * np.abs(A2).max()
    else:
        assert np.abs(ref["A"] - _A_of(c, MC.maps)).max() > 1e-6  # (the excess is there)


@pytest.mark.parametrize("name", ["k2", "zoo_a", "k4"])
def test_autograd_gradient_equals_central_differences(name):
    c, ref, _ = PC.data(name)
    p0 = PC.GC.pack_np(c["phys"], c["params"]).numpy()
    g = ref["grad"]
    h = 1e-6
    worst = 0.0
    for k in range(p0.shape[1]):
        up, dn = p0.copy(), p0.copy()
        up[:, k] += h
        dn[:, k] -= h
        fd = (PC.loglike_grad(c, F64, up)[0] - PC.loglike_grad(c, F64, dn)[0]) / (2 * h)
        worst = max(worst, float(np.abs(fd - g[:, k]).max() / max(np.abs(g[:, k]).max(), 1e-300)))
    print(f"{name}: autograd vs central differences {worst:.3e} of the column scale")
    assert worst <= 1e-5


def test_two_shear_planes_closed_form():
    """``A = I - T_1 G1 - T_2 G2 (I - C_12 G1)`` (``MC.two_shear_case``), the same at every point."""
    phys, _, mp, lp, T, A = MC.two_shear_case()
    x, y = PC._points(PC.lattice(21, -19, 3), F64, 1), PC._points(PC.lattice(4, -6, 22), F64, 1)
    lpt = MC._tensors({"lens_mass": lp}, F64)["lens_mass"]
    _, _, got, _ = PC.trace(phys, mp, lpt, x, y, T)
    want = [A[0, 0], A[0, 1], A[1, 0], A[1, 1]]
    for g, w in zip(got, want):
        assert np.abs(g.detach().numpy() - w).max() <= 1e-15
    assert abs(want[1] - want[2]) > 1e-4  # (not symmetric)


@pytest.mark.parametrize("name", PC.CASES)
def test_conditions_hold(name):
    c, ref, yard = PC.data(name)
    min_det, min_r = PC.conditions(c)
    print(f"{name}: min |det A| {min_det:.3f}, nearest lens centre {min_r:.1f} px; float32 yardstick log_like {yard['log_like']:.2e}, "
          f"red_chi2 {yard['red_chi2']:.2e}, gradient {yard['grad']:.2e} of the gate")
    assert min_det >= PC.MIN_DET and min_r >= PC.MIN_PIX
    assert np.isfinite(ref["grad"]).all() and yard["grad"] <= 0.25  # the float32 restatement itself sits well inside the gate
    J = sum(fm["x"].size for fm in c["fams"])
    n_par = ref["grad"].shape[1]
    assert 6 <= J <= 9 and c["B"] * J * n_par > 64  # ragged 64-thread blocks, several workgroups in P3
    between = [fm for fm in c["fams"] if 0 < np.count_nonzero(fm["T"]) < c["mp"].K]
    behind = [fm for fm in c["fams"] if np.count_nonzero(fm["T"]) == c["mp"].K]
    assert between and (behind or name == "front")


def test_front_case_has_exact_zero_columns():
    c, ref, _ = PC.data("front")
    assert (ref["grad"][:, 11:] == 0).all() and (np.abs(ref["grad"][:, :11]).max(axis=0) > 0).all()  # the SIS on the last plane: 11..13


# ---- ForwardProbModel(centroids_redshifts=...) -----------------------------------------------------------------------
def _prob_model(c, **kw):
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import ForwardProbModel
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), 0.01) for k, v in d.items()}) for d in c["params"]["lens_mass"]])))
    args = dict(PC.centroids(c), include_pixels=False)
    args.update(kw)
    return ForwardProbModel(prior, **args)


def test_centroids_redshifts_validation_and_the_table_of_couplings():
    from gigalens_amd.cosmology import deflection_scale
    c = PC.case("k3")
    pm = _prob_model(c)
    T = pm.position_targets(c["mp"])
    assert T.shape == (3, 3)
    assert (T[0, 1:] == 0).all() and T[0, 0] > 0            # z = 0.5: between planes 1 and 2
    assert T[1, 2] == 0 and (T[1, :2] > 0).all()            # z = 1.1: between planes 2 and 3
    assert (T[2] > 0).all()                                 # z = 2.5: behind all
    assert T[1, 1] == pytest.approx(deflection_scale(0.7, 1.1, MC.Z_REF), rel=1e-14)
    for f, fm in enumerate(c["fams"]):
        assert np.array_equal(T[f], fm["T"])
    with pytest.raises(ValueError, match="give one"):
        _prob_model(c, centroids_scales=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="one redshift per image family"):
        _prob_model(c, centroids_redshifts=[1.0, 2.0])
    with pytest.raises(ValueError, match="finite"):
        _prob_model(c, centroids_redshifts=[1.0, float("nan"), 2.0])
    with pytest.raises(ValueError, match="finite"):
        _prob_model(c, centroids_redshifts=[1.0, float("inf"), 2.0])
    for z in (0.3, 0.2):  # at, and in front of, the first plane
        with pytest.raises(ValueError, match="behind the first lens plane"):
            _prob_model(c, centroids_redshifts=[z, 1.1, 2.5]).position_targets(c["mp"])
    from gigalens_amd.model import ForwardProbModel
    with pytest.raises(ValueError, match="centroids_x"):
        ForwardProbModel(pm.prior, np.zeros((4, 4), np.float32), 0.1, 100.0, include_positions=False, centroids_redshifts=[1.0])


def test_one_plane_multiplane_is_retained_for_the_redshifts():
    """K = 1: ``PhysicalModel`` rewrites the planes into scales and keeps the object; ``centroids_redshifts`` become ``centroids_scales``
    there, and a model without any ``MultiPlane`` points to ``centroids_scales``."""
    import types

    from gigalens_amd.model import PhysicalModel
    c = PC.case("k2")
    mp1 = MC._mp([0.5, 0.5, 0.5])
    phys1 = PhysicalModel(c["phys"].lenses, [], [], multiplane=mp1)
    assert phys1.multiplane is None and phys1._multiplane_single is mp1
    pm = _prob_model(c)
    scales, given = pm._family_scales(types.SimpleNamespace(phys_model=phys1, _mp=None))
    assert given and scales.dtype == np.float32
    assert np.array_equal(scales, np.asarray([mp1.target_scales(fm["z"])[0] for fm in c["fams"]], dtype=np.float32))
    with pytest.raises(ValueError, match="centroids_scales"):
        pm._family_scales(types.SimpleNamespace(phys_model=c["phys"], _mp=None))
    plain = _prob_model(c, centroids_redshifts=None, centroids_scales=[0.8, 1.2])
    s2, g2 = plain._family_scales(types.SimpleNamespace(phys_model=c["phys"], _mp=None))
    assert g2 and np.array_equal(s2, np.asarray([0.8, 1.2], np.float32))


# ---- the kernels' register budget (code-object metadata of the built library, as tests/test_kernel_resources.py reads it) -------
def test_new_kernels_have_no_spill_and_no_private_segment():
    """No VGPR spill and no private segment (hence no scratch traffic, in the kernels or in what they call) in P1 and P3."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_flops as isa
    if not os.path.exists(isa.LIB):
        pytest.skip("library not built")
    md = isa.kernel_metadata(isa.code_object())
    for kernel in ("gl_mp_pos_p1_kernel", "gl_mp_pos_p3_kernel"):
        hits = [k for k in md if kernel in k]
        assert len(hits) == 1, (kernel, hits)
        m = md[hits[0]]
        print(f"{kernel}: {m['vgpr_count']} VGPRs, {m['sgpr_count']} SGPRs, {m['lds_bytes']} B LDS, {m['scratch_bytes']} B private")
        assert m["vgpr_spill_count"] == 0 and m["scratch_bytes"] == 0 and m["vgpr_count"] <= 256, (kernel, m)
