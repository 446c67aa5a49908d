"""Multi-plane ray tracing without a GPU: ``cosmology.MultiPlane``, the K = 1 reduction of ``PhysicalModel(multiplane=...)``, and the
float64 restatement of tests/multilens_cases.py pinned on closed forms (two Shear planes, two coaxial SIS planes)."""
import numpy as np
import pytest

from gigalens_amd import cosmology as cos
from tests import multilens_cases as MC


# ---- MultiPlane --------------------------------------------------------------------------------------------------------
def test_couplings_are_deflection_scales():
    z = [0.3, 0.7, 1.4]
    mp = cos.MultiPlane(z, [0.5, 1.0, 2.5], MC.Z_REF)
    assert mp.K == 3 and mp.S == 3 and mp.plane_of_lens.tolist() == [0, 1, 2]
    assert mp.lens_scales.shape == (3, 3) and mp.source_scales.shape == (3, 3)
    for i in range(3):
        for j in range(3):
            want = cos.deflection_scale(z[i], z[j], MC.Z_REF) if i < j else 0.0
            assert mp.lens_scales[i, j] == want, (i, j)
    assert np.all(np.tril(mp.lens_scales) == 0) and np.all(mp.lens_scales[np.triu_indices(3, 1)] > 0)
    # a plane at or behind a target does not deflect it
    for s, zs in enumerate([0.5, 1.0, 2.5]):
        for i in range(3):
            want = cos.deflection_scale(z[i], zs, MC.Z_REF) if z[i] < zs else 0.0
            assert mp.source_scales[i, s] == want, (i, s)
    assert mp.source_scales[:, 0].tolist()[1:] == [0.0, 0.0]
    np.testing.assert_array_equal(mp.target_scales(1.0), mp.source_scales[:, 1])
    assert mp.target_scales(1.4)[2] == 0.0 and mp.target_scales(0.7)[1] == 0.0  # a target ON a plane is not deflected by it
    # the reference plane itself: plane i couples to it with 1
    np.testing.assert_allclose(mp.target_scales(MC.Z_REF), 1.0, rtol=0, atol=1e-15)
    # the Hubble constant cancels and omega_m enters
    assert not np.allclose(cos.MultiPlane(z, [], MC.Z_REF, omega_m=0.25).lens_scales, mp.lens_scales)


def test_planes_are_ordered_and_equal_redshifts_merge():
    mp = cos.MultiPlane([1.0, 0.4, 1.0, 0.7, 0.4], [2.0], MC.Z_REF)
    assert mp.K == 3 and mp.z_planes.tolist() == [0.4, 0.7, 1.0]
    assert mp.plane_of_lens.tolist() == [2, 0, 2, 1, 0] and mp.plane_of_lens.dtype == np.int32
    assert mp.lens_scales[0, 2] == cos.deflection_scale(0.4, 1.0, MC.Z_REF)
    one = cos.MultiPlane([0.5, 0.5], [1.0, 2.0], MC.Z_REF)
    assert one.K == 1 and one.lens_scales.tolist() == [[0.0]] and one.plane_of_lens.tolist() == [0, 0]
    np.testing.assert_array_equal(one.source_scales[0], cos.deflection_scale(0.5, [1.0, 2.0], MC.Z_REF))


@pytest.mark.parametrize("args", [
    ([0.5, float("nan")], [2.0], 3.0), ([0.5, float("inf")], [2.0], 3.0), ([0.5, 0.0], [2.0], 3.0), ([0.5, -1.0], [2.0], 3.0),
    ([0.5, 1.0], [float("nan")], 3.0), ([0.5, 1.0], [-2.0], 3.0), ([0.5, 1.0], [2.0], float("inf")), ([0.5, 1.0], [2.0], 0.0),
    ([0.5, 1.0], [2.0], 1.0), ([0.5, 1.0], [2.0], 0.8),   # z_ref at / in front of a lens
    ([0.5, 1.0], [0.5], 3.0), ([0.5, 1.0], [0.3], 3.0),   # a source at / in front of the first plane
    ([0.1, 0.2, 0.3, 0.4, 0.5], [2.0], 3.0),              # five planes
    ([], [2.0], 3.0),
])
def test_multiplane_refusals(args):
    with pytest.raises(ValueError):
        cos.MultiPlane(*args)


def test_four_planes_and_a_bad_target():
    mp = cos.MultiPlane([0.1, 0.2, 0.3, 0.4], [], 3.0)
    assert mp.K == 4 and mp.S == 0 and mp.source_scales.shape == (4, 0)
    for z in (0.1, 0.05, float("nan")):
        with pytest.raises(ValueError):
            mp.target_scales(z)


# ---- PhysicalModel -----------------------------------------------------------------------------------------------------
def test_one_plane_reduces_to_source_light_scales():
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    mp = cos.MultiPlane([0.5, 0.5], [1.0, 2.0], MC.Z_REF)
    pm = PhysicalModel([SIE(), Shear()], [], [Sersic(), Sersic()], multiplane=mp)
    same = PhysicalModel([SIE(), Shear()], [], [Sersic(), Sersic()], source_light_scales=cos.deflection_scale(0.5, [1.0, 2.0], MC.Z_REF))
    assert pm.multiplane is None and pm._source_scales_given
    np.testing.assert_array_equal(pm.source_light_scales, same.source_light_scales)
    assert pm.source_light_scales.dtype == np.float32
    two = PhysicalModel([SIE(), Shear()], [], [Sersic(), Sersic()], multiplane=cos.MultiPlane([0.5, 0.8], [1.0, 2.0], MC.Z_REF))
    assert two.multiplane.K == 2 and not two._source_scales_given and two.source_light_scales.tolist() == [1.0, 1.0]
    assert PhysicalModel([SIE()], [], [Sersic()]).multiplane is None
    with pytest.raises(ValueError):
        PhysicalModel([SIE(), Shear()], [], [Sersic(), Sersic()], multiplane=mp, source_light_scales=[1.0, 1.0])
    with pytest.raises(ValueError):
        PhysicalModel([SIE()], [], [Sersic(), Sersic()], multiplane=mp)
    with pytest.raises(ValueError):
        PhysicalModel([SIE(), Shear()], [], [Sersic()], multiplane=mp)


# ---- the restatement on closed forms ----------------------------------------------------------------------------------------
def test_two_shear_planes_are_linear():
    phys, _, mp, lp, T, A = MC.two_shear_case()
    x, y = MC.points(7)
    m = MC.maps(phys, mp, lp, x, y, T)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        np.testing.assert_allclose(m[2 + k], A[i, j], rtol=0, atol=1e-15)
    theta = np.stack([x, y]).astype(np.float64)
    np.testing.assert_allclose(m[:2, :, 0], A @ theta, rtol=0, atol=1e-14)
    C12, T2 = float(np.float32(mp.lens_scales[0, 1])), float(np.float32(T[1]))
    rot = 0.5 * (m[3] - m[4])
    want = T2 * C12 * float(np.float32(0.06)) * float(np.float32(0.08))
    assert want > 1e-3
    np.testing.assert_allclose(rot, want, rtol=0, atol=1e-15)
    assert abs(A[0, 1] - A[1, 0]) > 1e-3


def test_two_coaxial_sis_planes():
    phys, _, mp, lp, T, x, y, th2, beta = MC.two_sis_case()
    assert (th2 > 0).any() and (th2 < 0).any() and np.abs(th2).min() > 0.369 * MC.PIX
    m = MC.maps(phys, mp, lp, x, y, T)
    np.testing.assert_allclose(m[0, :, 0], beta, rtol=0, atol=1e-14)
    np.testing.assert_allclose(m[1, :, 0], 0.0, rtol=0, atol=1e-15)
    # the second-plane position itself: the target "plane 2" is reached with the couplings C_12, 0
    C12 = mp.lens_scales[0, 1]
    m2 = MC.maps(phys, mp, lp, x, y, [C12, 0.0])
    np.testing.assert_allclose(m2[0, :, 0], th2, rtol=0, atol=1e-14)


def test_one_plane_restatement_is_the_scaled_plane():
    """K = 1: ``beta = theta - c sum alpha`` and ``A = I - c H`` of the single-plane oracle."""
    import torch
    from oracle import ref_torch as ref
    c = MC.map_case("epl_shear|sie")
    mp1 = cos.MultiPlane([0.5, 0.5, 0.5], [], MC.Z_REF)
    x, y = MC.points(12)
    lp = MC.sample_rows(c["lens_params"], 2)
    T = mp1.target_scales(2.0)
    m = MC.maps(c["phys"], mp1, lp, x, y, T)
    cs = float(np.float32(T[0]))
    xt = torch.as_tensor(x).double()[:, None].repeat(1, 2)
    yt = torch.as_tensor(y).double()[:, None].repeat(1, 2)
    lp64 = MC._tensors({"lens_mass": lp}, MC.F64)["lens_mass"]
    bx = by = 0
    for lens, p in zip(c["phys"].lenses, lp64):
        fx, fy = ref.mass_deriv(lens, xt, yt, **p)
        bx, by = bx + fx, by + fy
    np.testing.assert_allclose(m[0], (xt - cs * bx).numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(m[1], (yt - cs * by).numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", MC.MAP_CASES)
def test_map_cases_are_well_posed(name):
    """What keeps a gate from hiding a failure, on the reference alone: no ray meets a lens centre, the float32 yardsticks are of
    float32 size, and the cases do what they are there for (an asymmetric A; a plane behind the target that changes nothing)."""
    c, x, y, ref, yard = MC.map_data(name, 70, 3)
    assert MC.min_centre_distance(c["phys"], c["mp"], MC.sample_rows(c["lens_params"], 3), x, y) > 0.1 * 0.37 * MC.PIX
    assert np.isfinite(ref).all()
    # (the dPIE Hessian at r_core = 0.03 .. 0.08 is a difference of nearly equal terms: float32 keeps 3.6 digits of A there, the
    # other cases 6; a dropped or wrongly coupled plane moves A by more than 1e-2, asserted below)
    for k in MC.MAP_KEYS:
        assert 0 < 4 * yard[k] <= (1e-4 if k.startswith("beta") else 2e-3), (k, yard[k])
    assert np.abs(ref[3] - ref[4]).max() > 1e-2
    one = MC.maps(c["phys"], cos.MultiPlane([0.5] * len(c["phys"].lenses), [], MC.Z_REF), MC.sample_rows(c["lens_params"], 3), x, y, [c["target"][0]])
    assert np.abs(one[2:] - ref[2:]).max() > 1e-2  # the same lenses on ONE plane
    if name == "nfw|dpie|sis":
        assert c["target"][2] == 0.0 and c["target"][1] > 0.0
        far = MC.map_data("nfw|dpie|sis>", 70, 3)[3]
        assert np.abs(far - ref).max() > 1e-2


@pytest.mark.parametrize("name", MC.RENDER_CASES)
def test_render_cases_are_well_posed(name):
    c, obs, ref, yard = MC.render_data(name)
    mp = c["mp"]
    assert mp.K == 2 and mp.source_scales[1, 0] == 0.0 and mp.source_scales[1, 1] > 0.0  # source 0 sits between the planes
    assert np.isfinite(ref["image"]).all() and ref["image"].max() > 1.0
    for k, v in yard.items():
        assert 0 < 4 * v <= 1e-3, (k, v)
    # every part matters: dropping the second plane, or lensing source 0 by it, changes the image by far more than a gate
    only1, _ = MC.image(c["phys"], c["cfg"], c["psf"], cos.MultiPlane([0.5, 0.5, 0.5], [0.8, 2.0], MC.Z_REF), c["params"], c["B"])
    assert MC.rel_err(only1.numpy(), ref["image"]) > 1e-2
    both, _ = MC.image(c["phys"], c["cfg"], c["psf"], cos.MultiPlane([0.5, 0.5, 0.7], [0.8, 2.0], MC.Z_REF), c["params"], c["B"])
    assert MC.rel_err(both.numpy(), ref["image"]) > 1e-3


@pytest.mark.parametrize("name", ["epl_shear|sie", "shared", "nfw|dpie|sis>"])
def test_jacobian_recursion_equals_autograd(name):
    """``maps_hessian`` (the recursion of d theta_j / d theta with every lens's Hessian) is ``maps`` (autograd of the composition)
    where no Hessian override differs from the derivative of the deflection."""
    c, x, y, ref, _ = MC.map_data(name, 70, 3)
    got = MC.maps_hessian(c["phys"], c["mp"], MC.sample_rows(c["lens_params"], 3), x, y, c["target"])
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * np.abs(ref).max())


def test_dpis_excess_is_in_the_reference():
    """The dPIS case: beta is the autograd composition's, A is not -- the reference's analytic dPIS Hessian carries a convergence
    excess, on the lens's own plane and through d theta_2 / d theta on the next."""
    c, x, y, ref, _ = MC.map_data("dpis|sie", 70, 3)
    auto = MC.maps(c["phys"], c["mp"], MC.sample_rows(c["lens_params"], 3), x, y, c["target"])
    np.testing.assert_allclose(auto[:2], ref[:2], rtol=0, atol=1e-14)
    assert np.abs(auto[2:] - ref[2:]).max() > 1e-2
    # the part that went through the second plane: the excess times C_12 times the SIE's Hessian
    first = MC.maps_hessian(c["phys"], c["mp"], MC.sample_rows(c["lens_params"], 3), x, y, [c["target"][0], 0.0])
    first_auto = MC.maps(c["phys"], c["mp"], MC.sample_rows(c["lens_params"], 3), x, y, [c["target"][0], 0.0])
    through = (ref[2:] - first[2:]) - (auto[2:] - first_auto[2:])
    assert np.abs(through).max() > 1e-3
