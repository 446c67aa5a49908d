"""Arrival times on lens planes without a GPU: the weights of ``MultiPlane.delay_weights``, Fermat's principle and a closed form on the
composed float64 reference of tests/mp_tdelay_cases.py, and the host build of the kernel's thread body against that reference."""
import numpy as np
import pytest

from gigalens_amd.cosmology import MultiPlane, comoving_distance, deflection_scale, hubble_distance_mpc
from tests import mp_images_cases as MI
from tests import mp_tdelay_cases as TD
from tests import multilens_cases as MC

PLANE_SETS = ([0.4, 0.9, 1.4], [0.5, 1.0], [0.3, 0.6, 0.9, 1.2], [0.2, 0.21, 2.5])


# ---- the weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", PLANE_SETS)
def test_geometric_weight_times_coupling_is_the_potential_weight(planes):
    """``g_i C_{i, next(i)} = v_i`` (T_s in place of C for the last plane in front of the source), sources between and behind the planes."""
    mp = MultiPlane(planes, [], 3.0)
    between = [0.5 * (a + b) for a, b in zip(planes[:-1], planes[1:])]
    for z in between + [planes[-1] + 0.3, 2.0, 3.0, 4.5]:
        if z in planes:
            continue
        geom, pot = mp.delay_weights(z)
        T = mp.target_scales(z)
        ks = int(np.count_nonzero(T))
        assert geom.dtype == np.float64 and pot.dtype == np.float64 and geom.shape == pot.shape == (mp.K,)
        assert np.all(geom[:ks] > 0) and np.all(pot[:ks] > 0) and np.all(geom[ks:] == 0) and np.all(pot[ks:] == 0)
        assert ks == sum(zp < z for zp in planes)
        for i in range(ks):
            coupling = mp.lens_scales[i, i + 1] if i + 1 < ks else T[i]
            assert abs(geom[i] * coupling - pot[i]) <= 1e-13 * pot[i], (planes, z, i)
        # the potential weight is a constant of the plane
        assert np.array_equal(pot[:ks], mp.delay_weights(4.5)[1][:ks])


def test_a_source_on_a_plane_is_not_behind_it():
    mp = MultiPlane([0.4, 0.9], [], 3.0)
    geom, pot = mp.delay_weights(0.9)
    assert geom[1] == 0 and pot[1] == 0 and geom[0] > 0


def test_one_plane_weight_is_the_time_delay_distance():
    """``g_1 = (1 + z_d) D_d D_s / D_ds`` in units of c / H0, the angular-diameter distances from the comoving ones."""
    z_d, z_s = 0.5, 1.7
    mp = MultiPlane([z_d], [], 3.0)
    geom, pot = mp.delay_weights(z_s)
    xd, xs = float(comoving_distance(z_d)), float(comoving_distance(z_s))
    D_d, D_s, D_ds = xd / (1 + z_d), xs / (1 + z_s), (xs - xd) / (1 + z_s)
    assert abs(geom[0] - (1 + z_d) * D_d * D_s / D_ds) <= 1e-13 * geom[0]
    assert abs(pot[0] - geom[0] * deflection_scale(z_d, z_s, 3.0)) <= 1e-13 * pot[0]


def test_weight_and_hubble_distance_errors():
    mp = MultiPlane([0.4, 0.9], [], 3.0)
    for z in (0.4, 0.3, np.nan, np.inf, -1.0):
        with pytest.raises(ValueError):
            mp.delay_weights(z)
    assert hubble_distance_mpc(70.0) == 299792.458 / 70.0
    assert np.array_equal(hubble_distance_mpc([50.0, 100.0]), 299792.458 / np.asarray([50.0, 100.0]))
    for h in (0.0, -70.0, np.nan, np.inf, [70.0, 0.0]):
        with pytest.raises(ValueError):
            hubble_distance_mpc(h)


# ---- Fermat's principle: the images are the stationary points of T ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MI.GENERAL))
def test_images_are_stationary_points_of_the_arrival_time(name):
    """At the float64 images (Newton-polished to 1e-12) the central-difference gradient of the reference T (h = 1e-6) is at most
    1e-6 of the gradient one cell away.  A wrong weight breaks this at order one.  Images and T on the float64 couplings, the
    geometry the float64 weights belong to (mp_tdelay_cases: on the float32 values of the couplings the gradient at an image is
    6e-8 g |alpha|, the rounding of the couplings)."""
    cell = (MI.GENERAL_WINDOW[1] - MI.GENERAL_WINDOW[0]) / MI.GENERAL_CELLS
    n_images = 0
    for b in range(3):
        for s in range(2):
            img = TD.polished_images(name, b, s)
            if not len(img):
                continue
            at = np.linalg.norm(TD.reference_gradient(name, b, s, img[:, 0], img[:, 1]), axis=1)
            away = np.linalg.norm(TD.reference_gradient(name, b, s, img[:, 0] + cell, img[:, 1]), axis=1)
            print(f"{name} b={b} s={s}: |grad T| at the images {at.max():.2e}, a cell away {away.min():.2e}, ratio {(at / away).max():.2e}")
            assert np.all(at <= 1e-6 * away), (name, b, s, at, away)
            n_images += len(img)
    assert n_images >= 6


def test_exact_recursion_is_the_recursion_of_multilens_cases():
    """``exact_plane_sums`` differs from ``multilens_cases.plane_sums`` by the rounding of the couplings alone: with couplings that are
    float32 values both give the same bits, and the composed reference on either agrees to that rounding."""
    import torch
    c = MC.map_case("nfw|dpie|sis")

    class Rounded:
        K, plane_of_lens = c["mp"].K, c["mp"].plane_of_lens
        lens_scales = np.asarray(c["mp"].lens_scales, dtype=np.float32).astype(np.float64)
    px, py = MC.points(12)
    lp = MC._tensors({"lens_mass": MC.sample_rows(c["lens_params"], 3)}, MC.F64)["lens_mass"]
    x, y = (torch.as_tensor(v.astype(np.float64))[:, None].repeat(1, 3) for v in (px, py))
    for (ax, ay), (bx, by) in zip(TD.exact_plane_sums(c["phys"], Rounded, lp, x, y), MC.plane_sums(c["phys"], c["mp"], lp, x, y)):
        assert torch.equal(ax, bx) and torch.equal(ay, by)
    d = TD.lattice_data("nfw|dpie|sis")
    Te, _ = TD.reference_T(c["phys"], c["mp"], d["lens_params"], d["x"], d["y"], d["sx"], d["sy"], d["geom"], d["pot"], exact=True)
    assert 0 < TD.relative_to_terms(Te, d["ref"][0], d["ref"][1]) < 1e-6


def test_sis_closed_form():
    """``T(-) - T(+) = g_1 2 theta_E beta`` behind an SIS on plane 1 and an empty plane 2, to 1e-12."""
    phys, _, mp, lp = TD.sis_case()
    geom, pot = TD.weights(mp, [mp.z_ref])
    tE, beta = float(TD.SIS_THETA_E), float(TD.SIS_BETA)
    x = np.asarray([[[beta + tE, beta - tE]]])
    T, _ = TD.reference_T(phys, mp, lp, x, np.zeros_like(x), [[beta]], [[0.0]], geom, pot)
    want = TD.sis_closed_form(mp)
    print(f"T(-) - T(+) = {T[0, 0, 1] - T[0, 0, 0]:.15g}, closed form {want:.15g}")
    assert abs((T[0, 0, 1] - T[0, 0, 0]) - want) <= 1e-12 * want
    Th, _ = TD.host_T(phys, mp, lp, x, np.zeros_like(x), [[beta]], [[0.0]], geom, pot)  # (the float32 points: 1e-7 of theta)
    assert abs((Th[0, 0, 1] - Th[0, 0, 0]) - want) <= 1e-6 * want


# ---- the host build of the kernel's thread body against the composed reference ------------------------------------------------------
@pytest.mark.parametrize("name", MC.MAP_CASES)
def test_host_build_against_the_composed_reference(name):
    d = TD.lattice_data(name)
    (T, terms), (Tr, terms_r) = d["host"], d["ref"]
    assert np.isfinite(T).all() and np.isfinite(Tr).all() and (terms > 0).all()
    err = TD.relative_to_terms(T, Tr, terms)
    print(f"{name}: host build against the composed reference {err:.2e} of the terms (ceiling {TD.HOST_CEILING[name]:.2e}); "
          f"terms agree to {np.abs(terms / terms_r - 1).max():.1e}")
    assert err <= TD.HOST_CEILING[name]
    assert TD.HOST_CEILING[name] < 0.5 * TD.KERNEL_GATE  # the reference itself stands inside the kernel's gate
    # the two sources see different planes: the source between the last two planes is not deflected by the last
    assert np.count_nonzero(d["geom"][0]) == d["case"]["mp"].K - 1 and np.count_nonzero(d["geom"][1]) == d["case"]["mp"].K
    # T differs between the images of a lattice by far more than the gate resolves
    assert np.ptp(Tr, axis=2).min() > 1e6 * TD.KERNEL_GATE * terms.max()


def test_host_build_on_four_planes_against_the_composed_reference():
    """K = 4 = MP_MAXK: four sources behind 1, 2, 3 and 4 planes in one call (the last plane of a source is found by the first zero of
    its weights, or by the end of the row)."""
    d = TD.lattice_data(TD.FOUR_PLANES)
    (T, terms), (Tr, terms_r) = d["host"], d["ref"]
    assert d["case"]["mp"].K == TD.MAXK == 4 and T.shape == (1, 4, TD.N_LATTICE)
    assert [int(np.count_nonzero(g)) for g in d["geom"]] == [1, 2, 3, 4] and np.all(d["pot"] > 0)
    assert np.isfinite(T).all() and np.isfinite(Tr).all() and (terms > 0).all()
    err = TD.relative_to_terms(T, Tr, terms)
    print(f"four planes: host build against the composed reference {err:.2e} of the terms (ceiling {TD.HOST_CEILING[TD.FOUR_PLANES]:.2e}); "
          f"terms agree to {np.abs(terms / terms_r - 1).max():.1e}")
    assert err <= TD.HOST_CEILING[TD.FOUR_PLANES] < 0.5 * TD.KERNEL_GATE
    assert np.ptp(Tr, axis=2).min() > 1e6 * TD.KERNEL_GATE * terms.max()
    # every source's T is that of a call of its own
    mp = d["case"]["mp"]
    for s, z in enumerate(d["z"]):
        g, v = mp.delay_weights(z)
        alone = TD.host_T(d["case"]["phys"], mp, d["lens_params"], d["x"][:, s:s + 1], d["y"][:, s:s + 1], d["sx"][:, s:s + 1],
                          d["sy"][:, s:s + 1], g[None], v)[0]
        assert np.array_equal(alone[:, 0], T[:, s])


def test_sources_at_different_redshifts_share_one_call():
    """The joint weights of a call with two sources give each source the T of a call of its own with ``delay_weights(z_s)``: a plane
    behind the nearer source keeps its potential weight for the farther one, and does not enter the nearer one's T."""
    d = TD.lattice_data("nfw|dpie|sis")
    c = d["case"]
    z = TD.lattice_redshifts(c["mp"])
    assert np.all(d["pot"] > 0) and np.array_equal(d["pot"], c["mp"].delay_weights(z[1])[1])
    for s in (0, 1):
        g, v = c["mp"].delay_weights(z[s])
        for fn, joint in ((TD.reference_T, d["ref"][0]), (TD.host_T, d["host"][0])):
            alone = fn(c["phys"], c["mp"], d["lens_params"], d["x"][:, s:s + 1], d["y"][:, s:s + 1], d["sx"][:, s:s + 1],
                       d["sy"][:, s:s + 1], g[None], v)[0]
            assert np.array_equal(alone[:, 0], joint[:, s])


def test_host_build_propagates_nan_and_leaves_neighbours_alone():
    d = TD.lattice_data("epl_shear|sie")
    c = d["case"]
    x = d["x"].copy()
    x[1, 0, 7] = np.nan
    T, _ = TD.host_T(c["phys"], c["mp"], d["lens_params"], x, d["y"], d["sx"], d["sy"], d["geom"], d["pot"])
    assert np.isnan(T[1, 0, 7])
    keep = np.ones(T.shape, dtype=bool)
    keep[1, 0, 7] = False
    assert np.array_equal(T[keep], d["host"][0][keep])
