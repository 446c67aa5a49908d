"""CPU-side checks of the image-plane position likelihood (gl_imgplane_loglike): the symbols are exported and bound, the methods
exist, the argument validation answers without a device, ``ImageFamilies`` validates its arrays and forms the default caps; the
float64 restatement of tests/imgplane_cases.py is pinned against the SIS closed form and a central finite difference of the
Newton-solved log-likelihood; and every case of the GPU tests meets its conditions -- no lost image, min |det A| at the predicted
images above the floor the case states, 4 x its float32 yardstick under the cap -- on the reference alone."""
import ctypes

import numpy as np
import pytest

from tests import imgplane_cases as IC
from tests import shear_cases as SC


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


NAMES = ("gl_imgplane_loglike", "gl_imgplane_loglike_workspace_bytes")


def test_symbols_exported_and_bound(native):
    lib = native.lib()
    for name in NAMES:
        assert name in native.SYMBOLS
        assert getattr(lib, name).argtypes == native.SYMBOLS[name][1]
    assert callable(native.Model.imgplane_loglike)
    from gigalens_amd import model
    from gigalens_amd.simulator import LensSimulator
    assert callable(LensSimulator.image_plane_log_like_and_grad)
    for meth in ("log_prob", "log_prob_and_grad", "log_prior", "init_centroids"):
        assert callable(getattr(model.ImagePlaneProbModel, meth))
    assert callable(model.ImageFamilies)


def test_argument_validation_without_gpu(native):
    lib = native.lib()
    GL_EINVAL = -1
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    for args in ((None, 4, 8), (p, 0, 8), (p, -1, 8), (p, 4, 0), (p, 4, -5)):
        for with_source in (0, 1):
            for want_grad in (0, 1):
                assert lib.gl_imgplane_loglike_workspace_bytes(*args, with_source, want_grad) == 0, args
    off = (ctypes.c_int32 * 3)(0, 4, 8)
    # model, params, B, image_table, family_table, offsets, J, F, source, tol, max_iter, ll, chi2, n_lost, pred, grad, grad_source, ws, bytes, stream
    full = [p, p, 4, p, p, off, 8, 2, None, 1e-6, 30, p, p, p, None, None, None, p, 4096, None]
    for null_at in (0, 1, 3, 4, 5, 11, 12, 13, 17):  # model, params, the tables, the offsets, ll, chi2, n_lost, workspace
        args = list(full)
        args[null_at] = None
        assert lib.gl_imgplane_loglike(*args) == GL_EINVAL, null_at
        assert b"null argument" in lib.gl_last_error()
    for B, J, F in ((0, 8, 2), (-3, 8, 2), (4, 0, 2), (4, -1, 2), (4, 8, 0)):
        args = list(full)
        args[2], args[6], args[7] = B, J, F
        assert lib.gl_imgplane_loglike(*args) == GL_EINVAL, (B, J, F)
        assert b"must be positive" in lib.gl_last_error()

    def answer(offsets, J, source=None, grad_source=None, tol=1e-6, max_iter=30):
        args = list(full)
        args[5], args[6], args[7] = (ctypes.c_int32 * len(offsets))(*offsets), J, len(offsets) - 1
        args[8], args[16], args[9], args[10] = source, grad_source, tol, max_iter
        return lib.gl_imgplane_loglike(*args), lib.gl_last_error()

    assert answer([0, 65], 65) == (GL_EINVAL, answer([0, 65], 65)[1]) and b"at most 64" in answer([0, 65], 65)[1]  # a family of 65 images
    assert answer([0, 64, 129], 129)[0] == GL_EINVAL and b"family 1 holds 65" in lib.gl_last_error()
    assert answer([0, 4, 4], 4)[0] == GL_EINVAL and b"holds no image" in lib.gl_last_error()
    assert answer([0, 4, 7], 8)[0] == GL_EINVAL and b"family offsets" in lib.gl_last_error()
    assert answer([1, 8], 8)[0] == GL_EINVAL and b"family offsets" in lib.gl_last_error()
    assert answer([0, 1, 8], 8)[0] == GL_EINVAL and b"barycentre source takes two or more" in lib.gl_last_error()
    assert answer([0, 4, 8], 8, grad_source=p)[0] == GL_EINVAL and b"grad_source without" in lib.gl_last_error()
    for tol, max_iter in ((0.0, 30), (-1.0, 30), (float("nan"), 30), (1e-6, 0)):
        assert answer([0, 4, 8], 8, tol=tol, max_iter=max_iter)[0] == GL_EINVAL and b"tol must be > 0" in lib.gl_last_error()


def test_image_families_validation_and_default_caps():
    from gigalens_amd.model import ImageFamilies
    x, y = [[1.0, 0.0, -1.0], [0.5, -0.5]], [[0.0, 1.0, 0.0], [0.2, 0.1]]
    f = ImageFamilies(x, y, 0.02, scales=[1.0, 0.7])
    assert (f.F, f.J, len(f)) == (2, 5, 5) and f.offsets.tolist() == [0, 3, 5] and f.min_count == 2
    for a in (f.x, f.y, f.sigma, f.scales, f.max_shift):
        assert a.dtype == np.float32 and a.shape == (5,)
    assert f.scales.tolist() == [1.0, 1.0, 1.0, np.float32(0.7), np.float32(0.7)]
    # the default cap: half the distance to the nearest sibling, float64 then float32 -- the balls of two siblings at most touch
    half = [np.sqrt(2) / 2] * 3 + [0.5 * np.hypot(1.0, np.float64(np.float32(0.2)) - np.float64(np.float32(0.1)))] * 2
    assert np.array_equal(f.max_shift, np.asarray(half, dtype=np.float32))
    for a, b in ((0, 1), (1, 2), (3, 4)):
        assert np.hypot(f.x[a] - f.x[b], f.y[a] - f.y[b]) >= np.float64(f.max_shift[a]) + np.float64(f.max_shift[b]) - 1e-7
    assert np.array_equal(ImageFamilies(x, y, [0.02, 0.03]).sigma, np.float32([0.02] * 3 + [0.03] * 2))
    assert np.array_equal(ImageFamilies(x, y, [[0.02, 0.03, 0.04], 0.05]).sigma, np.float32([0.02, 0.03, 0.04, 0.05, 0.05]))
    assert np.array_equal(ImageFamilies(x, y, 0.02, max_shift=0.3).max_shift, np.full(5, 0.3, np.float32))
    assert np.array_equal(ImageFamilies(x, y, 0.02, max_shift=[[0.1, 0.2, 0.3], [0.4, 0.5]]).max_shift, np.float32([0.1, 0.2, 0.3, 0.4, 0.5]))
    one = ImageFamilies([[1.0]], [[0.0]], 0.02, max_shift=0.3)  # a family of one image: with its cap given
    assert one.min_count == 1 and one.max_shift.tolist() == [np.float32(0.3)]
    t = f.device_tables("cpu")
    assert t["image"].shape == (5, 5) and t["family"].shape == (3, 5) and t["family"].tolist() == [[0, 0, 0, 1, 1], [0, 0, 0, 3, 3], [3, 3, 3, 2, 2]]
    assert f.device_tables("cpu") is t  # uploaded once per device
    assert abs(f.norm - 5 * np.log(2 * np.pi * np.float64(np.float32(0.02)) ** 2)) <= 1e-12
    bad = [
        dict(x=x, y=[[0.0, 1.0], [0.2, 0.1]]),                       # a shape mismatch inside a family
        dict(x=x, y=y[:1]),                                         # families missing in y
        dict(x=[[1.0, np.nan, -1.0], [0.5, -0.5]]),                 # a position that is not finite
        dict(sigma=0.0), dict(sigma=[0.02, -0.02]), dict(sigma=np.inf), dict(sigma=[0.02, 0.02, 0.02]),
        dict(scales=[1.0, 0.0]), dict(scales=[1.0]),
        dict(max_shift=0.0), dict(max_shift=[[0.1, 0.2], [0.4, 0.5]]),
        dict(x=[[1.0, 1.0, -1.0], [0.5, -0.5]], y=[[0.0, 0.0, 0.0], [0.2, 0.1]]),  # two coincident images
        dict(x=[list(np.linspace(-2, 2, 65))], y=[[0.0] * 65]),     # more than 64 images in a family
        dict(x=[[1.0, 0.0], [0.5]], y=[[0.0, 1.0], [0.2]]),         # a family of one image without max_shift
    ]
    for kw in bad:
        args = dict(dict(x=x, y=y, sigma=0.02), **kw)
        with pytest.raises(ValueError):
            ImageFamilies(args.pop("x"), args.pop("y"), args.pop("sigma"), **args)


def test_prob_model_argument_checks():
    from gigalens_amd.model import ImageFamilies, ImagePlaneProbModel
    with pytest.raises(TypeError, match="ImageFamilies"):
        ImagePlaneProbModel(None, object())
    with pytest.raises(ValueError, match="two or more images"):
        ImagePlaneProbModel(None, ImageFamilies([[1.0]], [[0.0]], 0.02, max_shift=0.3))
    with pytest.raises(TypeError, match="ForwardProbModel"):
        ImagePlaneProbModel(None, ImageFamilies([[1.0, -1.0]], [[0.0, 0.1]], 0.02), strong=object())


def test_restatement_equals_the_sis_closed_form():
    c = IC.sis_case()
    fams = IC.families(c["fam"])
    r = IC.loglike_grad(c["phys"], c["rows"], fams, IC.F64, source=IC.sis_source(c))
    cf = IC.sis_closed_form(fams)
    assert not r["lost"].any() and r["n_lost"].tolist() == [0] * IC.B
    for b in range(IC.B):
        assert np.abs(r["predicted"][:, :, b] - cf["predicted"]).max() <= 1e-12
        assert abs(r["chi2"][b] - cf["chi2"]) <= 1e-10 * cf["chi2"]
        assert abs(r["log_like"][b] - (-0.5 * cf["chi2"] - fams.norm)) <= 1e-10
        got = np.array([r["grad"][b, 0], r["grad_source"][0, b, 0], r["grad_source"][1, b, 0]])
        assert np.all(np.abs(got - cf["grad"]) <= 1e-9 * cf["scale"]), (got, cf["grad"])
        assert np.all(r["grad"][b, 1:] != 0)  # the centre takes part: d beta / d centre at the images
    # the source moved beyond theta_E: the inner image does not exist and is lost at its cap, the survivor alone makes the gradient
    far = IC.sis_case(b=1.2)
    r = IC.loglike_grad(far["phys"], far["rows"], fams, IC.F64, source=IC.sis_source(far))
    assert r["lost"][:, 0].tolist() == [False, True] and np.isnan(r["predicted"][:, 1, 0]).all()
    b = float(np.float32(1.2))
    d = np.array([b + 1.0 - np.float64(fams.x[0]), -np.float64(fams.y[0])])
    w = 1.0 / np.float64(fams.sigma[0]) ** 2
    cap = np.float64(fams.max_shift[1])
    assert abs(r["chi2"][0] - ((d ** 2).sum() * w + cap ** 2 * w)) <= 1e-9 * r["chi2"][0]
    assert abs(r["grad"][0, 0] - (-d[0] * w)) <= 1e-9 * abs(d[0] * w)  # u_x d beta_x / d theta_E = -u_x at x > 0


@pytest.mark.parametrize("name", IC.CASES)
def test_restatement_gradient_equals_a_finite_difference(name):
    """Central differences of the Newton-solved float64 log-likelihood, h = 1e-6 on every column: their truncation and the solver's
    1e-11 leave ~1e-8 of the largest column, the bound is 1e-6 of it."""
    c, fams, ref, _ = IC.data(name)
    rows = c["rows"].astype(np.float64)
    h = 1e-6
    fd = np.zeros_like(ref["grad"])
    for k in range(rows.shape[1]):
        up, dn = rows.copy(), rows.copy()
        up[:, k] += h
        dn[:, k] -= h
        fd[:, k] = (IC.loglike_only(c["phys"], up, fams) - IC.loglike_only(c["phys"], dn, fams)) / (2 * h)
    err = np.abs(fd - ref["grad"]).max() / np.abs(ref["grad"]).max()
    print(f"{name}: implicit gradient against central differences {err:.2e} of the largest column")
    assert err <= 1e-6


def test_explicit_source_gradient_equals_a_finite_difference():
    import torch
    c, fams, bary, _ = IC.data("epl_shear_quad")
    _, lp = IC.PC.leaf(dict(phys=c["phys"]), IC.F64, packed=c["rows"])
    src = IC.solve(c["phys"], lp, fams, IC.F64)["src"].permute(0, 2, 1).numpy().astype(np.float32)  # [2, B, F]: the barycentres, rounded
    r = IC.loglike_grad(c["phys"], c["rows"], fams, IC.F64, source=src)
    ll = lambda sv: (-0.5 * IC.solve(c["phys"], lp, fams, IC.F64, source=torch.as_tensor(sv))["chi2_j"].sum(0)).numpy()
    h = 1e-6
    for a in range(2):
        up, dn = src.astype(np.float64), src.astype(np.float64)
        up[a] += h
        dn[a] -= h
        fd = (ll(up) - ll(dn)) / (2 * h)
        assert np.abs(fd - r["grad_source"][a, :, 0]).max() <= 1e-6 * np.abs(r["grad_source"]).max()
    # explicit sources leave no cotangent on the observed points: the lens gradient is another one than the barycentre's
    assert np.abs(r["grad"] - bary["grad"]).max() >= 1e-3 * np.abs(bary["grad"]).max()
    assert np.abs(r["chi2"] - bary["chi2"]).max() <= 1e-4 * np.abs(bary["chi2"]).max()  # (the same sources up to float32 rounding)


@pytest.mark.parametrize("name", IC.CASES)
def test_cases_meet_their_conditions_on_the_reference(name):
    c, fams, ref, yard = IC.data(name)
    assert c["rows"].shape[0] == IC.B and ref["predicted"].shape == (2, fams.J, IC.B)
    assert not ref["lost"].any() and ref["n_lost"].tolist() == [0] * IC.B
    min_det = float(np.abs(ref["det"]).min())
    print(f"{name}: J = {fams.J} in {fams.F} famil(ies), min |det A| {min_det:.3f} (floor {IC.DET_FLOOR[name]}), smallest cap "
          f"{fams.max_shift.min():.3f}, float32 yardstick " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    assert min_det >= IC.DET_FLOOR[name]
    assert 4 * yard["grad"] <= SC.GATE_CAP, (name, yard)
    # every predicted image stays well inside its cap, and chi2 is what its residuals say
    d = np.hypot(ref["predicted"][0] - fams.x[:, None], ref["predicted"][1] - fams.y[:, None])
    assert np.all(d <= 0.5 * fams.max_shift[:, None])
    assert np.allclose(ref["chi2"], (d ** 2 / np.float64(fams.sigma[:, None]) ** 2).sum(0), rtol=1e-12)
    if name == "epl_shear_quad":  # the four images the case is stated with
        im = c["truth_images"][0]
        assert im.shape[0] == 4
        for qx, qy in IC.QUAD_IMAGES:
            assert np.hypot(im[:, 0] - qx, im[:, 1] - qy).min() <= 1e-4
    if name == "two_planes":
        assert fams.F == 2 and sorted(set(fams.scales.tolist())) == [np.float32(0.7), 1.0]


@pytest.mark.parametrize("cfg", IC.EDGES)
def test_launch_edge_configurations_on_the_reference(cfg):
    d = IC.edge_data(cfg)
    fams, ref, yard = d["fams"], d["ref"], d["yard"]
    J, nb, F = IC.EDGES[cfg]
    assert (fams.J, d["case"]["rows"].shape[0], fams.F) == (J, nb, F) and str(J * nb) == cfg
    assert not ref["lost"].any() and float(np.abs(ref["det"]).min()) >= IC.DET_FLOOR["two_planes"]
    assert (d["source"] is None) == (fams.min_count >= 2)
    assert 4 * yard["grad"] <= SC.GATE_CAP, (cfg, yard)
    # lanes are (image, sample) with the sample fastest: a family straddles the boundary between the first two waves
    if J * nb > 64:
        first, last = fams.offsets[:-1] * nb, fams.offsets[1:] * nb - 1
        assert any(a < 64 <= b for a, b in zip(first, last))
