"""The lens-equation solver on lens planes (csrc/gl_multiplane_images.hip.h; ``LensSimulator.image_positions(source_redshifts=...)``) on
the GPU, against the closed forms and the float64 solver of tests/mp_images_cases.py.  Gates: those of
``images_cases._check_against_f64`` (residual in float64 <= 2 tol; position <= max(5e-5, 2e-6 |mu|); mu to 1e-3 relative below
|mu| = 30; images below |mu| = 0.02 not compared; a pair with two reference images closer than two cells left to the fold rule)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests import images_cases as IC
from tests import mp_images_cases as C
from tests import multilens_cases as MC
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
_SIMS = {}


def _sim(gl, key, phys_mp, B):
    from gigalens_amd.simulator import SimulatorConfig
    if (key, B) not in _SIMS:
        _SIMS[key, B] = gl.LensSimulator(phys_mp, SimulatorConfig(delta_pix=0.1, num_pix=8), bs=B)
    return _SIMS[key, B]


def _lens_t(lens_params, B=None):
    rows = lens_params if B is None else MC.sample_rows(lens_params, B)
    return [{k: torch.as_tensor(v) for k, v in d.items()} for d in rows]


def _images(out, b, s):
    x, y, mu, n = (t.cpu().numpy() for t in out)
    k = int(n[b, s])
    assert np.all(np.isnan(x[b, s, k:])) and np.all(np.isnan(y[b, s, k:])) and np.all(np.isnan(mu[b, s, k:]))
    return np.stack([x[b, s, :k], y[b, s, :k], mu[b, s, :k]], axis=1).astype(np.float64)


# ---- 1. two shear planes: A not symmetric, one root --------------------------------------------------------------------------------
@pytest.mark.parametrize("num_cells", [8, 1, 5])  # 1: two triangles; 5: 50 triangles, a partial wave round in every wave
def test_two_shear_planes_closed_form(gl, num_cells):
    (phys, phys_mp, mp, lp, T, A), sx, sy, roots, mu = C.two_shear_sources()
    sim = _sim(gl, "two_shear", phys_mp, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # nothing is dropped: no warning
        out = sim.image_positions(_lens_t(lp), torch.as_tensor(sx), torch.as_tensor(sy), window=C.SHEAR_WINDOW, num_cells=num_cells,
                                  source_redshifts=2.0, strict=True)
    assert tuple(out[0].shape) == (1, 3, 8) and out[3].cpu().tolist() == [[1, 1, 0]]  # (B S = 3; the third root lies outside)
    for s in (0, 1):
        got = _images(out, 0, s)
        dist = np.hypot(got[0, 0] - roots[s, 0], got[0, 1] - roots[s, 1])
        print(f"num_cells {num_cells} source {s}: position error {dist:.2e}, mu {got[0, 2]:.7f} (closed form {mu:.7f})")
        assert dist <= max(5e-5, 2e-6 * abs(mu)) and abs(got[0, 2] - mu) <= 1e-3 * abs(mu)
    assert len(_images(out, 0, 2)) == 0
    # the counters of the native call: nothing found, nothing dropped for the source outside
    o, n, d = sim._model.multiplane_image_positions(sim._pack_partial({"lens_mass": _lens_t(lp)}), torch.as_tensor(sx).to(sim.device),
                                                    torch.as_tensor(sy).to(sim.device), np.stack([T] * 3), C.SHEAR_WINDOW, num_cells, 8,
                                                    IC._default_tol(C.SHEAR_WINDOW), 30)
    assert n.cpu().tolist() == [[1, 1, 0]] and d.cpu().tolist() == [[0, 0, 0]] and bool(torch.isnan(o[0, 2]).all())


# ---- 2. two coaxial SIS planes, sources on the axis ---------------------------------------------------------------------------------
def test_two_coaxial_sis_planes(gl):
    phys, phys_mp, mp, lp, T = MC.two_sis_case()[:5]
    sim = _sim(gl, "two_sis", phys_mp, 1)
    sx, sy = C.SIS_BETA[None, :].copy(), np.zeros((1, len(C.SIS_BETA)), np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (triangles that straddle the ring theta_2 = 0 may seed candidates that drop)
        out = sim.image_positions(_lens_t(lp), torch.as_tensor(sx), torch.as_tensor(sy), window=C.SIS_WINDOW, num_cells=C.SIS_CELLS,
                                  source_redshifts=[2.0] * len(C.SIS_BETA))
    tol = IC._default_tol(C.SIS_WINDOW)
    for s, beta in enumerate(C.SIS_BETA):
        got = _images(out, 0, s)
        ref = C.solve64(phys, mp, lp, 0, T, beta, 0.0, C.SIS_WINDOW, 2 * C.SIS_CELLS)
        deriv = C.deriv64(phys, mp, lp, 0, T)
        res = IC._residual64(deriv, got[:, 0], got[:, 1], float(beta), 0.0)
        assert np.all(res <= 2 * tol), (s, res, tol)
        assert not C.fold_pair(ref, C.SIS_WINDOW, C.SIS_CELLS)
        assert C.compare_images(got, ref, f"two SIS planes, beta = {beta}") == len(ref)  # the count, and every image
        for x in C.two_sis_closed_form(beta)[1]:  # the outer branches against the closed form
            j = np.argmin(np.abs(got[:, 0] - x))
            assert np.hypot(got[j, 0] - x, got[j, 1]) <= max(5e-5, 2e-6 * abs(got[j, 2])), (beta, x, got[j])


# ---- 3. general lenses against float64: B = 3, two sources at two redshifts ------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.GENERAL))
def test_general_lenses_against_float64(gl, name):
    c = MC.map_case(name)
    z, sx, sy = C.general_sources(name)
    sim = _sim(gl, name, c["phys_mp"], 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        compared, counts = C.check_against_f64(sim, c["phys"], c["mp"], c["lens_params"], z, sx, sy, C.GENERAL_WINDOW, C.GENERAL_CELLS,
                                               maps=C.reference_maps(name))
    print(name, "pairs compared", compared, "images per pair", counts)
    assert 4 * (6 - compared) <= 6 and max(counts) >= 3


# ---- 4. a source between the planes: only the front plane acts -----------------------------------------------------------------------
def test_source_between_the_planes_equals_the_scaled_front_plane(gl):
    """z = 0.8 behind EPL + Shear (z = 0.5) and in front of the SIE (z = 1.0): the images of the single-plane solver on EPL + Shear alone
    with ``deflection_scale = T_0`` -- two independently coded paths."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    c = MC.map_case("epl_shear|sie")
    z, sx, sy = C.general_sources("epl_shear|sie")
    T = c["mp"].target_scales(0.8)
    assert T[0] > 0 and T[1] == 0
    sim = _sim(gl, "epl_shear|sie", c["phys_mp"], 3)
    front = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:2], [], []), SimulatorConfig(delta_pix=0.1, num_pix=8), bs=3)
    lt = _lens_t(c["lens_params"], 3)
    kw = dict(window=C.GENERAL_WINDOW, num_cells=C.GENERAL_CELLS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = sim.image_positions(lt, torch.as_tensor(sx), torch.as_tensor(sy), source_redshifts=0.8, **kw)
        b = front.image_positions(lt[:2], torch.as_tensor(sx), torch.as_tensor(sy), deflection_scale=float(np.float32(T[0])), **kw)
    assert torch.equal(a[3].cpu(), b[3].cpu()) and int(a[3].max()) >= 2
    for bb in range(3):
        for s in range(2):
            ga, gb = _images(a, bb, s), _images(b, bb, s)
            for p, q in zip(ga, gb):
                assert np.hypot(p[0] - q[0], p[1] - q[1]) <= max(5e-5, 2e-6 * abs(q[2])), (bb, s, p, q)
                if abs(q[2]) < 30:
                    assert abs(p[2] - q[2]) <= 1e-3 * abs(q[2]), (bb, s, p, q)


# ---- 5. per-source targets -----------------------------------------------------------------------------------------------------------
def test_per_source_targets(gl):
    c = MC.map_case("nfw|dpie|sis")
    sim = _sim(gl, "nfw|dpie|sis", c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"], 3)
    sx = torch.as_tensor(np.full((3, 2), 0.1, np.float32))
    sy = torch.as_tensor(np.full((3, 2), -0.05, np.float32))
    kw = dict(window=C.GENERAL_WINDOW, num_cells=C.GENERAL_CELLS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        both = sim.image_positions(lt, sx, sy, source_redshifts=[1.1, 2.5], **kw)  # (1.1: in front of the last of the K = 3 planes)
        one = [sim.image_positions(lt, sx[:, s:s + 1], sy[:, s:s + 1], source_redshifts=z, **kw) for s, z in enumerate((1.1, 2.5))]
    bits = lambda t: t.cpu().contiguous().view(torch.int32)  # (the NaN padding compares by its bits)
    for s in range(2):
        for t_both, t_one in zip(both, one[s]):
            assert torch.equal(bits(t_both[:, s:s + 1]), bits(t_one))
    # the same position at two redshifts: different image sets
    assert not torch.equal(torch.nan_to_num(both[0][:, 0]), torch.nan_to_num(both[0][:, 1]))
    assert int(both[3].min()) >= 1


# ---- 6. launch edges -----------------------------------------------------------------------------------------------------------------
def test_four_planes(gl):
    phys, phys_mp, mp, lp = C.four_plane_case()
    sim = _sim(gl, "four_planes", phys_mp, 1)
    sx, sy = np.array([[0.05, 0.1]], np.float32), np.array([[0.03, -0.05]], np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        compared, counts = C.check_against_f64(sim, phys, mp, lp, (2.0, 2.0), sx, sy, C.GENERAL_WINDOW, C.GENERAL_CELLS)
    assert compared == 2 and min(counts) >= 3


def test_three_planes_source_in_front_of_the_last(gl):
    c = MC.map_case("nfw|dpie|sis")
    sim = _sim(gl, "nfw|dpie|sis", c["phys_mp"], 1)
    assert c["mp"].K == 3 and c["mp"].target_scales(1.1)[2] == 0
    lp = MC.sample_rows(c["lens_params"], 1)
    sx, sy = np.array([[0.04]], np.float32), np.array([[-0.05]], np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        compared, counts = C.check_against_f64(sim, c["phys"], c["mp"], lp, 1.1, sx, sy, C.GENERAL_WINDOW, C.GENERAL_CELLS)
    assert compared == 1 and counts[0] >= 1


def test_max_images_one_on_a_multiply_imaged_source(gl):
    phys, phys_mp, mp, lp = C.four_plane_case()
    sim = _sim(gl, "four_planes", phys_mp, 1)
    args = (_lens_t(lp), torch.tensor([[0.05]]), torch.tensor([[0.03]]))
    kw = dict(window=C.GENERAL_WINDOW, num_cells=C.GENERAL_CELLS, source_redshifts=2.0, max_images=1)
    with pytest.warns(RuntimeWarning, match="found but not returned"):
        x, y, mu, n = sim.image_positions(*args, **kw)
    assert tuple(x.shape) == (1, 1, 1) and n.cpu().tolist() == [[1]] and bool(torch.isfinite(x).all())
    with pytest.raises(RuntimeError):
        sim.image_positions(*args, strict=True, **kw)
    _, n_img, n_drop = sim._model.multiplane_image_positions(sim._pack_partial({"lens_mass": args[0]}), args[1].to(sim.device),
                                                             args[2].to(sim.device), mp.target_scales(2.0)[None], C.GENERAL_WINDOW,
                                                             C.GENERAL_CELLS, 1, IC._default_tol(C.GENERAL_WINDOW), 30)
    assert n_img.cpu().tolist() == [[1]] and int(n_drop[0, 0]) > 0


# ---- 7. rules ------------------------------------------------------------------------------------------------------------------------
def test_python_rules(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    c = MC.map_case("epl_shear|sie")
    sim = _sim(gl, "epl_shear|sie", c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"], 3)
    src = (torch.zeros(3, 2) + 0.05, torch.zeros(3, 2) - 0.03)
    with pytest.raises(_native.UnsupportedLensError):  # planes, and a source without a redshift names no plane
        sim.image_positions(lt, *src)
    with pytest.raises(_native.UnsupportedLensError):
        sim.image_positions(lt, *src, deflection_scale=0.9)
    for bad_scale in (0.9, [1.0, 1.0], [0.9, 1.1]):
        with pytest.raises(ValueError, match="deflection_scale"):
            sim.image_positions(lt, *src, source_redshifts=2.0, deflection_scale=bad_scale)
    for bad_z in (float("nan"), float("inf"), 0.5, 0.3, [2.0, 0.5], [2.0, float("nan")], [2.0], [2.0, 2.0, 2.0], [[2.0, 2.0]]):
        with pytest.raises(ValueError, match="source_redshifts"):
            sim.image_positions(lt, *src, source_redshifts=bad_z)
    with pytest.raises(NotImplementedError):
        sim.image_positions(sim._pack_partial({"lens_mass": lt}).clone().requires_grad_(True), *src, source_redshifts=2.0)
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    plain = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:2], [], []), cfg, bs=3)
    with pytest.raises(ValueError, match="deflection_scale"):  # no MultiPlane: the keyword of that model is deflection_scale
        plain.image_positions(lt[:2], *src, source_redshifts=2.0)
    # a one-plane MultiPlane: the redshifts become the per-source deflection scales of the existing path, bit for bit
    from gigalens_amd.profiles.light.sersic import Sersic
    mp1 = MC._mp([0.5, 0.5], [2.0])
    single = gl.LensSimulator(PhysicalModel(c["phys"].lenses[:2], [], [Sersic()], multiplane=mp1), cfg, bs=3)
    kw = dict(window=C.GENERAL_WINDOW, num_cells=C.GENERAL_CELLS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = single.image_positions(lt[:2], *src, source_redshifts=[0.8, 2.0], **kw)
        b = single.image_positions(lt[:2], *src, deflection_scale=[mp1.target_scales(0.8)[0], mp1.target_scales(2.0)[0]], **kw)
    for p, q in zip(a, b):
        assert torch.equal(torch.nan_to_num(p), torch.nan_to_num(q))
    with pytest.raises(ValueError, match="source_redshifts"):
        single.image_positions(lt[:2], *src, source_redshifts=[0.8, 0.4], **kw)


def test_native_rules_and_workspace(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.simulator import SimulatorConfig
    L = _native.lib()
    GL_EINVAL, GL_ENOMEM = -1, -4
    c2, c3 = MC.map_case("epl_shear|sie"), MC.map_case("nfw|dpie|sis")
    sim2, sim3 = _sim(gl, "epl_shear|sie", c2["phys_mp"], 3), _sim(gl, "nfw|dpie|sis", c3["phys_mp"], 3)
    plain = gl.LensSimulator(PhysicalModel(c2["phys"].lenses[:2], [], []), SimulatorConfig(delta_pix=0.1, num_pix=8), bs=3)
    h2, h3, h1 = sim2._model._h, sim3._model._h, plain._model._h
    wsb, wsb1 = L.gl_multiplane_image_positions_workspace_bytes, L.gl_image_positions_workspace_bytes
    # 0 for every bad argument, and for a model without planes
    for bad in ((h2, 0, 2, 32, 8), (h2, 3, 0, 32, 8), (h2, 3, 2, 0, 8), (h2, 3, 2, 8193, 8), (h2, 3, 2, 32, 0), (h1, 3, 2, 32, 8),
                (None, 3, 2, 32, 8)):
        assert wsb(*bad) == 0, bad
    # the single-plane size + (K - 1) maps + the coupling rows
    up = lambda v: (v + 255) // 256 * 256
    for B, S, n in ((3, 2, 32), (1, 3, 5), (4, 1, 64)):
        one_map, single = up(B * (n + 1) ** 2 * 8), wsb1(h1, B, S, n, 8)
        for h, K in ((h2, 2), (h3, 3)):
            assert wsb(h, B, S, n, 8) == single + (K - 1) * one_map + up(S * K * 4), (B, S, n, K)
    assert wsb(h3, 3, 2, 32, 8) > wsb(h2, 3, 2, 32, 8) > wsb1(h1, 3, 2, 32, 8)
    # the argument checks of the entry
    packed = sim2._pack_partial({"lens_mass": _lens_t(c2["lens_params"], 3)})
    dev = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=sim2.device)
    sx, sy, out, ni, nd = dev(3, 2), dev(3, 2), dev(3, 2, 8, 3), dev(3, 2, dtype=torch.int32), dev(3, 2, dtype=torch.int32)
    ws = dev(wsb(h2, 3, 2, 32, 8), dtype=torch.uint8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    good_T = np.ascontiguousarray(np.stack([c2["mp"].target_scales(0.8), c2["mp"].target_scales(2.0)]), dtype=np.float32)

    def call(h=h2, T=good_T, K=2, window=(-2.4, 2.4, -2.4, 2.4), n=32, max_images=8, tol=1e-6, max_iter=30, nbytes=None, B=3, S=2):
        T = np.ascontiguousarray(T, dtype=np.float32)
        return L.gl_multiplane_image_positions(h, ptr(packed), B, ptr(sx), ptr(sy), S, T.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), K,
                                               *window, n, max_images, tol, max_iter, ptr(out), ptr(ni), ptr(nd), ptr(ws),
                                               ws.numel() if nbytes is None else nbytes, None)

    assert call() == 0
    assert call(h=h1) == GL_EINVAL and b"gl_model_set_lens_planes has not been called" in L.gl_last_error()
    assert call(K=3, T=np.ones((2, 3))) == GL_EINVAL and b"lens planes" in L.gl_last_error()
    for bad_T in ([[np.nan, 0.5], [1, 0.5]], [[1, 0.5], [np.inf, 0.5]], [[-0.1, 0.5], [1, 0.5]], [[1, 0.5], [0, 0.5]], [[0, 0], [1, 0.5]]):
        assert call(T=bad_T) == GL_EINVAL, bad_T
    for kw in (dict(B=0), dict(S=0), dict(n=0), dict(n=8193), dict(max_images=0), dict(max_images=65), dict(tol=0.0), dict(max_iter=0),
               dict(window=(1.0, 1.0, -1.0, 1.0)), dict(window=(-1.0, 1.0, 2.0, 1.0)), dict(window=(-np.inf, 1.0, -1.0, 1.0))):
        assert call(**kw) == GL_EINVAL, kw
    assert call(nbytes=ws.numel() - 1) == GL_ENOMEM
    # the single-plane entries keep refusing a model with planes
    ws1 = dev(max(wsb1(h2, 3, 2, 32, 8), 256), dtype=torch.uint8)
    rc = L.gl_image_positions(h2, ptr(packed), 3, ptr(sx), ptr(sy), 2, -2.4, 2.4, -2.4, 2.4, 32, 8, 1e-6, 30, ptr(out), ptr(ni), ptr(nd),
                              ptr(ws1), ws1.numel(), None)
    assert rc == _native.GL_EUNSUPPORTED and b"lens planes" in L.gl_last_error()
    torch.cuda.synchronize()
