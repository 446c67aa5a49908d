"""Arrival times on lens planes on the GPU (csrc/gl_multiplane_fermat.hip.h; ``LensSimulator.time_delays(source_redshifts=...)``,
``fermat_potential(source_redshift=...)``, ``ForwardProbModel.predicted_time_delays`` by redshift on one plane) against the float64 evaluations of tests/mp_tdelay_cases.py.  The kernel's gate: ``KERNEL_GATE`` = 1e-10 of the sum of the
magnitudes of the summands of T, against the host build of its own thread body (tests/test_mp_tdelays_host.py holds that build to the
composed reference without a GPU).  A returned delay adds the float32 rounding of the output, ``F32_OUT`` = 1e-6 relative."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests import mp_images_cases as MI
from tests import mp_tdelay_cases as TD
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


def _packed(sim, lens_params, B=None):
    return sim._pack_partial({"lens_mass": _lens_t(lens_params, B)})


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _dev(sim, a):
    return torch.as_tensor(np.array(a), device=sim.device)


# ---- 1. the kernel on a lattice, against the host build of its thread body ---------------------------------------------------------
@pytest.mark.parametrize("name", MC.MAP_CASES + (TD.FOUR_PLANES,))  # (the last: K = 4 = MP_MAXK, B = 1, sources behind 1 .. 4 planes)
def test_multiplane_fermat_on_a_lattice(gl, name):
    d = TD.lattice_data(name)
    c = d["case"]
    B, S = d["x"].shape[:2]
    assert (B, S) == ((1, 4) if name == TD.FOUR_PLANES else (3, 2))
    sim = _sim(gl, name, c["phys_mp"], B)
    packed = _packed(sim, d["lens_params"])
    T = sim._model.multiplane_fermat(packed, _dev(sim, d["x"]), _dev(sim, d["y"]), _dev(sim, d["sx"]), _dev(sim, d["sy"]), d["geom"],
                                     d["pot"])
    assert T.dtype == torch.float64 and tuple(T.shape) == d["x"].shape
    host, terms = d["host"]
    err = TD.relative_to_terms(T.cpu().numpy(), host, terms)
    print(f"{name}: kernel against the host build {err:.2e} of the terms (gate {TD.KERNEL_GATE:.0e}); against the composed reference "
          f"{TD.relative_to_terms(T.cpu().numpy(), d['ref'][0], terms):.2e}")
    assert err <= TD.KERNEL_GATE
    # fermat_potential(source_redshift=...): every point the one image of a source of its own -- the same threads, the same bits
    z = d["z"]
    for s in range(S):
        x, y = _dev(sim, d["x"][:, s].T), _dev(sim, d["y"][:, s].T)  # [n, B]: trailing axis = batch
        phi = sim.fermat_potential(x, y, _dev(sim, d["sx"][:, s]), _dev(sim, d["sy"][:, s]), _lens_t(d["lens_params"]), source_redshift=z[s])
        assert phi.dtype == torch.float64 and tuple(phi.shape) == (TD.N_LATTICE, B)
        assert torch.equal(_bits(phi), _bits(T[:, s].t()))


# ---- 2. time_delays(source_redshifts=...) on the general cases of the solver ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MI.GENERAL))
def test_time_delays_on_the_general_cases(gl, name):
    from gigalens_amd.cosmology import hubble_distance_mpc
    c = MC.map_case(name)
    z, sx, sy = MI.general_sources(name)
    sim = _sim(gl, name, c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"])
    kw = dict(window=MI.GENERAL_WINDOW, num_cells=MI.GENERAL_CELLS, source_redshifts=z)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        solver = sim.image_positions(lt, torch.as_tensor(sx), torch.as_tensor(sy), **kw)
        x, y, mu, n, dt = sim.time_delays(lt, torch.as_tensor(sx), torch.as_tensor(sy), **kw)
        days = sim.time_delays(lt, torch.as_tensor(sx), torch.as_tensor(sy), h0=70.0, **kw)[4]
    for got, want in zip((x, y, mu, n), solver):
        assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))
    assert dt.dtype == torch.float32 and tuple(dt.shape) == tuple(x.shape)
    assert torch.equal(torch.isnan(dt), torch.isnan(x))
    ok = ~torch.isnan(x)
    assert bool((dt[ok] >= 0).all())
    assert torch.equal((dt == 0).sum(dim=2), (n >= 1).to(torch.int64))  # the earliest image, and it alone
    assert int(n.max()) >= 3
    # the reference at the returned positions
    xn, yn, okn = x.cpu().numpy(), y.cpu().numpy(), ok.cpu().numpy()
    geom, pot = TD.weights(c["mp"], z)
    Tr, terms = TD.reference_T(c["phys"], c["mp"], c["lens_params"], np.where(okn, xn, 0.0), np.where(okn, yn, 0.0), sx, sy, geom, pot)
    Tr, terms = np.where(okn, Tr, np.inf), np.where(okn, terms, 0.0)
    first = np.argmin(Tr, axis=2)[..., None]
    want = Tr - np.take_along_axis(Tr, first, axis=2)
    tol = TD.KERNEL_GATE * (terms + np.take_along_axis(terms, first, axis=2)) + TD.F32_OUT * np.abs(want)
    got = dt.cpu().numpy().astype(np.float64)
    worst = np.max(np.where(okn, np.abs(got - np.where(okn, want, 0.0)) / np.where(okn & (tol > 0), tol, 1.0), 0.0))
    print(f"{name}: images per pair {n.cpu().tolist()}, largest |dt - reference| / tolerance {worst:.2e}, largest dt {np.nanmax(got):.4f}")
    assert np.all(np.abs(got - want)[okn] <= tol[okn])
    # days
    scale = hubble_distance_mpc(70.0) * gl.LensSimulator.DAYS_PER_MPC_ARCSEC2
    dn = days.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(dn), ~okn) and np.all(np.abs(dn - got * scale)[okn] <= 1e-6 * (got * scale)[okn])


# ---- 3. closed forms ----------------------------------------------------------------------------------------------------------------------
def test_sis_closed_form_through_time_delays(gl):
    """``T(-) - T(+) = g_1 2 theta_E beta`` (mp_tdelay_cases.sis_case) to 1e-6: float32 output rounding is 6e-8, and the position error
    of the solver enters at second order -- the images are stationary points of T."""
    phys, phys_mp, mp, lp = TD.sis_case()
    sim = _sim(gl, "sis|empty", phys_mp, 1)
    x, y, mu, n, dt = sim.time_delays(_lens_t(lp), torch.as_tensor([[float(TD.SIS_BETA)]]), torch.as_tensor([[0.0]]),
                                      source_redshifts=mp.z_ref, window=TD.SIS_WINDOW, num_cells=TD.SIS_CELLS, strict=True)
    assert n.cpu().tolist() == [[2]]
    xs = x[0, 0, :2].cpu().numpy()
    assert abs(xs[0] - (float(TD.SIS_BETA) - float(TD.SIS_THETA_E))) <= 5e-5 and abs(xs[1] - (float(TD.SIS_BETA) + float(TD.SIS_THETA_E))) <= 5e-5
    want = TD.sis_closed_form(mp)
    got = dt[0, 0, :2].cpu().numpy().astype(np.float64)
    print(f"dt = {got.tolist()}, closed form {want:.9g}")
    assert got[1] == 0.0 and abs(got[0] - want) <= 1e-6 * want


def test_one_plane_multiplane_takes_the_scaled_single_plane_path(gl):
    """A one-plane ``MultiPlane``: the source's ``deflection_scale`` c on the single-plane solver and potential, times ``geom[0]`` --
    behind an SIS ``T(-) - T(+) = g 2 (c theta_E) beta``."""
    from gigalens_amd.cosmology import MultiPlane
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    mp = MultiPlane([0.5], [], MC.Z_REF)
    sim = _sim(gl, "sis one plane", PhysicalModel([SIS()], [], [], multiplane=mp), 1)
    lp = [{"theta_E": MC._f32(1.0), "center_x": MC._f32(0.0), "center_y": MC._f32(0.0)}]
    z_s, beta = 1.5, 0.25
    x, y, mu, n, dt = sim.time_delays(_lens_t(lp), torch.as_tensor([[beta]]), torch.as_tensor([[0.0]]), source_redshifts=z_s,
                                      window=TD.SIS_WINDOW, num_cells=TD.SIS_CELLS, strict=True)
    (g,), _ = mp.delay_weights(z_s)
    want = g * 2.0 * float(np.float32(mp.target_scales(z_s)[0])) * beta
    assert n.cpu().tolist() == [[2]] and float(dt[0, 0, 1]) == 0.0 and abs(float(dt[0, 0, 0]) - want) <= 1e-6 * want


# ---- 4. image families placed by redshift ---------------------------------------------------------------------------------------------
def test_family_by_redshift_on_a_one_plane_multiplane(gl):
    """``predicted_time_delays`` of a family on a scaled source plane (``centroids_redshifts`` on a one-plane ``MultiPlane``), which was
    refused before: the images ``beta +- c theta_E`` of an SIS as observed images; the call equals ``time_delays`` for the barycentre
    source bit for bit, and ``dt = g 2 (c theta_E) beta`` in days.  On several lens planes the family calls stay refused
    (tests/test_gpu_mp_positions.py)."""
    from gigalens_amd import prior as tfd
    from gigalens_amd.cosmology import MultiPlane, hubble_distance_mpc
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    mp = MultiPlane([0.5], [], MC.Z_REF)
    sim = _sim(gl, "sis one plane", PhysicalModel([SIS()], [], [], multiplane=mp), 1)
    lp = [{"theta_E": MC._f32(1.0), "center_x": MC._f32(0.0), "center_y": MC._f32(0.0)}]
    z_s, beta = 1.5, 0.25
    c = float(np.float32(mp.target_scales(z_s)[0]))
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), 0.01) for k, v in d.items()}) for d in lp])))
    cx, cy = np.asarray([beta - c, beta + c], dtype=np.float32), np.zeros(2, dtype=np.float32)
    pm = gl.ForwardProbModel(prior, include_pixels=False, centroids_x=[cx], centroids_y=[cy], centroids_errors_x=[np.float32(0.05)],
                             centroids_errors_y=[np.float32(0.05)], centroids_redshifts=[z_s])
    packed = _packed(sim, lp)
    kw = dict(window=TD.SIS_WINDOW, num_cells=TD.SIS_CELLS)
    sx, sy = pm._family_sources(sim, packed)
    assert abs(float(sx[0, 0]) - beta) <= 1e-6 and abs(float(sy[0, 0])) <= 1e-6
    (tx, ty, tmu, tn, tdt), = pm.predicted_time_delays(sim, packed, h0=70.0, **kw)
    direct = sim.time_delays(packed, sx, sy, source_redshifts=[z_s], h0=70.0, **kw)
    for a, b in zip((tx, ty, tmu, tn, tdt), direct):
        assert torch.equal(_bits(a), _bits(b[:, 0]))
    (g,), _ = mp.delay_weights(z_s)
    want = g * 2.0 * c * beta * hubble_distance_mpc(70.0) * gl.LensSimulator.DAYS_PER_MPC_ARCSEC2
    print(f"dt = {tdt[0, :2].cpu().tolist()} days, closed form {want:.6f}")
    assert int(tn[0]) == 2 and float(tdt[0, 1]) == 0.0 and abs(float(tdt[0, 0]) - want) <= 1e-5 * want
    with pytest.raises(ValueError, match="time_delay_distance"):
        pm.predicted_time_delays(sim, packed, time_delay_distance=2000.0, **kw)


# ---- 5. launch edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,M", [(1, 1, 1), (3, 1, 21), (1, 2, 32), (1, 5, 13), (3, 1, 43)])  # B S M = 1, 63, 64, 65, 129
def test_launch_edges(gl, B, S, M):
    c = MC.map_case("nfw|dpie|sis")
    sim = _sim(gl, "nfw|dpie|sis", c["phys_mp"], B)
    lp = MC.sample_rows(c["lens_params"], B)
    packed = _packed(sim, lp)
    px, py = MC.points(M)
    x = np.ascontiguousarray(np.broadcast_to(px, (B, S, M)))
    y = np.ascontiguousarray(np.broadcast_to(py, (B, S, M)))
    sx = (0.01 * np.arange(B * S, dtype=np.float32) - 0.02).reshape(B, S)
    sy = (0.03 - 0.015 * np.arange(B * S, dtype=np.float32)).reshape(B, S)
    geom, pot = TD.weights(c["mp"], [(1.1, 2.5, 0.5, 3.5, 1.0)[s] for s in range(S)])
    call = lambda xx: sim._model.multiplane_fermat(packed, _dev(sim, xx), _dev(sim, y), _dev(sim, sx), _dev(sim, sy), geom, pot)
    T = call(x)
    host, terms = TD.host_T(c["phys"], c["mp"], lp, x, y, sx, sy, geom, pot)
    err = TD.relative_to_terms(T.cpu().numpy(), host, terms)
    print(f"B S M = {B} x {S} x {M}: kernel against the host build {err:.2e}")
    assert bool(torch.isfinite(T).all()) and err <= TD.KERNEL_GATE
    assert torch.equal(_bits(call(x)), _bits(T))  # two calls: identical bits
    hole = x.copy()
    hole.reshape(-1)[(B * S * M) // 2] = np.nan
    Th = call(hole)
    keep = torch.ones(B * S * M, dtype=torch.bool, device=T.device)
    keep[(B * S * M) // 2] = False
    assert bool(torch.isnan(Th.reshape(-1)[~keep]).all())
    assert torch.equal(_bits(Th.reshape(-1)[keep]), _bits(T.reshape(-1)[keep]))


# ---- 6. refusals: all of them before any launch -------------------------------------------------------------------------------------------
def test_refusals(gl):
    from gigalens_amd import _native
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass import Interpolated
    from gigalens_amd.profiles.mass.dpie_series import DPIESeries
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import SimulatorConfig
    c = MC.map_case("epl_shear|sie")
    z, sx, sy = MI.general_sources("epl_shear|sie")
    sim = _sim(gl, "epl_shear|sie", c["phys_mp"], 3)
    lt = _lens_t(c["lens_params"])
    sxt, syt = torch.as_tensor(sx), torch.as_tensor(sy)
    # the simulator
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim.time_delays(lt, sxt, syt)
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim.fermat_potential(torch.zeros(4, 3), torch.zeros(4, 3), 0.1, 0.1, lt)
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim.potential(torch.zeros(4, 3), torch.zeros(4, 3), lt)
    with pytest.raises(ValueError, match="time_delay_distance"):
        sim.time_delays(lt, sxt, syt, source_redshifts=z, time_delay_distance=2000.0)
    with pytest.raises(ValueError, match="h0"):
        sim.time_delays(lt, sxt, syt, h0=70.0)
    with pytest.raises(ValueError, match="h0"):
        sim.time_delays(lt, sxt, syt, source_redshifts=z, h0=-70.0)
    single = gl.LensSimulator(c["phys"], SimulatorConfig(delta_pix=0.1, num_pix=8), bs=3)
    with pytest.raises(ValueError, match="h0"):
        single.time_delays(lt, sxt, syt, h0=70.0)
    with pytest.raises(ValueError, match="MultiPlane"):
        single.time_delays(lt, sxt, syt, source_redshifts=z)
    packed = _packed(sim, c["lens_params"])
    with pytest.raises(NotImplementedError):
        sim.time_delays(packed.clone().requires_grad_(True), sxt, syt, source_redshifts=z)
    with pytest.raises(NotImplementedError):
        sim.time_delays(lt, sxt.clone().requires_grad_(True), syt, source_redshifts=z)
    with pytest.raises(NotImplementedError):
        sim.fermat_potential(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(3, requires_grad=True), 0.1, lt, source_redshift=2.0)
    # a series expansion or an interpolated lens on a plane: no such model exists
    cfg, mp = SimulatorConfig(delta_pix=0.1, num_pix=8), MC._mp([0.4, 0.9])
    flat = np.zeros((5, 5), dtype=np.float32)
    for second in (DPIESeries(2), Interpolated(flat, flat, 0.1)):
        with pytest.raises(_native.UnsupportedLensError):
            gl.LensSimulator(PhysicalModel([SIS(), second], [], [], multiplane=mp), cfg, bs=1)
    # the C entry: nothing is launched (the output keeps its fill)
    L, P = _native.lib(), (lambda t: ctypes.c_void_p(t.data_ptr()))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    h, dev = sim._model._h, sim.device
    x = torch.zeros((3, 2, 4), device=dev)
    sxd, syd = sxt.to(dev), syt.to(dev)
    out = torch.full((3, 2, 4), 7.0, dtype=torch.float64, device=dev)
    geom, pot = TD.weights(c["mp"], z)
    nbytes = L.gl_multiplane_fermat_workspace_bytes(h, 2)
    assert nbytes > 0 and L.gl_multiplane_fermat_workspace_bytes(h, 0) == 0
    assert L.gl_multiplane_fermat_workspace_bytes(single._model._h, 2) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call = lambda hh=h, g=geom, v=pot, K=2, nb=nbytes: L.gl_multiplane_fermat(hh, P(packed), 3, P(x), P(x), P(sxd), P(syd), 2, 4, dp(g), dp(v),
                                                                             K, P(out), P(ws), nb, None)
    assert call(hh=single._model._h) == -1 and b"gl_model_set_lens_planes has not been called" in L.gl_last_error()
    g3, v3 = np.zeros((2, 3)), np.ones(3)
    g3[:, 0] = 1.0
    assert call(g=g3, v=v3, K=3) == -1 and b"lens planes" in L.gl_last_error()  # a wrong K
    for i, j, v in ((0, 0, np.nan), (1, 1, -0.5), (1, 0, np.inf)):
        g = geom.copy()
        g[i, j] = v
        assert call(g=g) == -1, (i, j, v)
    behind_a_zero = np.ascontiguousarray([[0.0, 0.5], [1.0, 1.0]])
    assert call(g=behind_a_zero) == -1
    assert call(g=np.zeros((2, 2))) == -1 and b"every geometric weight is zero" in L.gl_last_error()
    for bad in (np.asarray([np.nan, 1.0]), np.asarray([1.0, -1.0])):
        assert call(v=bad) == -1
    assert call(nb=nbytes - 1) == -1 and b"workspace too small" in L.gl_last_error()
    assert L.gl_multiplane_fermat(h, P(packed), 3, P(x), P(x), P(sxd), P(syd), 2, 4, dp(geom), dp(pot), 2, P(out), None, 0, None) == -1
    assert L.gl_multiplane_fermat(h, None, 3, P(x), P(x), P(sxd), P(syd), 2, 4, dp(geom), dp(pot), 2, P(out), P(ws), nbytes, None) == -1
    assert L.gl_multiplane_fermat(h, P(packed), 0, P(x), P(x), P(sxd), P(syd), 2, 4, dp(geom), dp(pot), 2, P(out), P(ws), nbytes, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # ... and the binding's own shape checks
    with pytest.raises(_native.NativeLibraryError):
        sim._model.multiplane_fermat(packed, x, x, sxd, syd, geom[:1], pot)
    # gl_lens_potential keeps refusing planes
    with pytest.raises(_native.UnsupportedLensError):
        sim._model.lens_potential(packed, torch.zeros(4, 3, device=dev), torch.zeros(4, 3, device=dev))
    # the family calls of a ForwardProbModel keep refusing lens planes: tests/test_gpu_mp_positions.py
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())
