"""LensSimulator.beta_vjp (gl_lens_maps_vjp): the VJP of the ray-shoot beta = theta - c sum alpha with respect to the lens
parameters, for every built-in mass kind and a dPIE catalogue, against float64 autograd of the oracle's deflection; the skipped
points (zero or non-finite cotangents), the deflection scale, determinism, batch independence and the refusals.

Gate per kind: max(GRAD_RTOL_COL, 4 x the float32 yardstick of that kind), per element relative to its column's scale
(helpers.grad_col_err).  The yardstick is the same oracle code run in float32 on the same draw; 4 x yardstick <= 5e-2 is asserted
on the reference alone."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.potential_cases import KINDS, points_away, row_to_kwargs
from tests.test_gpu_image_positions import _rows, _sim
from tests.test_gpu_parity import GRAD_RTOL_COL

pytestmark = pytest.mark.gpu

B = 3
# one lane; the edges of the wave that owns 64 points; several workgroups; more than 64 partials for the second pass
N_PTS = [1, 63, 64, 65, 257, 4161]
YARD_CAP = 5e-2
# (seed, r_min) of every kind's draw.  The float32 oracle of the NFW family loses digits where a point meets r = Rs (its x = 1
# branch point) or comes close to the centre of a wide halo; these draws keep a halo with Rs inside the point box and hold
# 4 x yardstick under YARD_CAP (a draw that breaks the cap is replaced, the cap stays).
DRAW = {"NFW": (16, 0.2), "NFW_ELLIPSE": (13, 1.0), "TNFW": (16, 0.2)}
DRAW_DEFAULT = (11, 0.2)


def _kind_sim(name):
    from gigalens_amd.profiles.mass import epl, nfw, piemd, piep, shear, sie, sis, tnfw
    cls = {"EPL": epl.EPL, "SIE": sie.SIE, "NFW": nfw.NFW, "SHEAR": shear.Shear, "SIS": sis.SIS, "dPIS": piemd.DPIS,
           "dPIE": piemd.DPIE, "dPIEP": piep.DPIEP, "NFW_ELLIPSE": nfw.NFW_ELLIPSE, "TNFW": tnfw.TNFW}[name]
    return _sim([cls()], 8, 0.2, B)


def _draw(name, seed=None, r_min=None):
    """rows [B, n_par] float32; points [n, B] float32 at least r_min from each sample's centre; cotangents [n, B] with exact zeros."""
    seed = DRAW.get(name, DRAW_DEFAULT)[0] if seed is None else seed
    r_min = DRAW.get(name, DRAW_DEFAULT)[1] if r_min is None else r_min
    r = np.random.default_rng(seed)
    n = max(N_PTS)
    if name == "catalogue":
        rows = np.stack([r.uniform(0.2, 0.35, B), r.uniform(0.15, 0.25, B), r.uniform(1.5, 2.5, B)], 1).astype(np.float32)
        centres = [(0.0, 0.0)] * B
    else:
        rows = np.array([KINDS[name][2](r) for _ in range(B)], dtype=np.float32)
        kws = [row_to_kwargs(name, p) for p in rows]
        centres = [(kw.get("center_x", 0.0), kw.get("center_y", 0.0)) for kw in kws]
    pts = [points_away(r, n, c, r_min=r_min) for c in centres]
    x = np.stack([p[0] for p in pts], 1).astype(np.float32)
    y = np.stack([p[1] for p in pts], 1).astype(np.float32)
    cx, cy = r.standard_normal((n, B)).astype(np.float32), r.standard_normal((n, B)).astype(np.float32)
    for k in (3, 10, 70, 300, 4100):  # both cotangents exactly zero: skipped points
        cx[k], cy[k] = 0.0, 0.0
    cx[5, 1] = 0.0  # one of the two: not skipped
    return rows, x, y, cx, cy


def _oracle_grad(sim, rows, x, y, cx, cy, dtype):
    """[B, lens columns]: autograd of -sum (cx alpha_x + cy alpha_y) through the oracle's deflection, in ``dtype``, on the points
    whose cotangents are not both zero."""
    from oracle import ref_torch as ref
    phys = sim.phys_model
    out = []
    for b in range(rows.shape[0]):
        keep = (cx[:, b] != 0) | (cy[:, b] != 0)
        t = lambda a: torch.as_tensor(np.asarray(a[keep, b], dtype=np.float64)).to(dtype)
        xb, yb, cxb, cyb = t(x), t(y), t(cx), t(cy)
        leaves, tot, k = [], 0, 0
        for prof, c in zip(phys.lenses, phys.lenses_constants):
            kw = {}
            for nme in prof.params:
                v = torch.tensor(float(rows[b, k]), dtype=dtype, requires_grad=True)
                leaves.append(v)
                kw[nme] = v
                k += 1
            kw.update({nme: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype) for nme, v in c.items()})
            ax, ay = ref.mass_deriv(prof, xb, yb, **kw)
            tot = tot - (cxb * ax + cyb * ay).sum()
        g = torch.autograd.grad(tot, leaves)
        out.append([float(v) for v in g])
    return np.asarray(out, dtype=np.float64)


def _t(sim, a):
    return torch.as_tensor(a, device=sim.device)


def _check(name, sim, rows, x, y, cx, cy):
    packed = _rows(sim, rows)
    L = rows.shape[1]
    for n in N_PTS:
        sl = slice(0, n)
        g64 = _oracle_grad(sim, rows, x[sl], y[sl], cx[sl], cy[sl], torch.float64)
        g32 = _oracle_grad(sim, rows, x[sl], y[sl], cx[sl], cy[sl], torch.float32)
        assert np.all(np.isfinite(g64))
        yard = float(H.grad_col_err(g32, g64).max())
        assert 4 * yard <= YARD_CAP, (name, n, yard)  # the draw, not the cap, is what changes if this fails
        gate = max(GRAD_RTOL_COL, 4 * yard)
        g = sim.beta_vjp(_t(sim, x[sl]), _t(sim, y[sl]), packed, _t(sim, cx[sl]), _t(sim, cy[sl]))
        assert g.shape == (B, sim._model.P) and g.dtype == torch.float32
        g = g.cpu().numpy()
        assert np.all(g[:, L:] == 0.0)  # columns of no lens
        err = float(H.grad_col_err(g[:, :L], g64).max())
        print(f"beta_vjp {name} n_pts={n}: error {err:.3g}  gate {gate:.3g}  (float32 yardstick {yard:.3g})")
        assert err <= gate, (name, n, err, gate)


@pytest.mark.parametrize("name", sorted(KINDS))
def test_beta_vjp_matches_f64_autograd(name):
    sim = _kind_sim(name)
    _check(name, sim, *_draw(name))


def test_beta_vjp_catalogue():
    """A dPIE catalogue (GL_SCALED) of 3 members: the member loop on the duals."""
    from gigalens_amd import workloads
    from gigalens_amd.profiles.mass.dpie_subhalo import DPIESubhalo
    cat = workloads.galaxy_catalogue(3, half_width=3.0, seed=4)
    sim = _sim([DPIESubhalo(lum_star=1.0, galaxy_catalogue=cat)], 8, 0.2, B)
    _check("catalogue", sim, *_draw("catalogue", 13))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_point_at_the_centre_with_zero_cotangent_is_skipped():
    """An SIE's deflection has NaN derivatives at its exact centre: with a zero cotangent the point must not reach the sum."""
    sim = _kind_sim("SIE")
    rows, x, y, cx, cy = _draw("SIE", 17)
    n = 64
    x, y, cx, cy = (a[:n + 1].copy() for a in (x, y, cx, cy))
    x[n], y[n] = rows[:, 3], rows[:, 4]  # the float32 centre of every sample, exactly
    cx[n], cy[n] = 0.0, 0.0
    packed = _rows(sim, rows)
    with_pt = sim.beta_vjp(_t(sim, x), _t(sim, y), packed, _t(sim, cx), _t(sim, cy))
    without = sim.beta_vjp(_t(sim, x[:n]), _t(sim, y[:n]), packed, _t(sim, cx[:n]), _t(sim, cy[:n]))
    assert torch.isfinite(with_pt).all()
    assert torch.equal(_bits(with_pt), _bits(without))
    # a cotangent that is not finite is skipped as well
    cx[n, 0], cy[n, 1] = np.nan, np.inf
    again = sim.beta_vjp(_t(sim, x), _t(sim, y), packed, _t(sim, cx), _t(sim, cy))
    assert torch.equal(_bits(again), _bits(without))


def test_deflection_scale_scales_the_gradient():
    sim = _kind_sim("EPL")
    rows, x, y, cx, cy = _draw("EPL", 19)
    n = 257
    packed = _rows(sim, rows)
    args = (_t(sim, x[:n]), _t(sim, y[:n]), packed, _t(sim, cx[:n]), _t(sim, cy[:n]))
    g1 = sim.beta_vjp(*args).cpu().numpy()
    g7 = sim.beta_vjp(*args, deflection_scale=0.7).cpu().numpy()
    # float32(0.7) x every cotangent, each product rounded once: a few ulp of the column's scale after the sum
    assert float(H.grad_col_err(g7[:, :6], np.float64(np.float32(0.7)) * g1[:, :6]).max()) <= 1e-5
    with pytest.raises(ValueError):
        sim.beta_vjp(*args, deflection_scale=-1.0)


def test_deterministic_and_batch_independent():
    sim = _kind_sim("EPL")
    rows, x, y, cx, cy = _draw("EPL", 23)
    n = 4161
    packed = _rows(sim, rows)
    args = [_t(sim, a[:n]) for a in (x, y, cx, cy)]
    a = sim.beta_vjp(args[0], args[1], packed, args[2], args[3])
    b = sim.beta_vjp(args[0], args[1], packed, args[2], args[3])
    assert torch.equal(_bits(a), _bits(b))
    for s in range(B):  # a sample alone gives the bits it has in its batch
        one = sim.beta_vjp(args[0][:, s:s + 1], args[1][:, s:s + 1], packed[s:s + 1], args[2][:, s:s + 1], args[3][:, s:s + 1])
        assert torch.equal(_bits(one[0]), _bits(a[s]))


def test_native_validation_on_a_live_model():
    from gigalens_amd import _native
    sim = _kind_sim("SIS")
    m = sim._model
    L = _native.lib()
    assert L.gl_lens_maps_vjp_workspace_bytes(m._h, 0, 10) == 0
    assert L.gl_lens_maps_vjp_workspace_bytes(m._h, 2, 0) == 0
    need = L.gl_lens_maps_vjp_workspace_bytes(m._h, 2, 65)
    assert need >= 2 * 3 * 2 * 4 and need % 256 == 0
    packed = _rows(sim, np.array([[1.0, 0.0, 0.0]] * 2, np.float32))
    xy = torch.full((65, 2), 0.5, device=sim.device)
    cot = torch.ones((2, 65, 2), device=sim.device)
    out = torch.empty((2, m.P), device=sim.device)
    ws = torch.empty(need, dtype=torch.uint8, device=sim.device)
    p = lambda t: t.data_ptr()
    rc = L.gl_lens_maps_vjp(m._h, p(packed), 2, p(xy), p(xy), 65, 1, p(cot), p(out), p(ws), need - 1, None)
    assert rc == -4 and b"workspace too small" in L.gl_last_error()  # GL_ENOMEM
    assert L.gl_lens_maps_vjp(m._h, p(packed), 2, p(xy), p(xy), 65, 1, p(cot), p(out), p(ws), need, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_refusals():
    from gigalens_amd import _native, workloads
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profile import MassProfile
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.simulator import LensSimulator, SimulatorConfig
    from tests import multilens_cases as MC
    from tests.test_user_profile_compile import SIS_BODY
    # series-expansion lens
    wl = workloads.make("C6S", num_pix=32, batch=2, n_galaxies=8, n_sources=1)
    sim_s = LensSimulator(wl.phys_model, wl.sim_config, bs=2)
    packed_s = H.sample_packed(wl, sim_s, seed=1)
    with pytest.raises(_native.UnsupportedLensError, match="series"):
        sim_s.beta_vjp(0.5, 0.2, packed_s, 1.0, 1.0)

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    sim_u = _sim([UserSIS()], 8, 0.2, 2)
    pu = _rows(sim_u, np.array([[1.0, 0.0, 0.0]] * 2))
    with pytest.raises(_native.UnsupportedLensError, match="user-written"):
        sim_u.beta_vjp(0.5, 0.2, pu, 1.0, 1.0)
    # lens planes
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    sim_p = LensSimulator(PhysicalModel([SIS(), SIS()], [], [Sersic()], multiplane=MC._mp([0.4, 0.9], [2.0])), cfg, bs=2)
    pp = _rows(sim_p, np.array([[1.0, 0.0, 0.0, 0.5, 0.1, 0.1]] * 2))
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim_p.beta_vjp(0.5, 0.2, pp, 1.0, 1.0)
    with pytest.raises(_native.UnsupportedLensError):  # the native refusal itself
        L = _native.lib()
        t = torch.ones((2, 1, 2), device=sim_p.device)
        out = torch.empty((2, sim_p._model.P), device=sim_p.device)
        ws = torch.empty(256, dtype=torch.uint8, device=sim_p.device)
        _native._check_potential(L.gl_lens_maps_vjp(sim_p._model._h, pp.data_ptr(), 2, t.data_ptr(), t.data_ptr(), 1, 1, t.data_ptr(),
                                                    out.data_ptr(), ws.data_ptr(), 256, None))
