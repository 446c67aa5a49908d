"""LensSimulator.hessian_vjp (gl_lens_hessian_vjp): the VJP of the summed Hessian f_xx, f_xy, f_yx, f_yy of the lens maps with respect
to the lens parameters, for every built-in mass kind (the NFW family inside and outside its scale radius) and a dPIE catalogue,
against float64 autograd of the restatement in tests/shear_cases.py; consistency with the det A adjoint of the image-position
likelihood and with the convergence; the skipped points, the deflection scale, determinism, batch independence and the refusals.

Gate per draw: max(GRAD_RTOL_COL, 4 x the float32 yardstick of that draw), per element relative to its column's scale
(helpers.grad_col_err); 4 x yardstick <= 5e-2 is asserted on the reference alone.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests import flux_cases as FC
from tests import helpers as H
from tests import mp_positions_cases as PC
from tests import shear_cases as SC
from tests.test_gpu_image_positions import _rows, _sim
from tests.test_gpu_multilens_grad import _prior_of, _t as _struct_t
from tests.test_gpu_parity import GRAD_RTOL_COL

pytestmark = pytest.mark.gpu

B = SC.B
_SIMS = {}


def _kind_sim(kind):
    """One simulator per kind (a Sersic source behind the lens: packed columns that belong to no lens)."""
    if kind not in _SIMS:
        _SIMS[kind] = _sim(SC.kind_lenses(kind), 8, 0.2, B)
    return _SIMS[kind]


def _t(sim, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=sim.device)


def _vjp(sim, packed, x, y, cot, **kw):
    return sim.hessian_vjp(_t(sim, x), _t(sim, y), packed, *[_t(sim, c) for c in cot], **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("label", sorted(SC.DRAWS))
def test_hessian_vjp_matches_f64_autograd(label):
    kind, rows, x, y, cot, ref = SC.vjp_data(label)
    sim = _kind_sim(kind)
    packed = _rows(sim, rows)
    L = rows.shape[1]
    for n in SC.N_PTS:
        g64, yard = ref[n]
        assert np.all(np.isfinite(g64))
        assert 4 * yard <= SC.YARD_CAP, (label, n, yard)  # the draw, not the cap, is what changes if this fails
        gate = max(GRAD_RTOL_COL, 4 * yard)
        g = _vjp(sim, packed, x[:n], y[:n], cot[:, :n])
        assert g.shape == (B, sim._model.P) and g.dtype == torch.float32
        g = g.cpu().numpy()
        assert np.all(g[:, L:] == 0.0)  # columns of no lens
        err = float(H.grad_col_err(g[:, :L], g64).max())
        print(f"hessian_vjp {label} n_pts={n}: error {err:.3g}  gate {gate:.3g}  (float32 yardstick {yard:.3g})")
        assert err <= gate, (label, n, err, gate)


def test_half_trace_cotangents_give_the_gradient_of_the_convergence():
    """Cotangents (1/2, 0, 0, 1/2) on a dPIS (its convergence excess is part of f_xx and f_yy): d sum kappa / d params."""
    kind, rows, x, y, _, _ = SC.vjp_data("dPIS")
    n = 257
    cot = np.zeros((4, n, B), np.float32)
    cot[0], cot[3] = 0.5, 0.5
    phys = SC.kind_phys(kind)
    g64 = SC.hessian_vjp(phys, rows, x[:n], y[:n], cot, SC.F64)
    yard = float(H.grad_col_err(SC.hessian_vjp(phys, rows, x[:n], y[:n], cot, SC.F32), g64).max())
    assert 4 * yard <= SC.YARD_CAP
    sim = _kind_sim(kind)
    g = sim.hessian_vjp(_t(sim, x[:n]), _t(sim, y[:n]), _rows(sim, rows), 0.5, 0.0, 0.0, 0.5).cpu().numpy()  # scalars broadcast
    err, gate = float(H.grad_col_err(g[:, :rows.shape[1]], g64).max()), max(GRAD_RTOL_COL, 4 * yard)
    print(f"d sum kappa / d params (dPIS): error {err:.3g}  gate {gate:.3g}  (float32 yardstick {yard:.3g})")
    assert err <= gate


def test_det_adjoint_of_the_position_likelihood():
    """The gradient of the image-position likelihood is the ray-shoot VJP of its beta adjoints plus the Hessian VJP of its det A
    adjoint: with the cotangents d ll/d det x (-(1 - f_yy), -f_yx, -f_xy, -(1 - f_xx)) at the images of the ``plain`` families of
    tests/flux_cases.py, ``hessian_vjp`` equals gl_positions_fwd_bwd's gradient with the beta part (``beta_vjp``) removed."""
    from gigalens_amd.model import ForwardProbModel
    from gigalens_amd.simulator import LensSimulator, SimulatorConfig
    c = FC.case("plain")
    sim = LensSimulator(c["phys"], SimulatorConfig(delta_pix=0.1, num_pix=8), bs=c["B"])
    fams = c["fams"]
    pm = ForwardProbModel(_prior_of({"lens_mass": c["params"]["lens_mass"]}), include_pixels=False,
                          centroids_x=[f["x"] for f in fams], centroids_y=[f["y"] for f in fams],
                          centroids_errors_x=[f["ex"] for f in fams], centroids_errors_y=[f["ey"] for f in fams])
    packed = sim.pack(_struct_t(c["params"]))
    _, _, g_pos = pm._bind_positions(sim).positions(packed, True)
    px, py = np.concatenate([f["x"] for f in fams]), np.concatenate([f["y"] for f in fams])
    xs = _t(sim, np.repeat(px[:, None], c["B"], 1))
    ys = _t(sim, np.repeat(py[:, None], c["B"], 1))
    m = sim._lens_maps(xs, ys, packed).double().cpu().numpy()  # [6, J, B]
    adj_b, adj_d, j0 = np.zeros((2,) + m.shape[1:]), np.zeros(m.shape[1:]), 0
    det = (1 - m[2]) * (1 - m[5]) - m[3] * m[4]
    for f in fams:  # the adjoints of gl_pos_p2_kernel, in float64 on the maps the kernels return
        sl = slice(j0, j0 + f["x"].size)
        j0 += f["x"].size
        ex, ey = np.float64(f["ex"])[:, None] * det[sl], np.float64(f["ey"])[:, None] * det[sl]
        rx, ry = (m[0, sl] - m[0, sl].mean(0)) / ex, (m[1, sl] - m[1, sl].mean(0)) / ey
        adj_b[0, sl], adj_b[1, sl] = -rx / ex + (rx / ex).mean(0), -ry / ey + (ry / ey).mean(0)
        adj_d[sl] = -(2 - rx ** 2 - ry ** 2) / det[sl]
    f32 = lambda a: _t(sim, a.astype(np.float32))
    g_beta = sim.beta_vjp(xs, ys, packed, f32(adj_b[0]), f32(adj_b[1]))
    cot = [-(1 - m[5]) * adj_d, -m[4] * adj_d, -m[3] * adj_d, -(1 - m[2]) * adj_d]
    g_det = sim.hessian_vjp(xs, ys, packed, *[f32(v) for v in cot])
    want = (g_pos.double() - g_beta.double()).cpu().numpy()
    worst = PC.grad_gate(g_det.cpu().numpy(), want)
    share = float(np.abs(want).max() / np.abs(g_pos.cpu().numpy()).max())
    print(f"det A part of the position gradient: worst element {worst:.3f} of the gate (det part / whole gradient {share:.3g})")
    assert worst <= 1.0


def test_points_with_zero_or_non_finite_cotangents_are_skipped():
    """An SIE's Hessian has NaN derivatives at its exact centre: with four zero cotangents the point must not reach the sum."""
    sim = _kind_sim("SIE")
    rows, x, y, cot = SC.draw("SIE", None, 0.2, 37, n=65)
    n = 64
    x[n], y[n] = rows[:, 3], rows[:, 4]  # the float32 centre of every sample, exactly
    cot[:, n] = 0.0
    packed = _rows(sim, rows)
    with_pt = _vjp(sim, packed, x, y, cot)
    without = _vjp(sim, packed, x[:n], y[:n], cot[:, :n])
    assert torch.isfinite(with_pt).all()
    assert torch.equal(_bits(with_pt), _bits(without))
    for k, bad in enumerate((np.nan, np.inf, -np.inf, np.nan)):  # one cotangent of the four not finite: skipped as well
        c2 = cot.copy()
        c2[:, n] = 1.0
        c2[k, n, k % B] = bad
        c2[:, n, [(k + 1) % B, (k + 2) % B]] = 0.0
        assert torch.equal(_bits(_vjp(sim, packed, x, y, c2)), _bits(without)), k
    # one non-zero cotangent of the four, away from the centre: not skipped
    x[n], y[n] = rows[:, 3] + 0.5, rows[:, 4] - 0.25
    for k in range(4):
        c2 = cot.copy()
        c2[k, n] = 1.0
        g = _vjp(sim, packed, x, y, c2)
        assert torch.isfinite(g).all() and not torch.equal(_bits(g), _bits(without)), k


def test_deflection_scale_scales_the_gradient():
    sim = _kind_sim("EPL")
    rows, x, y, cot = SC.draw("EPL", None, 0.2, 39, n=257)
    packed = _rows(sim, rows)
    g1 = _vjp(sim, packed, x, y, cot).cpu().numpy()
    g7 = _vjp(sim, packed, x, y, cot, deflection_scale=0.7).cpu().numpy()
    # float32(0.7) x every cotangent, each product rounded once: a few ulp of the column's scale after the sum
    assert float(H.grad_col_err(g7[:, :6], np.float64(np.float32(0.7)) * g1[:, :6]).max()) <= 1e-5
    with pytest.raises(ValueError):
        _vjp(sim, packed, x, y, cot, deflection_scale=-1.0)


def test_deterministic_and_batch_independent():
    sim = _kind_sim("EPL")
    rows, x, y, cot = SC.draw("EPL", None, 0.2, 43)
    packed = _rows(sim, rows)
    a = _vjp(sim, packed, x, y, cot)
    b = _vjp(sim, packed, x, y, cot)
    assert torch.equal(_bits(a), _bits(b))
    for s in range(B):  # a sample alone gives the bits it has in its batch
        one = _vjp(sim, packed[s:s + 1], x[:, s:s + 1], y[:, s:s + 1], cot[:, :, s:s + 1])
        assert torch.equal(_bits(one[0]), _bits(a[s]))


def test_native_validation_on_a_live_model():
    from gigalens_amd import _native
    sim = _kind_sim("SIS")
    m = sim._model
    L = _native.lib()
    assert L.gl_lens_hessian_vjp_workspace_bytes(m._h, 0, 10) == 0
    assert L.gl_lens_hessian_vjp_workspace_bytes(m._h, 2, 0) == 0
    need = L.gl_lens_hessian_vjp_workspace_bytes(m._h, 2, 65)
    assert need >= 2 * 3 * 2 * 4 and need % 256 == 0
    packed = _rows(sim, np.array([[1.0, 0.0, 0.0]] * 2, np.float32))
    xy = torch.full((65, 2), 0.5, device=sim.device)
    cot = torch.ones((4, 65, 2), device=sim.device)
    out = torch.empty((2, m.P), device=sim.device)
    ws = torch.empty(need, dtype=torch.uint8, device=sim.device)
    p = lambda t: t.data_ptr()
    rc = L.gl_lens_hessian_vjp(m._h, p(packed), 2, p(xy), p(xy), 65, 1, p(cot), p(out), p(ws), need - 1, None)
    assert rc == -4 and b"workspace too small" in L.gl_last_error()  # GL_ENOMEM
    assert L.gl_lens_hessian_vjp(m._h, p(packed), 2, p(xy), p(xy), 65, 1, p(cot), p(out), p(ws), need, None) == 0
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
    one = (1.0, 0.0, 0.0, 1.0)
    # series-expansion lens
    wl = workloads.make("C6S", num_pix=32, batch=2, n_galaxies=8, n_sources=1)
    sim_s = LensSimulator(wl.phys_model, wl.sim_config, bs=2)
    packed_s = H.sample_packed(wl, sim_s, seed=1)
    with pytest.raises(_native.UnsupportedLensError, match="series"):
        sim_s.hessian_vjp(0.5, 0.2, packed_s, *one)

    class UserSIS(MassProfile):
        _name, _params = "USER_SIS", ["theta_E", "center_x", "center_y"]
        hip_body = SIS_BODY

    sim_u = _sim([UserSIS()], 8, 0.2, 2)
    pu = _rows(sim_u, np.array([[1.0, 0.0, 0.0]] * 2))
    with pytest.raises(_native.UnsupportedLensError, match="user-written"):
        sim_u.hessian_vjp(0.5, 0.2, pu, *one)
    # lens planes
    cfg = SimulatorConfig(delta_pix=0.1, num_pix=8)
    sim_p = LensSimulator(PhysicalModel([SIS(), SIS()], [], [Sersic()], multiplane=MC._mp([0.4, 0.9], [2.0])), cfg, bs=2)
    pp = _rows(sim_p, np.array([[1.0, 0.0, 0.0, 0.5, 0.1, 0.1]] * 2))
    with pytest.raises(_native.UnsupportedLensError, match="lens planes"):
        sim_p.hessian_vjp(0.5, 0.2, pp, *one)
    with pytest.raises(_native.UnsupportedLensError):  # the native refusal itself
        L = _native.lib()
        t = torch.ones((4, 1, 2), device=sim_p.device)
        out = torch.empty((2, sim_p._model.P), device=sim_p.device)
        ws = torch.empty(256, dtype=torch.uint8, device=sim_p.device)
        _native._check_potential(L.gl_lens_hessian_vjp(sim_p._model._h, pp.data_ptr(), 2, t.data_ptr(), t.data_ptr(), 1, 1, t.data_ptr(),
                                                       out.data_ptr(), ws.data_ptr(), 256, None))
