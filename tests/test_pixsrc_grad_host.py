"""Host checks (no GPU) of the evidence gradient: the two-stage float64 oracle of tests/pixsrc_grad_cases.py against the
restatement's evidence and against central differences, the closed form of dE/dF, the convention on rays that are not finite, and
the boundary of the new C entries (symbols, argument validation without a device)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import pixsrc_cases as PC
from tests import pixsrc_grad_cases as GC


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


@pytest.mark.parametrize("name", PC.CASES)
def test_oracle_evidence_is_the_restatements(name):
    c, obs, err, lam, o64, _ = GC.case_oracle(name)
    ref = PC.data(name)[3]["log_evidence"]
    ref = ref[:, 1] if ref.ndim == 2 else ref
    d = np.abs(o64["E"] - ref).max()
    print(f"{name}: |E - log_evidence| = {d:.3g}")
    assert d <= 1e-9 * (1 + np.abs(ref).max())


@pytest.mark.parametrize("name", ["A", "B", "C11", "C21"])
def test_oracle_gradient_equals_central_differences(name):
    """h = 1e-6 in float64: truncation ~ h^2 E''' and rounding ~ 1e-16 |E| / h stay far below 1e-5 of a column's scale as long as no
    ray crosses a grid line inside +-h (the rays are >= 1e-4 from the lines, asserted in the GPU test of the conditions)."""
    c, obs, err, lam, o64, _ = GC.case_oracle(name)
    h, worst = 1e-6, 0.0

    def fd(params=None, plus=None, minus=None, dpose=None):
        if dpose is not None:
            return (GC.evidence_only(c, obs, err, lam, dpose=dpose) - GC.evidence_only(c, obs, err, lam, dpose=tuple(-v for v in dpose))) / (2 * h)
        return (GC.evidence_only(c, obs, err, lam, params=plus) - GC.evidence_only(c, obs, err, lam, params=minus)) / (2 * h)

    for grp, key in (("lens_mass", "grad_lens"), ("lens_light", "grad_light")):
        for i, d in enumerate(c["params"].get(grp, [])):
            for k in d:
                plus, minus = copy.deepcopy(c["params"]), copy.deepcopy(c["params"])
                base = np.broadcast_to(np.asarray(d[k], dtype=np.float32), (c["B"],)).astype(np.float64)
                plus[grp][i][k], minus[grp][i][k] = base + h, base - h  # float64: kept as they are
                got, want = o64[key][i][k], fd(plus=plus, minus=minus)
                e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
                worst = max(worst, e)
                assert e <= 1e-5, (name, grp, i, k, got, want)
    for j in range(3):
        dp = [0.0, 0.0, 0.0]
        dp[j] = h
        got, want = o64["grad_pose"][:, j], fd(dpose=tuple(dp))
        e = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        worst = max(worst, e)
        assert e <= 1e-5, (name, "pose", j, got, want)
    print(f"{name}: worst |autograd - central difference| / column scale = {worst:.3g}")


def test_case_d_convention():
    """D is left out of the central differences: moving e1 of its e = 0 sample, or the centre of its pixel-centred sample, makes NaN
    rays finite and E itself jumps.  The convention instead: the all-NaN sample has an exactly zero gradient, the others are finite."""
    c, obs, err, lam, o64, _ = GC.case_oracle("D")
    for d in o64["grad_lens"]:
        for k, v in d.items():
            assert v[1] == 0.0 and np.all(np.isfinite(v)), (k, v)
    assert np.all(o64["grad_beta"][:, 1] == 0.0) and np.all(o64["grad_pose"][1] == 0.0)
    assert np.all(np.isfinite(o64["grad_beta"])) and np.abs(o64["grad_beta"][:, 0]).max() > 0 and np.abs(o64["grad_beta"][:, 2]).max() > 0


def test_closed_form_dE_dF_equals_autograd():
    """dE/dF = D (rw s^T - Fw M^-1), against autograd with F itself as the leaf (case A, sample 0)."""
    c, obs, err, lam, o64, _ = GC.case_oracle("A")
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(c["phys"], c["cfg"], 1, dtype=GC.F64, supersampled_kernel=c["psf"])
    kw = c["kw"]
    H, W = rs.wcs.n_x, rs.wcs.n_y
    fx, fy = (torch.as_tensor(r[:, 0]) for r in o64["rays"])
    finite = torch.isfinite(fx) & torch.isfinite(fy)
    far = torch.full_like(fx, GC.FAR)
    L = PC.mapping(torch.where(finite, fx, far), torch.where(finite, fy, far), kw["n_src"], kw["pitch"][0], kw["center"][0][0], kw["center"][1][0])
    pix = torch.from_numpy(PC.used_pixels(rs, kw["mask"]).astype(np.int64))
    tp = GC._tparams(c["params"], c["B"], GC.F64)
    rsB = ref.RefSimulator(c["phys"], c["cfg"], c["B"], dtype=GC.F64, supersampled_kernel=c["psf"])
    ll = PC.lens_light_image(rsB, tp).reshape(c["B"], H * W)[0]
    sig = torch.as_tensor(err.astype(np.float64)).reshape(-1)[pix]
    y = torch.as_tensor(obs[0].astype(np.float64)).reshape(-1)[pix] - ll[pix]
    F = PC.operator(rs, L)[pix].clone().requires_grad_(True)
    R = torch.as_tensor(PC.reg_matrix(kw["regularization"], kw["n_src"]))
    Fw, yw = F / sig[:, None], y / sig
    M = Fw.t() @ Fw + float(lam[0]) * R
    C = torch.linalg.cholesky(M)
    s = torch.cholesky_solve((Fw.t() @ yw)[:, None], C)[:, 0]
    rw = yw - Fw @ s
    E = -0.5 * (rw * rw).sum() - 0.5 * float(lam[0]) * (s @ (R @ s)) - torch.log(torch.diagonal(C)).sum()
    (g,) = torch.autograd.grad(E, F)
    with torch.no_grad():
        closed = (rw[:, None] * s[None, :] - Fw @ torch.linalg.inv(M)) / sig[:, None]
    d = float((g - closed).abs().max() / closed.abs().max())
    print(f"dE/dF: closed form against autograd, relative {d:.3g}")
    assert d <= 1e-10


def test_symbols_and_argument_validation_without_gpu(native):
    lib = native.lib()
    for name in ("gl_pixsrc_evidence_grad", "gl_pixsrc_grad_workspace_bytes", "gl_pixsrc_grad_layout"):
        assert name in native.SYMBOLS and getattr(lib, name).argtypes == native.SYMBOLS[name][1]
    assert callable(native.Model.pixsrc_evidence_grad)
    from gigalens_amd.simulator import LensSimulator
    assert callable(LensSimulator.source_evidence_and_grad)
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    assert lib.gl_pixsrc_grad_workspace_bytes(None, 2, 4, 4, 10) == 0
    assert lib.gl_pixsrc_grad_workspace_bytes(p, 0, 4, 4, 10) == 0
    assert lib.gl_pixsrc_grad_workspace_bytes(p, -1, 4, 4, 10) == 0
    full = [p, p, p, 2, p, p, None, p, 10, 4, 4, p, 1, p, p, p, p, p, p, p, p, 4096, None]
    for null_at in (0, 1, 2, 4, 5, 7, 11, 13, 14, 15, 16, 17, 18, 19):
        args = list(full)
        args[null_at] = None
        assert lib.gl_pixsrc_evidence_grad(*args) == -1, null_at
        assert b"null argument" in lib.gl_last_error()
    for pos, val in ((3, 0), (3, -2), (8, 0), (9, 0), (10, -1)):  # B, n_used, ny, nx
        args = list(full)
        args[pos] = val
        assert lib.gl_pixsrc_evidence_grad(*args) == -1, (pos, val)
