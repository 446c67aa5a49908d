"""The float64 restatement of the pixelated source reconstruction (tests/pixsrc_cases.py), pinned without a GPU and independently of
the kernels: its forward operator against the interpolated-light restatement, its evidence against the Gaussian marginal
likelihood computed directly, the closed-form ``log det R`` against a dense determinant, and the zero rows of the mapping."""
import math

import numpy as np
import pytest
import torch

from tests import interp_cases as IC
from tests import pixsrc_cases as PC


def _lens_params(c, B, dtype=torch.float64):
    return [{k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype).reshape(-1).expand(B) for k, v in d.items()}
            for d in c["params"]["lens_mass"]]


def test_forward_identity_with_interpolated_light():
    """``F s`` == the image of the same lens with ONE source ``Interpolated(image=s, order=1)`` at ``center``, ``phi = 0``,
    ``scale = pitch``, amplitude 1 (interp_cases.expected_image: a dense contraction per pixel, coded independently of ``L`` and
    ``F``), with a PSF at supersample 2, to 1e-11 of the largest pixel."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light import Interpolated
    from oracle import ref_torch as ref
    c = PC.case("A")
    B, kw = c["B"], c["kw"]
    ny, nx = kw["n_src"]
    s = np.stack([PC.smooth_source((ny, nx), b) for b in range(B)]).astype(np.float32)
    rs = ref.RefSimulator(c["phys"], c["cfg"], B, supersampled_kernel=c["psf"])
    fx, fy = PC.frame_beta(rs, _lens_params(c, B))
    for b in range(B):
        pitch, cx, cy = float(kw["pitch"][b]), float(kw["center"][0][b]), float(kw["center"][1][b])
        F = PC.operator(rs, PC.mapping(fx[:, b], fy[:, b], (ny, nx), pitch, cx, cy)).numpy()
        got = (F @ s[b].reshape(-1).astype(np.float64)).reshape(12, 10)
        phys = PhysicalModel(list(c["phys"].lenses), [], [Interpolated(s[b], order=1)])
        rsi = ref.RefSimulator(phys, c["cfg"], B, supersampled_kernel=c["psf"])
        one = lambda v: torch.full((B,), float(v), dtype=torch.float64)
        params = {"lens_mass": _lens_params(c, B),
                  "source_light": [dict(center_x=one(cx), center_y=one(cy), phi=one(0.0), scale=one(pitch), amp=one(1.0))]}
        want = IC.expected_image(rsi, params)[b].numpy()
        assert np.abs(want).max() > 0
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("reg", PC.REGS)
@pytest.mark.parametrize("n_src", [(2, 2), (3, 2)])
def test_evidence_is_the_gaussian_marginal_likelihood(reg, n_src):
    """``log_evidence`` == ``log N(y; 0, C + F (lambda R)^-1 F^T)`` computed directly in float64 (30 used pixels), to 1e-9 relative."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE
    from gigalens_amd.simulator import SimulatorConfig
    c = PC.case("C11")
    phys = PhysicalModel([SIE(), Shear()], [], [Sersic()])
    cfg = SimulatorConfig(delta_pix=PC.DELTA_PIX, num_pix=(6, 6), supersample=1)
    mask = np.ones((6, 6), dtype=bool)
    mask[0, :] = False  # 30 used pixels
    rng = np.random.default_rng(19)
    err = (0.02 * rng.uniform(0.7, 1.4, size=(6, 6))).astype(np.float32)
    obs = (0.05 * rng.normal(size=(6, 6))).astype(np.float32)
    lam = np.float32(0.7)
    kw = dict(n_src=n_src, pitch=np.float32(0.12), center=(np.float32(0.01), np.float32(-0.02)), regularization=reg,
              strength=np.asarray([lam]), mask=mask)
    out, parts = PC.reconstruct(phys, cfg, None, c["params"], obs, err, **kw, return_parts=True)
    _, F, y, _, _ = parts[0]
    assert F.shape == (30, n_src[0] * n_src[1]) and np.abs(F).max() > 0
    sig = err.astype(np.float64).reshape(-1)[np.flatnonzero(mask.reshape(-1))]
    K = np.diag(sig ** 2) + F @ np.linalg.inv(float(lam) * PC.reg_matrix(reg, n_src)) @ F.T
    sign, logdet = np.linalg.slogdet(K)
    want = -0.5 * y @ np.linalg.solve(K, y) - 0.5 * logdet - 0.5 * len(y) * math.log(2 * math.pi)
    assert sign > 0
    assert abs(out["log_evidence"][0] - want) <= 1e-9 * abs(want)


@pytest.mark.parametrize("n_src", [(1, 1), (2, 3), (7, 6), (32, 32)])
@pytest.mark.parametrize("reg", PC.REGS)
def test_log_det_regularization_closed_form(reg, n_src):
    from gigalens_amd.simulator import LensSimulator
    got, want = LensSimulator.log_det_regularization(reg, n_src), PC.log_det_reg(reg, n_src)
    assert abs(got - want) <= 1e-10 * max(1.0, abs(want))


def test_unknown_regularization_is_refused():
    from gigalens_amd.simulator import LensSimulator
    with pytest.raises(ValueError, match="regularization"):
        LensSimulator.log_det_regularization("laplace", (3, 3))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_zero_rows(dtype):
    """Rows of ``L`` for a ``beta`` that is not finite, or far outside the grid, are exactly zero; a ray on a node has weight 1."""
    nan, inf = float("nan"), float("inf")
    bx = torch.tensor([0.0, nan, 0.0, inf, -inf, 1e30, 0.5, 0.0, -0.101], dtype=dtype)
    by = torch.tensor([0.0, 0.0, nan, 0.0, 0.0, 0.0, 0.0, -3e38, 0.0], dtype=dtype)
    L = PC.mapping(bx, by, (3, 4), 0.1, 0.05, 0.0).numpy()
    assert L.shape == (9, 12)
    assert np.all(L[1:8] == 0) and not np.isnan(L).any()
    assert L[0, 1 * 4 + 1] == 1.0 and np.count_nonzero(L[0]) == 1  # u = v = 1 exactly: node (1, 1) alone
    assert np.count_nonzero(L[8]) == 1  # u = -0.01: only node 0 of the row still sees the ray (zero extension)


def test_native_entries_validate_without_gpu():
    """The two C-ABI entries exist and refuse a null model before anything is launched."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    lib = _native.lib()
    assert lib.gl_pixsrc_workspace_bytes(None, 2, 1, 4, 4, 100) == 0
    null = ctypes.c_void_p(0)
    rc = lib.gl_pixsrc_reconstruct(None, null, null, 2, null, null, null, null, 100, 4, 4, null, 1, null, 1, null, null, null, null,
                                   null, 0, null)
    assert rc == -1 and b"null" in lib.gl_last_error()
