"""gl_pixsrc_reconstruct (csrc/gl_pixsrc.hip.h, csrc/gl_api_pixsrc.hip) at every block, chunk and slice edge, against the float64
restatement from rays of tests/pixsrc_cases.py (``MATRIX``; ``reconstruct_from_rays``).

The tests hand rays of their own to ``sim._model.pixsrc_reconstruct``; the simulator supplies the frame, the supersampling and the
PSF alone.  Groups of cases (tests/pixsrc_cases.py ``_matrix`` names what each sits on):
  solve_S*     S = 32, 33, 64, 65, 288, 289, 1024: the 32-column blocks of the Cholesky and the strides of its 256-row loops;
               dense_S289: 289 nodes under a PSF, the one case whose M is dense (without a PSF M is banded, and the rows the second
               stride of those loops reaches hold zeros)
  stencil_*    ny or nx in {1, 2, 3} under gradient and curvature: every branch of ``pix_r1``
  pixels_*     n_used = 5 .. 120 against the tile of 32 (n_used < S: A0 singular), scattered masks, a PSF at supersample 2;
               frame_255: 255 supersampled pixels
  hand_*       rays on nodes, on and one float32 step either side of the range test, in the half-supported border cells, NaN and
               infinite, a node no ray touches; a sample whose every ray misses; a sample of the uniform recipe
  slices_*, planes_budget, planes_cap, chunks   the three host loops, each proven by ``pixsrc_layout`` to make a second iteration
  pivot        a pivot that is not finite in the SECOND block of the factorisation
  hard         cond(M) in [1e3, 1e4], with a gate of its own

Value gates: the rule of tests/test_gpu_pixsrc.py -- arrays relative to their largest element, scalars to ``|chi2| + |log det| + S``,
gate = 4 x the worst error of the restatement run in float32 on the CPU over this file's cases bar ``hard`` (whose gate is 4 x its
own yardstick); both figures are printed before they are asserted, and nothing in a gate comes from the kernels.  Asserted on the
reference alone: ``ok`` everywhere bar ``pivot``, ``cond(M) <= 1e4`` for every (sample, strength), every main gate <= 1e-5.
Measured on one MI355X (kernel error / gate, worst over the cases): see DESIGN.md section 7."""
import numpy as np
import pytest
import torch

from tests import pixsrc_cases as PC
from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = PC.ARRAYS + PC.SCALARS
SCANS = tuple(n for n in PC.MAIN if PC.MATRIX[n]["L"] > 1)
_SIMS, _RUNS = {}, {}


def _S(c):
    return c["n_src"][0] * c["n_src"][1]


def _sim(gl, name, B):
    if (name, B) not in _SIMS:
        phys, cfg, psf = PC.matrix_sim_args(name)
        _SIMS[name, B] = gl.LensSimulator(phys, cfg, bs=B, supersampled_kernel=psf)
    return _SIMS[name, B]


def _call(gl, name, samples=None, column=None):
    """The native call on the inputs of a case (all samples or ``samples``; all strengths or one ``column``) -> numpy dict with
    the ``L`` axis.  ``log_evidence`` is put together on the host in float64 as ``reconstruct_source`` does."""
    c, inp, _, _ = PC.matrix_data(name)
    sel = np.arange(c["B"]) if samples is None else np.asarray(samples)
    sim = _sim(gl, name, len(sel))
    H, W = c["frame"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(sim.device)
    lam = inp["strength"][sel] if column is None else inp["strength"][sel][:, column:column + 1]
    ll = None if inp["lens_light"] is None else t(inp["lens_light"][sel].reshape(-1, H, W))
    src, img, scal, ok = sim._model.pixsrc_reconstruct(t(inp["beta_x"][sel]), t(inp["beta_y"][sel]), t(inp["obs"][sel]),
                                                       t(inp["sigma"][sel]), ll, t(inp["pix"]), c["n_src"], t(inp["pose"][sel]),
                                                       gl.LensSimulator.REGULARIZATIONS[c["reg"]], t(lam))
    torch.cuda.synchronize()
    src, img, scal, ok = (v.cpu().numpy() for v in (src, img, scal, ok))
    lam64, sig64 = lam.astype(np.float64), inp["sigma"][sel].astype(np.float64)
    with np.errstate(divide="ignore"):
        noise = np.log(2.0 * np.pi * sig64 ** 2).sum(axis=1, keepdims=True)
    ldr = gl.LensSimulator.log_det_regularization(c["reg"], c["n_src"])
    out = {"source": src, "model_image": img, "chi2": scal[..., 0], "reg": scal[..., 1], "log_det": scal[..., 2], "ok": ok != 0}
    out["log_evidence"] = (-0.5 * out["chi2"] - 0.5 * lam64 * out["reg"] - 0.5 * out["log_det"] + 0.5 * _S(c) * np.log(lam64) + 0.5 * ldr
                           - 0.5 * noise)
    return out


def _run(gl, name):
    """One GPU call per case, shared by the tests (left unchanged)."""
    if name not in _RUNS:
        _RUNS[name] = _call(gl, name)
    return _RUNS[name]


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS + ("ok",))


def _take(out, b=slice(None), l=slice(None)):
    return {k: v[b, l] for k, v in out.items()}


def _yardstick(name):
    c, _, ref, f32 = PC.matrix_data(name)
    e = PC.errors(f32, ref, _S(c))
    print(f"float32 yardstick {name}: " + ", ".join(f"{k} {e[k]:.3e}" for k in KEYS))
    return e


@pytest.fixture(scope="module")
def gates():
    """4 x the worst float32-restatement error over the main cases, per quantity."""
    worst = {k: 0.0 for k in KEYS}
    for name in PC.MAIN:
        e = _yardstick(name)
        worst = {k: max(worst[k], e[k]) for k in KEYS}
    print("float32 yardstick maxima: " + ", ".join(f"{k} {worst[k]:.3e}" for k in KEYS))
    return {k: 4 * v for k, v in worst.items()}


@pytest.fixture(scope="module")
def hard_gates():
    return {k: 4 * v for k, v in _yardstick("hard").items()}


def test_conditions_on_the_reference(gates, hard_gates):
    """What keeps a gate from hiding a failure, asserted on the reference alone."""
    for name in PC.MAIN + ("hard",):
        _, _, ref, f32 = PC.matrix_data(name)
        assert ref["ok"].all() and f32["ok"].all(), name
        assert np.all(ref["cond"] <= 1e4), (name, ref["cond"])
    for k in KEYS:
        assert gates[k] <= 1e-5, (k, gates[k])
    cond = PC.matrix_data("hard")[2]["cond"]
    assert np.all(cond >= 1e3), cond
    assert PC.matrix_data("pivot")[3]["ok"][:, 0].tolist() == [False, True]


def _check_values(name, got, ref, S, gate):
    assert got["ok"].all()
    for k in KEYS + ("ok",):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    e = PC.errors(got, ref, S)
    for k in KEYS:
        print(f"{name} {k}: kernel error {e[k]:.3e}, gate {gate[k]:.3e}, ratio {e[k] / gate[k]:.3f}")
    for k in KEYS:
        assert e[k] <= gate[k], (name, k, e[k], gate[k])


def _check_off_pixels(c, inp, got):
    """Off the used pixels ``model_image`` is bitwise the lens light, or 0 where there is none."""
    H, W = c["frame"]
    off = np.ones(H * W, dtype=bool)
    off[inp["pix"]] = False
    ll = np.zeros((c["B"], H * W), dtype=np.float32) if inp["lens_light"] is None else inp["lens_light"]
    img = got["model_image"].reshape(c["B"], -1, H * W)
    for l in range(img.shape[1]):
        assert np.array_equal(img[:, l][:, off], ll[:, off])


@pytest.mark.parametrize("name", PC.MAIN)
def test_values_against_float64(gl, gates, name):
    c, inp, ref, _ = PC.matrix_data(name)
    got = _run(gl, name)
    _check_values(name, got, ref, _S(c), gates)
    _check_off_pixels(c, inp, got)
    if c["group"] == "hand":  # sample 1: every ray misses the grid
        assert np.all(got["source"][1] == 0) and np.all(got["model_image"][1] == 0) and np.all(got["reg"][1] == 0)
        lam = float(inp["strength"][1, 0])  # M = lambda R exactly: log det M = S log lambda + log det R, the host's closed form
        want = _S(c) * np.log(lam) + gl.LensSimulator.log_det_regularization(c["reg"], c["n_src"])
        e = abs(got["log_det"][1, 0] - want) / (abs(ref["chi2"][1, 0]) + abs(want) + _S(c))
        print(f"{name} all-miss log_det: error {e:.3e}, gate {gates['log_det']:.3e}")
        assert e <= gates["log_det"]


def test_harder_system(gl, hard_gates):
    c, inp, ref, _ = PC.matrix_data("hard")
    got = _run(gl, "hard")
    _check_values("hard", got, ref, _S(c), hard_gates)
    _check_off_pixels(c, inp, got)


def test_layout_is_the_restatement(gl):
    """``pixsrc_layout`` against the restatement of tests/pixsrc_cases.py for every case, and its refusals."""
    from gigalens_amd._native import NativeLibraryError
    for name, c in PC.MATRIX.items():
        n_used = c["n_used"] or c["frame"][0] * c["frame"][1]
        got = _sim(gl, name, c["B"])._model.pixsrc_layout(c["B"], c["L"], c["n_src"], n_used)
        assert got == PC.layout(c["frame"], c["ss"], c["psf"], c["B"], c["L"], _S(c), n_used), name
    model = _sim(gl, "pivot", 2)._model
    for B, L, n_src, n_used in ((0, 1, (5, 8), 120), (65536, 1, (5, 8), 120), (2, 0, (5, 8), 120), (2, 1, (0, 8), 120),
                                (2, 1, (33, 32), 120), (2, 1, (5, 8), 0), (2, 1, (5, 8), 121)):
        with pytest.raises(NativeLibraryError):
            model.pixsrc_layout(B, L, n_src, n_used)


@pytest.mark.parametrize("name", PC.LOOPS)
def test_host_loop_makes_a_second_iteration(gl, name):
    """The split a host-loop case is named for, from the library's own ``pix_layout``."""
    c = PC.MATRIX[name]
    lay = _sim(gl, name, c["B"])._model.pixsrc_layout(c["B"], c["L"], c["n_src"], c["frame"][0] * c["frame"][1])
    print(name, lay)
    PC.check_split(name, lay)


@pytest.mark.parametrize("name", PC.MAIN + ("hard",))
def test_deterministic(gl, name):
    assert _same_bits(_run(gl, name), _call(gl, name))


@pytest.mark.parametrize("name", SCANS)
def test_scan_columns_equal_single_calls(gl, name):
    scan = _run(gl, name)
    for l in range(PC.MATRIX[name]["L"]):
        assert _same_bits(_take(scan, l=slice(l, l + 1)), _call(gl, name, column=l)), l


@pytest.mark.parametrize("name", PC.LOOPS)
def test_sample_equals_the_sample_alone(gl, name):
    """Across chunks, launches of planes and slices a sample has the bits it has in a call of its own with B = 1."""
    both = _run(gl, name)
    for b in PC.alone_samples(name):
        assert _same_bits(_take(both, b=slice(b, b + 1)), _call(gl, name, samples=[b])), b


def test_pivot_failure_in_a_later_block(gl):
    """Sample 0: one ray exactly on node 35 whose pixel has an rms of 1e-25, so A0[35][35] is not finite in float32 and the pivot
    fails in the second 32-column block (flagged by the float32 restatement first): ``ok == [0, 1]``, every output of sample 0 NaN,
    sample 1 bitwise what it is alone."""
    _, _, _, f32 = PC.matrix_data("pivot")
    assert f32["ok"][:, 0].tolist() == [False, True]
    got = _run(gl, "pivot")
    assert got["ok"][:, 0].tolist() == [False, True]
    assert all(np.isnan(got[k][0]).all() for k in KEYS)
    assert all(np.isfinite(got[k][1]).all() for k in KEYS)
    assert _same_bits(_take(got, b=slice(1, 2)), _call(gl, "pivot", samples=[1]))
