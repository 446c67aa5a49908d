"""The shapelet kernels (csrc/gl_shp.hip.h) at every compaction, cull and block edge (tests/shp_edge_cases.py).

Per case the four modes run against the float64 oracle under the gates of tests/test_gpu_dispatch_matrix.py, with the
`gl_shp_kernel<...>` instantiation of each mode declared; then the kernel's own counters in the pad slots of its partial rows --
chain rounds, wave-tiles, wave-tiles that ran the lens -- must EQUAL what the float64 geometry of the case says
(tests/test_shp_edges_host.py keeps every case far enough from the table boundary and the cull thresholds for that): a case
that no longer takes the branch it is there for fails instead of passing on another path.  No pixel of any case lies within
the margin of the table boundary, so no pixel is left out of any image comparison.

Then: cull off = cull on bit for bit; blocked order = linear order bit for bit in the image; other tilings of the chunks
(GIGALENS_HIP_TARGET_WGS: the third and later trips of the coordinate prefetch) = the default bit for bit in the image; the
orders n_max = 0 (the smallest the front end accepts), 1, 2, 3, 10; and the fused linear solve (`gl_shp_normal_kernel`) on its
own edges against the oracle and the library's stack path."""
import numpy as np
import pytest
import torch

from tests import dispatch_cases as DC
from tests import helpers as H
from tests import shp_edge_cases as SE
from tests.test_gpu_dispatch_matrix import check_case_vs_oracle, kernel_name  # noqa: F401  (kernel_name: the module fixture)
from tests.test_gpu_lstsq import _observation
from tests.test_gpu_parity import GRAD_RTOL_COL, LL_RTOL, gl  # noqa: F401  (gl: the module fixture)

pytestmark = pytest.mark.gpu

KNOBS = DC.ENV_KNOBS + ("GIGALENS_HIP_SHP_CULL", "GIGALENS_HIP_TARGET_WGS", "GIGALENS_HIP_LSTSQ_FUSED", "GIGALENS_HIP_LSTSQ_WGS", "GIGALENS_HIP_CHUNK_PX")
_ids = lambda cases: [c.id for c in cases]


@pytest.fixture(autouse=True)
def _a_gpu_error_ends_the_session():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # nothing more is started on a device that reported an error
        pytest.exit(f"GPU error: {e}", returncode=3)


def _set_env(monkeypatch, case):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def expected_chunks(case):
    """chunking() of csrc/gigalens_hip.hip restated: chunks per sample of a launch of the specialised kernels."""
    N, B = case.n_pixels, case.batch
    want = max(-(-768 // B), -(-N // 8192))
    if "GIGALENS_HIP_TARGET_WGS" in case.env:
        want = max(1, -(-int(case.env["GIGALENS_HIP_TARGET_WGS"]) // B))
    per = max(1024, -(-(-(-N // want)) // 1024) * 1024)
    return -(-N // per)


def launch(gl, case, monkeypatch):
    """simulate and the fused forward + gradient of `case` under its knobs, with the kernel's counters per sample."""
    _set_env(monkeypatch, case)
    wl = SE.workload(case)
    obs, err, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=wl.batch)
    packed = H.sample_packed(wl, sim, seed=0)
    m = sim._model
    img = m.simulate_fwd(packed).clone()
    mask = sim.img_region if case.pix_region else None
    ll, chi, g = m.loglike(packed, obs, err, mask, wl.background_rms, wl.exp_time, True)
    rows = m.partial_rows(wl.batch).double().cpu()
    pk = rows[:, :, 3]
    return dict(img=img, ll=ll.clone(), chi=chi.clone(), g=g.clone(), n_chunks=rows.shape[1],
                rounds=rows[:, :, 2].sum(1).numpy(), tiles=torch.remainder(pk, 4096.0).sum(1).numpy(),
                lensed=torch.floor(pk / 4096.0).sum(1).numpy())


def check_counters(case, out):
    """The branch ran: rounds = sum ceil(count / 64) (direct mode: 2 per wave-tile), every wave-tile was seen, and exactly the
    wave-tiles the float64 restatement of the cull test leaves ran the lens -- per sample, as equalities."""
    g = SE.geometry(case)
    per_sample = g.tiles // case.batch
    rounds = ((g.count + 63) // 64).sum(1) if case.interpolate else np.full(case.batch, 2 * per_sample)
    print(f"{case.id}: chunks {out['n_chunks']}  rounds {out['rounds']} (oracle {rounds})  wave-tiles {out['tiles']}  "
          f"ran the lens {out['lensed']} (oracle {per_sample - g.culled.sum(1)})")
    assert out["n_chunks"] == expected_chunks(case)
    assert np.array_equal(out["tiles"], np.full(case.batch, per_sample)), (out["tiles"], per_sample)
    assert np.array_equal(out["rounds"], rounds), (out["rounds"], rounds)
    assert np.array_equal(out["lensed"], per_sample - g.culled.sum(1)), (out["lensed"], per_sample - g.culled.sum(1))
    return g


def same_bits(a, b, names):
    for n in names:
        assert torch.equal(a[n], b[n]), (n, float((a[n] - b[n]).abs().max()))


def run_case(gl, case, kernel_name, monkeypatch):  # noqa: F811
    _set_env(monkeypatch, case)
    check_case_vs_oracle(gl, case, kernel_name, wl=SE.workload(case))
    out = launch(gl, case, monkeypatch)
    check_counters(case, out)
    return out


@pytest.mark.parametrize("case", SE.CASES, ids=_ids(SE.CASES))
def test_edge_case_vs_oracle(gl, case, kernel_name, monkeypatch):  # noqa: F811
    """All four modes against the oracle, the declared kernels, and the counters of the LL_GRAD launch."""
    run_case(gl, case, kernel_name, monkeypatch)


@pytest.mark.parametrize("case", SE.ORDER_CASES, ids=_ids(SE.ORDER_CASES))
def test_orders_vs_oracle(gl, case, kernel_name, monkeypatch):  # noqa: F811
    """n_max = 0, 1, 2, 3 (1, 3, 6, 10 amplitudes in the zero-padded 12 x 12 matrix, the epilogue's n_amp loop) and 10, table and
    direct.  n_max = 0 is the smallest order the front end accepts."""
    run_case(gl, case, kernel_name, monkeypatch)


CULL_CASES = [c for c in SE.CASES if "cull" in c.roles]


@pytest.mark.parametrize("case", CULL_CASES, ids=_ids(CULL_CASES))
def test_cull_off_equals_cull_on(gl, case, monkeypatch):  # noqa: F811
    """Nothing of a culled tile's lens evaluation reaches an output: GIGALENS_HIP_SHP_CULL=0 gives the same bits, and then every
    wave-tile runs the lens."""
    on = launch(gl, case, monkeypatch)
    off_case = SE.variant(case, "nocull", GIGALENS_HIP_SHP_CULL=0)
    off = launch(gl, off_case, monkeypatch)
    same_bits(on, off, ("ll", "chi", "g", "img"))
    check_counters(off_case, off)
    assert np.array_equal(off["lensed"], off["tiles"]) and (on["lensed"] < on["tiles"]).all()


WHOLE_TABLE = [c for c in SE.CASES if SE.blocked(c)]


@pytest.mark.parametrize("case", WHOLE_TABLE, ids=_ids(WHOLE_TABLE))
def test_blocked_equals_linear(gl, case, kernel_name, monkeypatch):  # noqa: F811
    """GIGALENS_HIP_SHP_BLOCKED=0 orders the same per-pixel work differently: the image is the same bit for bit; log-likelihood
    and gradient, summed in another order, agree within the oracle gates.  The count-pinning cases also run all four modes against
    the oracle in the linear order (their squares give other counts there: the host test lists them)."""
    lin_case = SE.variant(case, "linear", GIGALENS_HIP_SHP_BLOCKED=0)
    blk = launch(gl, case, monkeypatch)
    lin = launch(gl, lin_case, monkeypatch)
    same_bits(blk, lin, ("img",))
    check_counters(lin_case, lin)
    ll_b, ll_l = blk["ll"].cpu().numpy(), lin["ll"].cpu().numpy()
    ge = float(H.grad_col_err(lin["g"].cpu().numpy(), blk["g"].cpu().numpy()).max())
    print(f"{case.id}: blocked vs linear: ll {float(np.max(np.abs(ll_l - ll_b) / np.abs(ll_b))):.2e} (gate {LL_RTOL:.0e})  "
          f"grad {ge:.2e} (gate {GRAD_RTOL_COL:.0e})")
    assert np.allclose(ll_l, ll_b, rtol=LL_RTOL)
    assert np.allclose(lin["chi"].cpu().numpy(), blk["chi"].cpu().numpy(), rtol=LL_RTOL)
    assert ge <= GRAD_RTOL_COL
    if "count" in case.roles:
        _set_env(monkeypatch, lin_case)
        check_case_vs_oracle(gl, lin_case, kernel_name, wl=SE.workload(lin_case))


# (case, GIGALENS_HIP_TARGET_WGS, chunks per sample, tiles per chunk)
CHUNKINGS = [("shp_cull64", 1, 1, 8), ("shp_cull64", 4, 2, 4), ("shp_blk96", 1, 1, 18),
             ("shp_direct64", 1, 1, 8), ("shp_direct64", 4, 2, 4), ("shp_direct96", 1, 1, 18)]


@pytest.mark.parametrize("cid,wgs,n_chunks,tiles_per_chunk", CHUNKINGS, ids=[f"{c}_wgs{w}" for c, w, _, _ in CHUNKINGS])
def test_tiles_per_chunk(gl, cid, wgs, n_chunks, tiles_per_chunk, kernel_name, monkeypatch):  # noqa: F811
    """More than two 512-pixel tiles per chunk: the third and later trips of the coordinate prefetch of table mode, the re-read at
    the chunk's last tile, the plain tile loop of direct mode.  Inside the oracle gates, the chunking as intended, and in table
    mode the same image bits as the default chunking (two tiles per chunk)."""
    base = SE.BY_ID[cid]
    case = SE.variant(base, f"wgs{wgs}", GIGALENS_HIP_TARGET_WGS=wgs)
    assert expected_chunks(case) == n_chunks and base.n_pixels == n_chunks * tiles_per_chunk * 512
    assert expected_chunks(base) == base.n_pixels // 1024
    out = run_case(gl, case, kernel_name, monkeypatch)
    assert out["n_chunks"] == n_chunks
    if base.interpolate:
        same_bits(out, launch(gl, base, monkeypatch), ("img",))


@pytest.mark.parametrize("case", SE.LSTSQ_CASES + SE.LSTSQ_ONE_WG, ids=_ids(SE.LSTSQ_CASES + SE.LSTSQ_ONE_WG))
def test_fused_solve_edges(gl, case, monkeypatch):  # noqa: F811
    """test_gpu_lstsq.py::test_lstsq_without_the_stack on the edges of gl_shp_normal_kernel: the oracle, the library's own stack
    path (GIGALENS_HIP_LSTSQ_FUSED=0) and the kernel name; its gates (2e-4 of the image's maximum, chi^2 rtol 1e-4).  Three
    cases run again with one workgroup per sample, which then walks every tile of the image.
    (The normal matrix of the fused path is not exposed to Python, so its (Y, Y) entry is not compared on its own.)"""
    from oracle import ref_torch as ref
    _set_env(monkeypatch, case)
    wl = SE.workload(case)
    B = case.batch
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=B)
    monkeypatch.setenv("GIGALENS_HIP_LSTSQ_FUSED", "0")   # read once per model: this one goes through the stack
    sim_stack = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=B)
    monkeypatch.delenv("GIGALENS_HIP_LSTSQ_FUSED")
    x = wl.prior.sample(B)
    obs, err = _observation(wl)
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, B, dtype=torch.float64)
    x64 = {g: [{k: v.double() for k, v in d.items()} for d in lst] for g, lst in x.items()}
    img_o = ref.lstsq_simulate(rs, x64, obs, err).numpy()
    img = sim.lstsq_simulate(x, obs, err).cpu().numpy()
    c = sim.lstsq_simulate(x, obs, err, return_coeffs=True)
    name = sim._model.last_main_kernel()
    assert "gl_shp_normal_kernel" in name, name
    img_s = sim_stack.lstsq_simulate(x, obs, err).cpu().numpy()
    assert "gl_shp_normal_kernel" not in sim_stack._model.last_main_kernel()
    top = np.abs(img_o).max()
    w = 1.0 / err
    chi = lambda im: (((im - obs) * w) ** 2).sum(axis=(1, 2))
    e_o, e_s = np.abs(img - img_o).max() / top, np.abs(img - img_s).max() / top
    print(f"{case.id}: Dl {c.shape[1]} (o = {c.shape[1] & 3})  image vs oracle {e_o:.2e}, vs the stack path {e_s:.2e} (gate 2e-4)  "
          f"chi^2 vs the stack path {float(np.max(np.abs(chi(img) / chi(img_s) - 1))):.2e} (gate 1e-4), "
          f"vs the oracle {float(np.max(np.abs(chi(img) / chi(img_o) - 1))):.2e}")
    assert c.shape == (B, (case.n_max + 1) * (case.n_max + 2) // 2)
    assert e_o <= 2e-4, e_o
    assert e_s <= 2e-4, e_s
    assert np.allclose(chi(img), chi(img_s), rtol=1e-4)
