"""The deferred guard of the select-free whole tiles (csrc/gl_pair.hip.h).

A select-free tile no longer tests its guard: it folds the range checks and the NaN test of its image into wave-private state, and
after the LAST whole tile of the chunk each wave asks once.  A wave whose guard fired anywhere throws its sums away and redoes the
whole chunk with the careful body.  What can go wrong is new: sums that are not reset (or reset for the wrong wave), a wave that
redoes while its neighbour does not, a tile counted twice, image pixels left over from the select-free pass -- and it shows only
with several whole tiles per chunk and several waves deciding differently, which tests/test_gpu_pair_select_free.py (2 tiles per
chunk) does not have.  Shapes here: batch 768 (one chunk per sample, chunking()) at 64 x 64 -- 8 whole pair tiles per chunk -- and
at 72 x 72 -- 10 whole tiles and a ragged one of 64 pixels.

For every input the results must be BITWISE those of GIGALENS_HIP_CAREFUL_TILES=1 (every whole tile careful), the log-likelihood of a
few rows is held to the float64 oracle at LL_RTOL, and in the singular cases only every other sample is singular: the regular
samples in between must come out, bitwise, as in a launch where no sample is singular."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_parity import LL_RTOL, gl  # noqa: F401
from tests.test_gpu_pair_select_free import _both, _column, _equal_bits, _models

pytestmark = pytest.mark.gpu

BATCH = 768
TILE = 512                     # pixels of a pair tile: lane t of the workgroup owns pixels t and t + 256 of it
ORACLE_ROWS = [1, 2, 383, 767]  # two singular (odd) and two regular rows where half of the batch is singular


def _workload(gl, name, num_pix):
    from gigalens_amd.simulator import SimulatorConfig
    phys, prior = _models(gl)[name]
    return gl.workloads.Workload(name, phys, prior, SimulatorConfig(delta_pix=0.065, num_pix=num_pix), BATCH)


def _cotangent(n, seed=5):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn((BATCH, n, n), generator=g, dtype=torch.float32).to("cuda")


def _whole_tiles(num_pix):
    return (num_pix * num_pix) // TILE


def _wave(j):
    return ((j % TILE) % 256) // 64


_SETUP = {}


def _setup(gl, name, num_pix):
    """(workload, observation, regular packed rows, their log-likelihood and chi^2 from a default launch), once per shape."""
    key = (name, num_pix)
    if key not in _SETUP:
        wl = _workload(gl, name, num_pix)
        obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
        sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=BATCH)
        packed = H.sample_packed(wl, sim, seed=4)
        ll, chi2, _ = sim._model.loglike(packed, obs, None, None, wl.background_rms, wl.exp_time, True)
        torch.cuda.synchronize()
        assert torch.isfinite(ll).all() and torch.isfinite(chi2).all()
        _SETUP[key] = (wl, obs, packed.clone(), ll.clone(), chi2.clone())
    return _SETUP[key]


def _oracle_ll(wl, packed, obs, err, rows):
    from oracle import ref_torch as ref
    rs = ref.RefSimulator(wl.phys_model, wl.sim_config, len(rows), dtype=torch.float64)
    with torch.no_grad():
        ll, _ = ref.stats_pixels(rs, H.struct_from_packed(wl.phys_model, packed[rows].double()), obs.cpu().numpy(),
                                 wl.background_rms, wl.exp_time, error_map=None if err is None else err.cpu().numpy())
    return ll.numpy().reshape(-1)


def _check_ll(wl, packed, obs, err, ll, rows=ORACLE_ROWS):
    got, want = ll.cpu().numpy().reshape(-1)[rows], _oracle_ll(wl, packed.cpu(), obs, err, rows)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.allclose(got, want, rtol=LL_RTOL, equal_nan=True), (got, want)
    return want


def _index(rows, t):
    return torch.as_tensor(np.asarray(rows), dtype=torch.long, device=t.device)


def _put_centre(packed, phys, group, rows, gx, gy, j):
    """Centre of the profile `group` = the float32 grid point j, for `rows`: x - cx and y - cy are exact zeros at that pixel."""
    cx, cy = _column(phys, *group, "center_x"), _column(phys, *group, "center_y")
    packed[_index(rows, packed), cx] = float(gx[j])
    packed[_index(rows, packed), cy] = float(gy[j])
    p = packed.cpu().numpy()
    assert p.dtype == np.float32 and np.all((gx[j] - p[rows, cx]) == 0) and np.all((gy[j] - p[rows, cy]) == 0)


def _assert_same_as_careful(default, careful, finite):
    assert len(default) == len(careful)
    for a, b in zip(default, careful):
        assert _equal_bits(a, b)
        if finite:
            assert torch.isfinite(a).all()


def _assert_regular_rows_untouched(gl, name, num_pix, default, regular):
    _, _, _, ll0, chi0 = _setup(gl, name, num_pix)
    keep = _index(regular, ll0)
    assert _equal_bits(default[0].reshape(-1)[keep], ll0.reshape(-1)[keep])
    assert _equal_bits(default[1].reshape(-1)[keep], chi0.reshape(-1)[keep])


@pytest.mark.parametrize("with_err", [False, True])
@pytest.mark.parametrize("num_pix", [64, 72])
@pytest.mark.parametrize("name", ["EPL+Shear|Sersic", "SIE|Sersic"])
def test_regular_draws_equal_the_careful_path_bitwise(gl, monkeypatch, name, num_pix, with_err):
    wl = _workload(gl, name, num_pix)
    obs, _, _ = gl.workloads.synthetic_observation(wl, gl.LensSimulator)
    err = (0.2 + 0.05 * obs.abs()).contiguous() if with_err else None
    x = wl.prior.sample(BATCH, seed=3)
    packed = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=BATCH).pack(x)
    pm = gl.ForwardProbModel(wl.prior, obs.cpu().numpy(), wl.background_rms, wl.exp_time, include_positions=False)
    z = pm.bij.inverse(x).to("cuda")
    default, careful = _both(gl, monkeypatch, wl, obs, err, packed, _cotangent(num_pix), z)
    assert len(default) == 8  # loglike, chi2, gradient, image, image VJP; fused log_prob, reduced chi2, gradient in z
    _assert_same_as_careful(default, careful, finite=True)
    _check_ll(wl, packed, obs, err, default[0])


def _positions(num_pix):
    """(label, pixel) of the EPL-centre cases: first, a middle and the last whole tile, both halves of a pair; the ragged tile."""
    last = _whole_tiles(num_pix) - 1
    if num_pix == 64:  # 8 whole tiles, no ragged one
        return [("first-lower", 212), ("first-upper", 340), ("middle-lower", 4 * TILE + 100), ("middle-upper", 4 * TILE + 300),
                ("last-lower", last * TILE + 150), ("last-upper", last * TILE + 400)]
    # 72 x 72: 10 whole tiles and the ragged [5120, 5184), whose 64 pixels are all lower halves
    return [("middle-lower", 5 * TILE + 40), ("last-upper", last * TILE + 300), ("ragged", 5150)]


@pytest.mark.parametrize("num_pix,where", [(n, w) for n in (64, 72) for w, _ in _positions(n)])
def test_epl_centre_on_a_pixel_in_every_position(gl, monkeypatch, num_pix, where):
    name = "EPL+Shear|Sersic"
    wl, obs, packed0, _, _ = _setup(gl, name, num_pix)
    j = dict(_positions(num_pix))[where]
    tile, n_whole = j // TILE, _whole_tiles(num_pix)
    which = "first" if tile == 0 else "last" if tile == n_whole - 1 else "ragged" if tile == n_whole else "middle"
    assert j < num_pix * num_pix and where == (which if which == "ragged" else which + ("-lower" if j % TILE < 256 else "-upper"))
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=BATCH)
    gx, gy = sim.img_X.cpu().numpy(), sim.img_Y.cpu().numpy()
    assert gx.dtype == np.float32 and gx.shape == (num_pix * num_pix,)
    singular, regular = np.arange(1, BATCH, 2), np.arange(0, BATCH, 2)
    packed = packed0.clone()
    _put_centre(packed, wl.phys_model, ("lens_mass", 0), singular, gx, gy, j)
    default, careful = _both(gl, monkeypatch, wl, obs, None, packed, _cotangent(num_pix))
    assert len(default) == 5
    _assert_same_as_careful(default, careful, finite=True)
    assert np.isfinite(_check_ll(wl, packed, obs, None, default[0])).all()
    _assert_regular_rows_untouched(gl, name, num_pix, default, regular)


@pytest.mark.parametrize("num_pix", [64, 72])
def test_two_singular_profiles_on_two_waves_of_one_workgroup(gl, monkeypatch, num_pix):
    name = "EPL+Shear|Sersic|Sersic"
    wl, obs, packed0, _, _ = _setup(gl, name, num_pix)
    ja, jb = 3 * TILE + 286, 2 * TILE + 420  # tiles 3 and 2 (the same workgroup also where a sample's chunk is halved), waves 0 and 2
    assert ja // TILE != jb // TILE and max(ja, jb) // TILE < _whole_tiles(num_pix) // 2 and (_wave(ja), _wave(jb)) == (0, 2)
    sim = gl.LensSimulator(wl.phys_model, wl.sim_config, bs=BATCH)
    gx, gy = sim.img_X.cpu().numpy(), sim.img_Y.cpu().numpy()
    singular, regular = np.arange(1, BATCH, 2), np.arange(0, BATCH, 2)
    packed = packed0.clone()
    _put_centre(packed, wl.phys_model, ("lens_mass", 0), singular, gx, gy, ja)
    _put_centre(packed, wl.phys_model, ("lens_light", 0), singular, gx, gy, jb)
    default, careful = _both(gl, monkeypatch, wl, obs, None, packed, _cotangent(num_pix))
    assert len(default) == 5
    _assert_same_as_careful(default, careful, finite=True)
    assert np.isfinite(_check_ll(wl, packed, obs, None, default[0])).all()
    _assert_regular_rows_untouched(gl, name, num_pix, default, regular)


@pytest.mark.parametrize("num_pix", [64, 72])
def test_overflowing_sersic(gl, monkeypatch, num_pix):
    name = "EPL+Shear|Sersic"
    wl, obs, packed0, _, _ = _setup(gl, name, num_pix)
    phys = wl.phys_model
    singular, regular = np.arange(1, BATCH, 2), np.arange(0, BATCH, 2)
    packed = packed0.clone()
    col = lambda n: _column(phys, "source_light", 0, n)
    packed[_index(singular, packed), col("n_sersic")] = 0.05
    packed[_index(singular, packed), col("R_sersic")] = 0.01
    packed[_index(singular, packed), col("center_x")] = 0.7
    packed[_index(singular, packed), col("center_y")] = 0.7
    # singular by construction: (R / R_sersic)^(1/n) = (R / 0.01)^20 is beyond float32 for R > 0.85 arcsec; the reference's ray-shoot
    # in float32 on the host says so for pixels of the whole tiles of the singular rows that are checked
    from oracle import ref_torch as ref
    rows = [r for r in ORACLE_ROWS if r % 2 == 1]
    rs = ref.RefSimulator(phys, wl.sim_config, len(rows), dtype=torch.float32)
    bx, by = rs.beta(rs.img_X, rs.img_Y, H.struct_from_packed(phys, packed.cpu()[rows])["lens_mass"])
    u = torch.pow(torch.hypot(bx - 0.7, by - 0.7) / np.float32(0.01), np.float32(1.0 / 0.05))
    assert u.dtype == torch.float32 and bool(torch.isinf(u[:_whole_tiles(num_pix) * TILE]).any(0).all())
    default, careful = _both(gl, monkeypatch, wl, obs, None, packed, _cotangent(num_pix))
    assert len(default) == 5
    _assert_same_as_careful(default, careful, finite=False)
    for a, b in zip(default, careful):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))
    ll, img = default[0].cpu().numpy().reshape(-1), default[3].cpu().numpy()
    assert not np.isnan(img).any() and (img[singular] == 0).any()  # NaN -> 0: the select-free pass's pixels were stored over
    ll_o = _check_ll(wl, packed, obs, None, default[0])
    assert np.isnan(ll_o[[i for i, r in enumerate(ORACLE_ROWS) if r % 2 == 1]]).all()
    assert np.isnan(ll[singular]).all() and np.isfinite(ll[regular]).all()
    _assert_regular_rows_untouched(gl, name, num_pix, default, regular)
