"""The launch shape and the workspace layout are facts the host layer derives in one place (launch_plan) and every entry point,
the workspace carve and the sort's split rank read from there.  This pins them: for every workload and batch size below, the
workspace sizes and the four outputs of gl_model_launch_shape equal the values recorded in tests/golden/launch_layout.json by this
same code at the commit named in the file's first key.  Models are created and asked questions only; no kernel is launched."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.test_gpu_parity import gl  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_layout.json")
BATCHES = [1, 2, 3, 64, 767, 768, 1000, 1024, 1025]
NUM_PIX = 32
WORKLOADS = ["C1", "C2", "C3", "C3L", "C3D", "C4", "C6", "C2_psf_ss2"]


def _simulator(gl, name):
    if name != "C2_psf_ss2":
        wl = gl.workloads.make(name, num_pix=NUM_PIX, batch=1)
        return gl.LensSimulator(wl.phys_model, wl.sim_config, bs=1)
    from gigalens_amd.simulator import SimulatorConfig
    wl = gl.workloads.make("C2", num_pix=NUM_PIX, batch=1)
    u = np.arange(7, dtype=np.float64) - 3.0
    psf = np.exp(-0.5 * (u[:, None] ** 2 + u[None, :] ** 2) / 1.5 ** 2)
    cfg = SimulatorConfig(delta_pix=wl.sim_config.delta_pix, num_pix=NUM_PIX, supersample=2)
    return gl.LensSimulator(wl.phys_model, cfg, bs=1, supersampled_kernel=(psf / psf.sum()).astype(np.float32))


def measure(gl, name):
    """{str(B): {...}} of one workload: every integer the host layer reports about a call on B samples."""
    from gigalens_amd import _native
    L = _native.lib()
    m = _simulator(gl, name)._model
    out = {}
    for B in BATCHES:
        chunk, rows, row_floats, off = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        _native._check(L.gl_model_launch_shape(m._h, B, ctypes.byref(chunk), ctypes.byref(rows), ctypes.byref(row_floats),
                                               ctypes.byref(off)))
        rec = {"workspace_bytes": int(L.gl_workspace_bytes(m._h, B)), "chunk_px": chunk.value, "n_rows": rows.value,
               "row_floats": row_floats.value, "partial_offset_bytes": int(off.value), "num_pixels": int(m.N)}
        if m.num_linear():
            rec["lstsq_workspace_bytes"] = int(L.gl_lstsq_workspace_bytes(m._h, B))
        out[str(B)] = rec
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", WORKLOADS)
def test_launch_shape_and_workspace_layout_are_the_recorded_ones(gl, golden, name):
    assert next(iter(golden)) == "recorded_at"
    got, want = measure(gl, name), golden["cases"][name]
    assert sorted(want, key=int) == [str(B) for B in BATCHES]
    for B in BATCHES:
        assert got[str(B)] == want[str(B)], (name, B)
    if name in ("C3", "C3L", "C3D"):  # the models with linear columns: their solve's workspace is part of the pin
        assert all("lstsq_workspace_bytes" in want[str(B)] for B in BATCHES)


def test_the_pin_holds_a_tapered_launch(gl, golden):
    """C2 at 32 x 32 pixels and 1000 samples: 1000 workgroups over 768 resident slots leave a remainder of 232, the smallest shape
    at which the tapered end of the cost-ordered dispatch engages -- the rows a sample owns are twice its chunks.  Asserted on the
    recording and on the library, so the pin cannot silently hold the plain grid."""
    for rec in (golden["cases"]["C2"]["1000"], measure(gl, "C2")["1000"]):
        chunks = -(-rec["num_pixels"] // rec["chunk_px"])
        assert rec["n_rows"] == 2 * chunks
    plain = golden["cases"]["C2"]["768"]
    assert plain["n_rows"] == -(-plain["num_pixels"] // plain["chunk_px"])
