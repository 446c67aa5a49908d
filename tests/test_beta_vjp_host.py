"""CPU-side checks of the ray-shoot VJP's boundary (gl_lens_maps_vjp): the symbols are exported and bound, the methods exist,
and the argument validation answers without a device -- null arguments and sizes <= 0 are refused before the model is read."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


def test_symbols_exported_and_bound(native):
    lib = native.lib()
    for name in ("gl_lens_maps_vjp", "gl_lens_maps_vjp_workspace_bytes"):
        assert name in native.SYMBOLS
        assert getattr(lib, name).argtypes == native.SYMBOLS[name][1]
    assert callable(native.Model.lens_maps_vjp)
    from gigalens_amd.simulator import LensSimulator
    assert callable(LensSimulator.beta_vjp)


def test_argument_validation_without_gpu(native):
    lib = native.lib()
    GL_EINVAL = -1
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    assert lib.gl_lens_maps_vjp_workspace_bytes(None, 4, 100) == 0
    assert lib.gl_lens_maps_vjp_workspace_bytes(p, 0, 100) == 0
    assert lib.gl_lens_maps_vjp_workspace_bytes(p, -1, 100) == 0
    assert lib.gl_lens_maps_vjp_workspace_bytes(p, 4, 0) == 0
    assert lib.gl_lens_maps_vjp_workspace_bytes(p, 4, -5) == 0
    full = [p, p, 4, p, p, 100, 1, p, p, p, 4096, None]
    for null_at in (0, 1, 3, 4, 7, 8, 9):  # model, params, x, y, cot, grad_params, workspace
        args = list(full)
        args[null_at] = None
        assert lib.gl_lens_maps_vjp(*args) == GL_EINVAL, null_at
        assert b"null argument" in lib.gl_last_error()
    for B, n_pts in ((0, 100), (-3, 100), (4, 0), (4, -1)):
        args = list(full)
        args[2], args[5] = B, n_pts
        assert lib.gl_lens_maps_vjp(*args) == GL_EINVAL, (B, n_pts)
        assert b"must be positive" in lib.gl_last_error()
