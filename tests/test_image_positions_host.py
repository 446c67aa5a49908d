"""Lens-equation solver: the C ABI's argument checks, no device needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def native():
    from gigalens_amd import _native
    try:
        _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))
    return _native


def test_image_positions_refuses_bad_arguments(native):
    lib = native.lib()
    assert lib.gl_image_positions_workspace_bytes(None, 4, 2, 64, 8) == 0
    null = ctypes.c_void_p(0)
    rc = lib.gl_image_positions(None, null, 4, null, null, 2, -1.0, 1.0, -1.0, 1.0, 64, 8, 1e-6, 30, null, null, null, null, 0,
                                null)
    assert rc == -1  # GL_EINVAL
    assert b"null" in lib.gl_last_error()


def test_stage_counts_refuses_bad_arguments(native):
    lib = native.lib()
    null = ctypes.c_void_p(0)
    assert lib.gl_image_positions_stage_counts(None, 4, 2, 64, null, 0, null, null, null) == -1  # GL_EINVAL
    assert b"null" in lib.gl_last_error()
    # ... and its twin for a workspace of the solver on lens planes: the model, the workspace and either output
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks return before reading any
    p = ctypes.addressof(buf)
    full = [p, 4, 2, 64, p, 4096, p, p, None]
    for entry in (lib.gl_image_positions_stage_counts, lib.gl_multiplane_image_positions_stage_counts):
        for null_at in (0, 4, 6, 7):
            args = list(full)
            args[null_at] = None
            assert entry(*args) == -1, null_at
            assert b"null argument" in lib.gl_last_error()
