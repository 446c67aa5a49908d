"""The multi-plane gradient without a GPU: the float64 reference against a closed form, the kernel's specification (the reverse
recursion of tests/multilens_grad_cases.py) against autograd on the whole composition, and the C ABI of the three gradient entries."""
import ctypes

import numpy as np
import pytest

from tests import multilens_cases as MC
from tests import multilens_grad_cases as GC

NEW_ENTRIES = ("gl_multiplane_simulate_bwd", "gl_multiplane_loglike_fwd_bwd", "gl_multiplane_logprob_fwd_bwd")


def test_two_shear_planes_closed_form_gradient():
    """beta = (I - T1 G1 - T2 G2 (I - C12 G1)) theta: the gradient of a quadratic loss in beta with respect to the four gamma, from
    the float64 reference (autograd) and from the reverse recursion, equals the closed-form derivative to 1e-12."""
    g = GC.two_shear_gradients()
    scale = np.abs(g["closed"]).max()
    assert scale > 1e-2 and (np.abs(g["closed"]) > 1e-3 * scale).all(), g["closed"]  # no gradient of the four vanishes
    for what in ("autograd", "recursion"):
        err = np.abs(g[what] - g["closed"]).max() / scale
        print(f"two Shear planes, {what} vs closed form: {err:.3e}")
        assert err <= 1e-12, (what, g[what], g["closed"])


@pytest.mark.parametrize("name", MC.MAP_CASES)
def test_reverse_recursion_equals_autograd(name):
    """abar / thetabar in reverse plane order, fed with every lens's own float64 Jacobian, is autograd on the composition."""
    auto, rec = GC.map_case_gradients(name)
    assert auto.shape == rec.shape and np.isfinite(auto).all() and np.abs(auto).max() > 0
    err = np.abs(rec - auto).max() / np.abs(auto).max()
    print(f"{name}: reverse recursion vs autograd {err:.3e} ({auto.size} gradient elements)")
    assert err <= 1e-10, (name, err)


def test_reference_differentiates_cleanly_on_the_zoo_cases():
    """Finite gradient, no NaN pixel, a non-zero scale in every column (what the GPU tests assert again before they use the metric)."""
    for name in GC.ZOO_CASES:
        c, obs, _, ll, g, _ = GC.grad_data(name)
        scale = np.abs(g).max(axis=0)
        print(f"{name}: {g.shape[1]} columns, scales {scale.min():.3g} .. {scale.max():.3g}")
        assert g.shape == (c["B"], c["phys"]._packing().P) and np.isfinite(ll).all()


def _library():
    """The built library; a load error is a failure, not a skip."""
    import os

    from gigalens_amd import _native
    assert os.path.exists(_native.lib_path()), "library not built: python -c 'import __graft_entry__ as g; g.build()'"
    return _native.lib()


def test_new_entries_are_exported_and_bound():
    from gigalens_amd import _native
    L = _library()
    for name in NEW_ENTRIES:
        assert name in _native.SYMBOLS, name
        assert hasattr(L, name), name
    for method in ("multiplane_simulate_bwd", "multiplane_loglike_grad", "multiplane_logprob"):
        assert callable(getattr(_native.Model, method, None)), method


def test_null_model_is_refused_without_a_gpu():
    """A null model is answered with GL_EINVAL before anything touches the GPU (the null checks behind a live model need a device:
    tests/test_gpu_multilens_grad.py::test_refusals)."""
    L = _library()
    GL_EINVAL = -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gl_multiplane_simulate_bwd(None, p, p, 1, p, p, 256, None) == GL_EINVAL and b"null" in L.gl_last_error()
    assert L.gl_multiplane_loglike_fwd_bwd(None, p, p, None, None, 0.1, 100.0, 1, p, p, p, p, 256, None) == GL_EINVAL
    assert L.gl_multiplane_logprob_fwd_bwd(None, p, p, None, None, 0.1, 100.0, 1, p, p, p, p, 1.0, 1, p, 256, None) == GL_EINVAL
    assert b"null" in L.gl_last_error()
