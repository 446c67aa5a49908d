"""CPU-side checks of the lens-equation solver on lens planes (gl_multiplane_image_positions): the symbols are exported, declared and
bound; the argument checks that need no device answer; and the float64 references of tests/mp_images_cases.py agree with the closed
forms and meet the conditions the GPU tests (tests/test_gpu_mp_images.py) put on the chosen sources.

(A model cannot be created without a device, so the growth of the workspace with the number of planes is asserted beside the GPU
tests, in test_gpu_mp_images.py::test_native_rules_and_workspace.)"""
import ctypes
import os

import numpy as np
import pytest

from tests import mp_images_cases as C
from tests import multilens_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gl_multiplane_image_positions_workspace_bytes", "gl_multiplane_image_positions")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


def test_symbols_exported_declared_and_bound(native):
    lib = native.lib()
    raw = ctypes.CDLL(native.lib_path())
    header = open(os.path.join(ROOT, "include", "gigalens_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in native.SYMBOLS and f" {name}(" in header, name
        assert getattr(lib, name).argtypes == native.SYMBOLS[name][1]
    assert callable(native.Model.multiplane_image_positions)
    import inspect

    from gigalens_amd.simulator import LensSimulator
    assert inspect.signature(LensSimulator.image_positions).parameters["source_redshifts"].default is None


def test_argument_validation_without_gpu(native):
    lib = native.lib()
    GL_EINVAL = -1
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    # the workspace size is 0 for a null model whatever the sizes (the other bad arguments need a model: the GPU tests)
    for args in ((None, 4, 2, 64, 8), (None, 0, 2, 64, 8), (None, 4, 0, 64, 8), (None, 4, 2, 0, 8), (None, 4, 2, 64, 0)):
        assert lib.gl_multiplane_image_positions_workspace_bytes(*args) == 0, args
    T = (ctypes.c_float * 4)(1.0, 0.5, 1.0, 0.5)
    full = [p, p, 4, p, p, 2, T, 2, -1.0, 1.0, -1.0, 1.0, 8, 8, 1e-6, 30, p, p, p, p, 4096, None]
    for null_at in (0, 1, 3, 4, 6, 16, 17, 18):  # model, params, src_x, src_y, targets, out, n_images, n_dropped
        args = list(full)
        args[null_at] = None
        assert lib.gl_multiplane_image_positions(*args) == GL_EINVAL, null_at
        assert b"null argument" in lib.gl_last_error()


def test_two_shear_reference_is_the_closed_form():
    """The float64 solver on the two-shear recursion returns the single root ``A^-1 beta_s`` with ``mu = 1 / det A`` -- and none for the
    source whose root lies outside the window."""
    (phys, _, mp, lp, T, A), sx, sy, roots, mu = C.two_shear_sources()
    assert abs(A[0, 1] - A[1, 0]) > 1e-3  # the case is not symmetric
    x_lo, x_hi, y_lo, y_hi = C.SHEAR_WINDOW
    inside = [x_lo < r[0] < x_hi and y_lo < r[1] < y_hi for r in roots]
    assert inside == [True, True, False]
    for s in range(3):
        for n in (2, 16):
            ref = C.solve64(phys, mp, lp, 0, T, sx[0, s], sy[0, s], C.SHEAR_WINDOW, n)
            if not inside[s]:
                assert len(ref) == 0
                continue
            assert ref.shape == (1, 3)
            assert np.hypot(ref[0, 0] - roots[s, 0], ref[0, 1] - roots[s, 1]) <= 1e-12 and abs(ref[0, 2] - mu) <= 1e-12 * abs(mu)


def test_two_sis_reference_has_the_closed_form_roots():
    """Coaxial SIS planes, sources on the axis: the float64 solver holds both outer images ``x = beta +- (T_1 tE1 + T_2 tE2)`` (where the
    ray passes both centres on the same side), on the axis."""
    for beta in C.SIS_BETA:
        (phys, _, mp, lp, T, *_), xs = C.two_sis_closed_form(beta)
        assert len(xs) == 2
        ref = C.solve64(phys, mp, lp, 0, T, beta, 0.0, C.SIS_WINDOW, 2 * C.SIS_CELLS)
        assert len(ref) >= 2 and np.abs(ref[:, 1]).max() <= 1e-9
        for x in xs:
            assert np.abs(ref[:, 0] - x).min() <= 1e-9, (beta, x, ref)
    # no vertex of the window on the centre of either plane: the axis point of the vertices' rows and columns is 0.37 PIX off
    xs, ys = (np.float32(C.SIS_WINDOW[0]) + np.arange(C.SIS_CELLS + 1, dtype=np.float32) * np.float32(4.0 / C.SIS_CELLS) for _ in range(2))
    assert np.abs(xs).min() > 0.3 * MC.PIX and np.abs(ys).min() > 0.3 * MC.PIX


@pytest.mark.parametrize("name", sorted(C.GENERAL))
def test_general_sources_meet_the_fold_condition(name):
    """At most a quarter of the (sample, source) pairs of a general case go to the fold rule (two images closer than two cells), the
    two sources sit at different redshifts, some pair that is compared holds three or more images above the |mu| gate, and every
    compared image lies a cell or more from the centre of every EPL / SIE / SIS in front of its source."""
    z, sx, sy = C.general_sources(name)
    assert z[0] != z[1] and sx.shape == sy.shape == (3, 2)
    c = MC.map_case(name)
    assert not np.array_equal(c["mp"].target_scales(z[0]), c["mp"].target_scales(z[1]))
    ref = C.general_reference(name)
    folds = [k for k, r in ref.items() if C.fold_pair(r, C.GENERAL_WINDOW, C.GENERAL_CELLS)]
    assert 4 * len(folds) <= len(ref), folds
    assert max(int(np.sum(np.abs(r[:, 2]) >= C.MU_MIN)) for k, r in ref.items() if k not in folds) >= 3
    # no compared image on the cell of a singular lens centre (mp_images_cases.singular_centre_cells)
    for (b, s), r in ref.items():
        if (b, s) in folds:
            continue
        for xi, yi, mi in r:
            if abs(mi) >= C.MU_MIN:
                d = C.singular_centre_cells(name, b, c["mp"].target_scales(z[s]), xi, yi)
                print(f"{name} b={b} s={s} image ({xi:+.4f}, {yi:+.4f}): {d:.2f} cells from the nearest singular centre")
                assert d >= 1.0, (b, s, xi, yi, d)


def test_four_plane_reference_is_multiply_imaged():
    phys, _, mp, lp = C.four_plane_case()
    assert mp.K == 4
    ref = C.solve64(phys, mp, lp, 0, mp.target_scales(2.0), 0.05, 0.03, C.GENERAL_WINDOW, 2 * C.GENERAL_CELLS)
    assert len(ref) >= 3 and not C.fold_pair(ref, C.GENERAL_WINDOW, C.GENERAL_CELLS)
