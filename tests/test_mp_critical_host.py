"""CPU-side checks of the critical curves on lens planes (gl_multiplane_critical_curves): the float64 references of
tests/mp_critical_cases.py agree with the closed form and with ``multilens_cases.maps`` / ``maps_hessian`` and meet the conditions the
GPU tests (tests/test_gpu_mp_critical.py) put on the chosen windows; the symbols are exported, declared and bound; the argument
checks that need no device answer; the two new kernels use no private segment.

(A model cannot be created without a device, so the rules that need one -- a model without planes, ``n_planes``, the coupling rows, the
sizes, the workspace, and every rule of the Python surface that reaches a simulator -- are asserted beside the GPU tests, in
test_gpu_mp_critical.py::test_native_rules_and_workspace and ::test_python_rules.)"""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest

from tests import critical_cases as CC
from tests import mp_critical_cases as C
from tests import mp_images_cases as IC
from tests import multilens_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NEW_SYMBOLS = ("gl_multiplane_critical_curves_workspace_bytes", "gl_multiplane_critical_curves")
NEW_KERNELS = ("gl_mpcrit_map_kernel", "gl_mpcrit_refine_kernel")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from gigalens_amd import _native
    return _native


# ---- 1. the closed form, and the recursion fields against maps / maps_hessian --------------------------------------------------------------
@pytest.mark.parametrize("b", [0, 1, 2])
def test_closed_form_against_contour64(b):
    c = C.sis_shear_case()
    cf = C.sis_shear_closed_form(b)
    fields = C.recursion_fields(c["phys"], c["mp"], c["lens_params"], b, c["target"])
    ref = CC.contour64(fields, C.CF_WINDOW, C.CF_CELLS)
    assert not ref["open"] and ref["n_flagged"] == 0 and ref["n_ambiguous"] == 0
    assert len(ref["seg"]) >= 40 and np.all(ref["kind"] == 0) and CC.count_loops(ref["seg"]) == (1, 0)
    p = ref["seg"].reshape(-1, 2)
    d = p - cf["centre"]
    phi = np.arctan2(d[:, 1], d[:, 0])
    assert np.max(np.abs(np.hypot(d[:, 0], d[:, 1]) - cf["radius"](phi))) <= 1e-11
    assert np.max(np.abs(ref["cau"].reshape(-1, 2) - cf["caustic"](phi).T)) <= 1e-11
    # D along the closed-form curve, and the determinant lemma itself off the curve
    q = cf["point"](np.linspace(0.1, 6.2, 9))
    D, bx, by, omk = fields(q[0], q[1])
    assert np.max(np.abs(D)) <= 1e-12 and np.all(omk > 0.3)  # tangential: tr A / 2 ~ 1 / 2
    assert np.max(np.hypot(bx - cf["caustic"](np.linspace(0.1, 6.2, 9))[0], by - cf["caustic"](np.linspace(0.1, 6.2, 9))[1])) <= 1e-12
    x, y = np.array([0.7, -1.3, 2.1]), np.array([0.4, 0.9, -1.7])
    dx, dy = x - cf["centre"][0], y - cf["centre"][1]
    r = np.hypot(dx, dy)
    t = np.stack([-dy / r, dx / r])
    lemma = np.linalg.det(cf["M"]) * (1 - cf["theta_E"] / r * np.einsum("ik,ij,jk->k", t, np.linalg.solve(cf["M"], cf["N"]), t))
    assert np.max(np.abs(fields(x, y)[0] - lemma)) <= 1e-12
    # the inscribed polygon: below the closed-form area by at most pi h^2 / 3 (chords of at most sqrt(2) h on a convex curve)
    h = (C.CF_WINDOW[1] - C.CF_WINDOW[0]) / C.CF_CELLS
    assert 0 < cf["area"] - ref["area"][0] <= math.pi * h * h / 3
    assert abs(cf["perimeter"] / (2 * math.sqrt(math.pi * cf["area"])) - 1) < 0.01  # nearly a circle
    # C_12 enters the curve: without it (N = T_1 I) the radius differs by far more than any gate
    tt = np.stack([-np.sin(phi), np.cos(phi)])
    wrong = cf["theta_E"] * np.einsum("ik,ij,jk->k", tt, np.linalg.solve(cf["M"], np.float64(np.float32(c["target"][0])) * np.eye(2)), tt)
    assert np.max(np.abs(wrong - cf["radius"](phi))) > 1e-3


@pytest.mark.parametrize("name", MC.MAP_CASES)
def test_recursion_fields_equal_the_maps_at_float32_points(name):
    c = MC.map_case(name)
    x, y = MC.points(40)
    for b in range(3):
        f = C.recursion_fields(c["phys"], c["mp"], c["lens_params"], b, c["target"])
        D, bx, by, omk = f(x.astype(np.float64), y.astype(np.float64))
        hb = f.hessian(x.astype(np.float64), y.astype(np.float64))
        m = MC.maps(c["phys"], c["mp"], [{k: v[b:b + 1] for k, v in d.items()} for d in c["lens_params"]], x, y, c["target"])[:, :, 0]
        assert np.max(np.abs(np.stack([bx, by]) - m[:2])) <= 1e-13
        assert np.max(np.abs(D - (m[2] * m[5] - m[3] * m[4]))) <= 1e-12 and np.max(np.abs(omk - 0.5 * (m[2] + m[5]))) <= 1e-13
        assert np.max(np.abs(np.stack(hb[2:]) - np.stack([1 - m[2], -m[3], -m[4], 1 - m[5]]))) <= 1e-13
        if c["maps"] is MC.maps:  # no override differs: maps_hessian is the same Jacobian
            mh = MC.maps_hessian(c["phys"], c["mp"], [{k: v[b:b + 1] for k, v in d.items()} for d in c["lens_params"]], x, y,
                                 c["target"])[:, :, 0]
            assert np.max(np.abs(mh - m)) <= 1e-12
        else:  # the dPIS excess: maps_hessian is the reference of that case, and differs
            g = C.maps_fields(MC.maps_hessian, c["phys"], c["mp"], c["lens_params"], b, c["target"])(x, y)
            assert np.max(np.abs(g[0] - D)) > 1e-4 and np.max(np.hypot(g[1] - bx, g[2] - by)) <= 1e-13


# ---- 2., 3. the general cases: closed, unflagged, no ambiguous cell; float32 crosses the same edges ----------------------------------------
def _general():
    return [(name, s) for name in sorted(C.GENERAL) for s in range(len(C.GENERAL[name][0]))]


@pytest.mark.parametrize("name,s", _general())
def test_general_references_are_closed_and_float32_crosses_the_same_edges(name, s):
    c = MC.map_case(name)
    z, T = C.general_targets(name)
    _, window, n = C.GENERAL[name]
    assert 32 <= n <= 64 and abs(window[1] - window[0] - 6.0) < 1e-9 and abs(window[3] - window[2] - 6.0) < 1e-9
    for b in range(3):
        _, ref = C.general_reference(name, b, s)
        assert not ref["open"] and ref["n_flagged"] == 0 and ref["n_ambiguous"] == 0, (b, ref["open"], ref["n_flagged"], ref["n_ambiguous"])
        assert len(ref["seg"]) >= 20 and CC.count_loops(ref["seg"])[1] == 0
        D32 = C.vertex_plane(C.maps_fields(MC.maps, c["phys"], c["mp"], c["lens_params"], b, T[s], MC.F32), window, n)
        assert np.isfinite(D32).all()
        assert C.crossing_edges(D32) == set(ref["edges"]), (b, C.crossing_edges(D32) ^ set(ref["edges"]))
    if name == "epl_shear|sie":
        assert T[1][1] == 0 and T[1][0] > 0  # the second redshift lies between the planes
    if name == "nfw|dpie|sis":
        assert c["mp"].K == 3 and T[0][2] == 0 and T[0][1] > 0  # the first lies in front of the last plane


def test_dpis_and_four_plane_references():
    name, z, window, n = C.DPIS
    c = MC.map_case(name)
    assert c["maps"] is MC.maps_hessian
    T = c["mp"].target_scales(z[0])
    for b in range(3):
        D = C.vertex_plane(C.maps_fields(MC.maps_hessian, c["phys"], c["mp"], c["lens_params"], b, T), window, n)
        e64 = C.crossing_edges(D)
        e32 = C.crossing_edges(C.vertex_plane(C.maps_fields(MC.maps_hessian, c["phys"], c["mp"], c["lens_params"], b, T, MC.F32), window, n))
        assert len(e64) >= 20 and e64 == e32 and np.isfinite(D).all()
        border = np.concatenate([D[0], D[-1], D[:, 0], D[:, -1]])
        assert np.all(border > 0)  # closed inside the window
    phys, _, mp, lp = IC.four_plane_case()
    assert mp.K == 4
    _, ref = C.four_plane_reference()
    assert not ref["open"] and ref["n_flagged"] == 0 and ref["n_ambiguous"] == 0 and len(ref["seg"]) >= 40
    D32 = C.vertex_plane(C.maps_fields(MC.maps, phys, mp, lp, 0, mp.target_scales(2.0), MC.F32), C.FOUR_WINDOW, C.FOUR_CELLS)
    assert C.crossing_edges(D32) == set(ref["edges"])


# ---- 4., 5., 6. symbols, argument rules, Python surface ------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_bound(native):
    lib = native.lib()
    raw = ctypes.CDLL(native.lib_path())
    header = open(os.path.join(ROOT, "include", "gigalens_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in native.SYMBOLS and f" {name}(" in header, name
        assert getattr(lib, name).argtypes == native.SYMBOLS[name][1]
    assert len(native.SYMBOLS["gl_multiplane_critical_curves"][1]) == 23
    assert callable(native.Model.multiplane_critical_curves)
    from gigalens_amd.simulator import LensSimulator
    for fn in (LensSimulator.critical_curves,):
        assert inspect.signature(fn).parameters["source_redshifts"].default is None
    assert "source_redshifts" in LensSimulator.einstein_radius.__doc__
    src = inspect.getsource(LensSimulator._single_plane)
    assert "critical_curves(source_redshifts=...)" in src and "einstein_radius(source_redshifts=...)" in src


def test_argument_validation_without_gpu(native):
    lib = native.lib()
    GL_EINVAL = -1
    buf = ctypes.create_string_buffer(4096)  # stands for every non-null pointer; the checks below return before reading any
    p = ctypes.addressof(buf)
    # the workspace size is 0 for a null model whatever the sizes
    for args in ((None, 3, 2, 48, 384), (None, 0, 2, 48, 384), (None, 3, 0, 48, 384), (None, 3, 2, 0, 384), (None, 3, 2, 48, 0)):
        assert lib.gl_multiplane_critical_curves_workspace_bytes(*args) == 0, args
    T = (ctypes.c_float * 4)(1.0, 0.5, 1.0, 0.5)
    full = [p, p, 3, T, 2, 2, -1.0, 1.0, -1.0, 1.0, 8, 8, p, p, p, p, p, p, p, p, p, 4096, None]
    # model, params, targets, seg, cau, kind, n_seg, n_dropped, n_flagged, open, area
    for null_at in (0, 1, 3, 12, 13, 14, 15, 16, 17, 18, 19):
        args = list(full)
        args[null_at] = None
        assert lib.gl_multiplane_critical_curves(*args) == GL_EINVAL, null_at
        assert b"null argument" in lib.gl_last_error()


def test_python_surface_without_gpu():
    """What of the Python rules needs no simulator: the helper that turns the redshifts into couplings refuses both keywords at once,
    a model without a MultiPlane, and a redshift not behind the first plane (the calls themselves: test_gpu_mp_critical.py)."""
    from gigalens_amd.simulator import LensSimulator
    c = MC.map_case("epl_shear|sie")

    class Stub:
        _mp = c["mp"]
        phys_model = c["phys_mp"]
    mp, T = LensSimulator._source_targets(Stub(), [2.0, 0.8], 2, 1.0)
    assert T.shape == (2, 2) and T[1, 1] == 0 and T[1, 0] > 0 and T[0, 1] > 0
    with pytest.raises(ValueError, match="deflection_scale"):
        LensSimulator._source_targets(Stub(), 2.0, 1, 0.9)
    for bad in (0.5, 0.3, float("nan"), [2.0, 0.4]):
        with pytest.raises(ValueError, match="source_redshifts"):
            LensSimulator._source_targets(Stub(), bad, np.size(bad), 1.0)

    class Plain:
        _mp = None
        phys_model = c["phys"]
    with pytest.raises(ValueError, match="MultiPlane"):
        LensSimulator._source_targets(Plain(), 2.0, 1, 1.0)
    # the result dict of critical_curves from [B, S] native outputs: closed, the NaN areas and the warning per (sample, source)
    import torch
    B, S, M = 2, 3, 4
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    dropped = z(B, S, dtype=torch.int32)
    dropped[1, 2] = 5
    opened = z(B, S, dtype=torch.int32)
    opened[0, 1] = 1
    args = (z(B, S, M, 2, 2), z(B, S, M, 2, 2), z(B, S, M, dtype=torch.int32), z(B, S, dtype=torch.int32), dropped, z(B, S, dtype=torch.int32),
            opened, -torch.ones(B, S, 4))
    with pytest.warns(RuntimeWarning, match=r"5 segment\(s\) not returned over 1 \(sample, source\) pair"):
        res = LensSimulator._curves_result(*args, M, False, "(sample, source) pair(s)", 2)
    assert res["closed"].tolist() == [[True, False, True], [True, True, False]]
    assert torch.isnan(res["area_tangential"]).tolist() == [[False, True, False], [False, False, True]]
    assert res["area_radial"][0, 0] == 1.0 and tuple(res["caustic_area_radial"].shape) == (B, S)
    with pytest.raises(RuntimeError, match="not returned"):
        LensSimulator._curves_result(*args, M, True, "(sample, source) pair(s)", 2)


# ---- 7. the resource rule ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def metadata(native):
    import isa_flops as isa
    assert os.path.exists(isa.LIB), "library not built (__graft_entry__.build())"
    return isa.kernel_metadata(isa.code_object())


@pytest.mark.parametrize("pat", NEW_KERNELS)
def test_new_kernels_use_no_private_segment(metadata, pat):
    import isa_flops as isa
    hits = [k for k in metadata if pat in k]
    assert len(hits) == 1, (pat, hits)
    md = metadata[hits[0]]
    print(hits[0], {k: md[k] for k in md if k not in ("co",)})
    assert md["vgpr_spill_count"] == 0 and md["scratch_bytes"] == 0, (hits[0], md)
    ins = isa.disassemble(md["co"], md["symbol"])
    assert len(ins) > 100 and not [i for i in ins if i[1].startswith("scratch_")], hits[0]
