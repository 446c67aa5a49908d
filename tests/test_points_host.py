"""The launch-edge matrix of the point-likelihood kernels (tests/points_cases.py) without a GPU: the shapes and their thread counts on
both sides of every 64-thread workgroup edge, the measurement kinds every accumulating launch meets, the input conditions of every
case, the float32 yardsticks under their caps, and the new recipes pinned to the restatements of tests/mp_positions_cases.py,
tests/flux_cases.py and tests/tdelay_cases.py on their own small cases."""
import os
import re

import numpy as np
import pytest

from tests import flux_cases as FC
from tests import mp_positions_cases as PC
from tests import points_cases as X
from tests import tdelay_cases as TC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gigalens_amd", "csrc")
U = 2.0 ** -24
# A value of these terms is a sum of at most a few hundred float32 addends none of which cancels by more than a factor of ~20 (flux
# and delay residuals of 5 - 20 % of the measurement): a float32 yardstick beyond 256 u would point at an input that cancels, which
# the matrix is not about.  The delay values keep the ceilings of tests/tdelay_cases.py.
VALUE_CEILING = 256 * U
GRAD_CAP = 0.25  # of the gate of PC.grad_gate


# ---- 1: the matrix ---------------------------------------------------------------------------------------------------
# name: (B, F, J, B F, B J) as the design states them
TABLE = {"one": (1, 1, 1, 1, 1), "bf63": (9, 7, 20, 63, 180), "bf64": (8, 8, 22, 64, 176), "bf65": (13, 5, 16, 65, 208),
         "bj63": (7, 3, 9, 21, 63), "bj64": (8, 3, 8, 24, 64), "bj65": (5, 3, 13, 15, 65), "long": (3, 2, 14, 6, 42),
         "big": (33, 13, 41, 429, 1353), "b1": (1, 8, 22, 8, 22), "j4": (4, 1, 1, 4, 4), "j5": (5, 1, 1, 5, 5)}


def test_shapes_are_the_table():
    for name, (B, F, J, BF, BJ) in TABLE.items():
        b, sizes = X.SHAPES[name]
        assert (b, len(sizes), sum(sizes), b * len(sizes), b * sum(sizes)) == (B, F, J, BF, BJ), name
    b, sizes = X.SHAPES["many"]
    assert b == 2 and len(sizes) == 65 and set(sizes) == {1, 2} and b * len(sizes) == 130
    assert X.SHAPES["b1"][1] == X.SHAPES["bf64"][1]
    assert max(X.SHAPES["long"][1]) == 12 and max(max(s) for _, s in X.SHAPES.values()) == 12
    sets = {s: {shape for shape, t in X.CASES if t == s} for s in X.SETS}
    assert sets["plain"] == set(X.SHAPES)
    assert sets["scaled"] == {"bf63", "bf64", "bf65"}
    assert sets["planes"] >= {"bf63", "bf64", "bf65", "bj63", "bj64", "bj65", "big"}
    assert len(sets["zoo1"]) == 1


def test_lens_sets():
    plain, scaled, planes, zoo = (X.case("bj65", "plain"), X.case("bf65", "scaled"), X.case("bj65", "planes"), X.case("bj65", "zoo1"))
    names = lambda c: [type(l).__name__ for l in c["phys"].lenses]
    assert names(plain) == names(scaled) == names(planes) == ["EPL", "Shear", "SIE"]
    assert plain["P"] == 18 and plain["lens_cols"] == 13 and [type(s).__name__ for s in plain["phys"].source_light] == ["Sersic"]
    assert plain["scales"] is None and plain["phys_mp"] is None and all(fm["T"].tolist() == [1.0] for fm in plain["fams"])
    assert len(set(scaled["scales"])) == 2 and all(0 < s < 2 and s != 1.0 for s in scaled["scales"])
    k2 = PC.case("k2")
    assert planes["mp"].K == 2 and np.array_equal(planes["mp"].plane_of_lens, k2["mp"].plane_of_lens)
    assert np.array_equal(np.asarray(planes["mp"].lens_scales), np.asarray(k2["mp"].lens_scales))
    between = [fm["T"][-1] == 0 for fm in planes["fams"]]
    assert any(between) and not all(between)  # families between the planes and behind both
    assert names(zoo) == ["DPIS", "DPIEP", "TNFW", "NFW_ELLIPSE", "DPIESubhalo"] and len(zoo["catalogue"]["lum"]) == 3
    assert zoo["P"] == zoo["lens_cols"] == 26
    for c in (plain, scaled, planes, zoo):
        assert X.packed_rows(c).shape == (c["B"], c["P"])
        assert sum(len(d) for d in c["params"]["lens_mass"]) == c["lens_cols"]


def test_samples_follow_the_recipe_of_b65():
    lp = TC._lens_sets()["epl"][1]
    mine, theirs = X._rows(lp, 65), TC.case("b65")["params"]["lens_mass"]
    for d, e, src in zip(mine, theirs, lp):
        for k in d:
            assert np.array_equal(d[k][3:], e[k][3:]), k            # beyond the three rows: the recipe, bit for bit
            assert np.array_equal(d[k][:3], np.asarray(src[k])), k  # the three rows themselves
    big = X.case("big", "plain")["params"]["lens_mass"][0]["theta_E"]
    assert big.shape == (33,) and len(set(big.tolist())) == 33 and np.abs(big[3:] / big[np.arange(3, 33) % 3] - 1).max() <= 0.0201


# ---- 2: thread counts ------------------------------------------------------------------------------------------------
def _grids(c):
    """The four grid formulas of ``run_positions`` restated from its text: threads B J (P1), B F (P2, fluxes, delays), B J lens_params
    (P3, the delay gradient), B (P + 1) (P4) -- with J, F, lens_params and P taken from the data the library receives: the
    concatenated positions, the family list, the columns of the lens group and the width of the packed rows."""
    J, F = int(np.concatenate([fm["x"] for fm in c["fams"]]).size), len(c["fams"])
    L = sum(len(d) for d in c["params"]["lens_mass"])
    P = X.packed_rows(c).shape[1]
    return dict(p1=c["B"] * J, p2=c["B"] * F, p3=c["B"] * J * L, p4=c["B"] * (P + 1))


def test_thread_counts_are_those_of_run_positions():
    text = open(os.path.join(CSRC, "gl_api_points.hip")).read()
    body = text[text.index("int run_positions("):text.index("extern \"C\"")]
    assert "return dim3((unsigned)((n + 63) / 64))" in body
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), blocks\(\(long long\)([^)]*)\)\)?, dim3\((\w+)\)", body)
    want = {"gl_pos_p1_kernel": "B * a.J", "gl_mp_pos_p1_kernel": "B * a.J", "gl_pos_p2_kernel": "B * a.F", "gl_pos_flux_kernel": "B * a.F",
            "gl_pos_tdelay_kernel": "B * a.F", "gl_pos_p3_kernel": "B * a.J * m->lens_params", "gl_mp_pos_p3_kernel": "B * a.J * m->lens_params",
            "gl_pos_tdelay_grad_kernel": "B * a.J * m->lens_params", "gl_pos_p4_kernel": "B * (a.P + 1"}
    seen = {}
    for kernel, n, wg in launches:
        assert wg in ("64", "MP_POS_WG"), (kernel, wg)
        assert seen.setdefault(kernel, n) == n
    assert seen == want, seen
    assert "constexpr int MP_POS_WG = 64;" in open(os.path.join(CSRC, "gl_multiplane_pos.hip.h")).read()
    for shape, s in X.CASES:
        c = X.case(shape, s)
        assert X.thread_counts(c) == _grids(c), (shape, s)
    # the figures of the module's docstring
    assert X.thread_counts(X.case("big", "plain")) == dict(p1=1353, p2=429, p3=17589, p4=627)
    assert X.thread_counts(X.case("bj65", "zoo1")) == dict(p1=65, p2=15, p3=1690, p4=135)
    assert X.thread_counts(X.case("j4", "planes")) == dict(p1=4, p2=4, p3=52, p4=56)


def test_every_count_has_a_case_on_both_sides_of_64():
    edges = X.edge_counts()
    for k in ("p1", "p2"):  # one thread per element: 63, 64 and 65 exactly
        counts = {n for n, _, _ in edges[k]}
        assert {63, 64, 65} <= counts, (k, sorted(counts))
    for k in ("p3", "p4"):  # strides of L resp. P + 1 threads: 64 itself is no multiple of any of them ...
        strides = {s for _, s, _ in edges[k]}
        assert all(64 % s for s in strides), strides
        below = [(n, s, name) for n, s, name in edges[k] if 64 - s < n <= 64]
        above = [(n, s, name) for n, s, name in edges[k] if 64 < n <= 64 + s]
        print(k, "below", below, "above", above)
        assert below and above, (k, edges[k][:6])  # ... so: the last full stride below the edge, and the first across it
    # more than one workgroup, and a last workgroup that is partly empty, for every count
    for k in edges:
        assert any(n > 128 and n % 64 for n, _, _ in edges[k]), k
    # the per-thread LDS columns of the plane kernel: a workgroup with all 64 lanes live, and lanes 45 ... 63 live
    planes = [X.thread_counts(X.case(shape, s))["p1"] for shape, s in X.CASES if s == "planes"]
    assert max(planes) >= 64 and {63, 64, 65} <= set(planes)


# ---- 3: the measurements every accumulating launch meets -------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in X.SHAPES if X.has_pairs(s)])
def test_measurement_kinds(shape):
    B, sizes = X.SHAPES[shape]
    m, F = X.modes(shape), len(sizes)
    assert all(kind == "none" for kind, n in zip(m, sizes) if n == 1)
    want = {"full", "one_nan", "none"} if (F >= 3 and max(sizes) >= 3) else {"full", "one_nan"} if shape == "long" else {"full", "none"}
    assert set(m) == want, (shape, m)
    c = X.case(shape, "plain")
    for fm, kind, n in zip(c["fams"], m, sizes):
        for key in ("flux", "delay"):
            v = fm[key]
            count = 0 if v is None else int(np.count_nonzero(~np.isnan(v)))
            assert count == {"none": 0, "full": n, "one_nan": n - 1}[kind], (shape, key, kind)
            assert count != 1
        measured = 0 if fm["delay"] is None else int(np.count_nonzero(~np.isnan(fm["delay"])))
        if measured and np.isnan(fm["scale"]):
            assert measured >= 3  # a profiled scale takes three or more times
    scales = [np.isnan(fm["scale"]) for fm in c["fams"] if fm["delay"] is not None]
    assert not all(scales) and (any(scales) or shape == "many"), (shape, scales)  # given and profiled scales
    at_or_beyond_64 = {m[i % F] for i in range(64, B * F)}
    if shape == "big":
        assert at_or_beyond_64 == {"full", "one_nan", "none"}
    elif shape == "many":
        assert at_or_beyond_64 == {"full", "none"}
    elif shape == "bf65":
        assert at_or_beyond_64 == {"one_nan"}
    else:
        assert B * F <= 64


# ---- 4: input conditions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lens_set", X.CASES, ids=X.IDS)
def test_conditions(shape, lens_set):
    c = X.case(shape, lens_set)
    min_det, min_pix = PC.conditions(c)
    det = X.det_signs(c)
    margin = np.abs(det).min()
    print(f"{shape}-{lens_set}: min |det A| {min_det:.3f}, {min_pix:.1f} pixels to the nearest centre, det A within [{det.min():.3f}, {det.max():.3f}]")
    assert min_det >= PC.MIN_DET and min_pix >= PC.MIN_PIX
    assert (np.sign(det) == np.sign(det[:, :1])).all() and margin >= 0.05  # no image near a change of parity between samples
    for fm in c["fams"]:  # lattice points
        assert np.array_equal(fm["x"], PC.lattice(*np.rint(fm["x"] / PC.MC.PIX).astype(int)))
        assert np.array_equal(fm["y"], PC.lattice(*np.rint(fm["y"] / PC.MC.PIX).astype(int)))
    if "delays" in X.held(shape, lens_set):
        d = X.min_centre(c)
        print(f"   the line integral's paths keep {d:.3f} arcsec from every profile centre")
        assert d >= TC.MIN_CENTRE


# ---- 5: the float32 yardsticks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lens_set", X.CASES, ids=X.IDS)
def test_yardsticks_are_under_their_caps(shape, lens_set):
    for term in X.held(shape, lens_set):
        c, ref, yard = X.data(shape, lens_set, term)
        print(f"{shape}-{lens_set} {term}: " + ", ".join(f"{k} {'-' if v is None else format(v, '.2e')}" for k, v in yard.items()))
        assert np.isfinite(ref["log_like"]).all() and np.isfinite(ref["chi2"]).all() and np.isfinite(ref["grad"]).all()
        assert ref["fam"].shape == (c["B"], len(c["fams"]), 2) and ref["grad"].shape == (c["B"], c["P"])
        assert (ref["grad"][:, c["lens_cols"]:] == 0).all()  # the columns of no lens
        assert np.allclose(ref["fam"].sum(axis=1), np.stack([ref["log_like"], ref["chi2"]], axis=-1), rtol=1e-13, atol=0)
        for k in X.VALUE_KEYS[term]:
            ceiling = TC.YARD_CEILING.get({"fam_ll": "log_like", "fam_chi2": "chi2"}.get(k, k), VALUE_CEILING) if term == "delays" else VALUE_CEILING
            # the gate of a value is 4 x its yardstick (the rule of the per-term GPU tests): a quarter of it by construction -- what
            # can go wrong is the yardstick itself, which stays under a ceiling that does not come from the kernels
            assert yard[k] <= ceiling, (term, k, yard[k], ceiling)
        if term == "delays":
            assert yard["grad"] is None  # (tests/tdelay_cases.py has no float32 gradient: psi comes from the host build there)
            # what stands in for it: no lens column of the delay gradient may be a sum that cancels to nothing -- a column's scale
            # against the scale of all columns.  `many` (two-image families, both measured) fails it on the two Shear columns, where
            # the sum is identically 0: its delay term runs inside the fused sums only (X.terms_of)
            cols = np.abs(ref["grad"][:, :c["lens_cols"]]).max(axis=0)
            dead = np.flatnonzero(cols <= 1e-9 * cols.max()).tolist()
            print(f"   delay gradient: column scales from {cols.min():.3e} to {cols.max():.3e}, cancelling columns {dead}")
            assert dead == ([6, 7] if shape == "many" else []), (shape, dead)
            assert (term in X.terms_of(shape, lens_set)) == (not dead)
        else:
            assert yard["grad"] <= GRAD_CAP, (term, yard["grad"])
        none = [k for k, kind in enumerate(X.modes(shape)) if kind == "none"] if term != "positions" and X.has_pairs(shape) else []
        assert (ref["fam"][:, none] == 0).all()  # a family without a measurement: exactly 0
    for combo in X.combos_of(shape, lens_set):
        c, ref, yard = X.fused(shape, lens_set, combo)
        print(f"{shape}-{lens_set} fused {'+'.join(combo)}: " + ", ".join(f"{k} {'-' if v is None else format(v, '.2e')}" for k, v in yard.items()))
        assert np.isfinite(ref["log_prob"]).all() and (ref["red_chi2"] >= 0).all()
        ceiling = max(TC.YARD_CEILING.values()) if "delays" in combo else VALUE_CEILING
        assert max(yard["log_prob"], yard["red_chi2"], yard["fam_ll"], yard["fam_chi2"]) <= ceiling
        assert (yard["grad"] is None) == ("delays" in combo) and (yard["grad"] is None or yard["grad"] <= GRAD_CAP)


# ---- 6: the recipes against the modules they extend ------------------------------------------------------------------
def _same(a, b):
    return (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_extended_patterns_reproduce_the_old_data():
    for name in ("plain", "one_nan", "partial"):
        c = FC.case(name)
        bare = [{k: v for k, v in fm.items() if k not in ("flux", "flux_err")} for fm in c["fams"]]
        rule = {"plain": None, "one_nan": lambda f, j: not (f == 1 and j == 2), "partial": lambda f, j: f == 0 and j != 1}[name]
        for fm, old in zip(X.with_fluxes(c, bare, rule), c["fams"]):
            assert _same(fm["flux"], old["flux"]) and _same(fm["flux_err"], old["flux_err"]), name
    for name, rule, given in (("quad", None, ()), ("quad_nan", lambda k, j: j != 2, ()), ("b65", None, (1,)),
                              ("two_fams", lambda k, j: True if k == 0 else None, ()), ("cat", None, ())):
        c = TC.case(name)
        bare = [{k: v for k, v in fm.items() if k not in ("delay", "delay_err", "scale")} for fm in c["fams"]]
        for fm, old in zip(X.with_delays(dict(c, fams=bare), bare, rule, given), c["fams"]):
            assert _same(fm["delay"], old["delay"]) and _same(fm["delay_err"], old["delay_err"]), name
            assert _same(fm["scale"], old["scale"]), name
    long = X.case("long", "plain")["fams"][0]  # ... and cycle beyond five images
    assert long["flux"].size == 12 and np.array_equal(long["delay_err"], np.resize(np.asarray(TC.ERRORS, np.float32), 12))


def test_family_sums_reproduce_the_old_references():
    _, ref, _ = PC.data("k2")
    c = PC.case("k2")
    got = X.evaluate(dict(c, catalogue=None), "positions")
    n_position = 2.0 * sum(fm["x"].size for fm in c["fams"])
    assert np.allclose(got["log_like"], ref["log_like"], rtol=1e-13) and np.allclose(got["chi2"] / n_position, ref["red_chi2"], rtol=1e-13)
    assert np.allclose(got["grad"], ref["grad"], rtol=1e-10, atol=1e-9 * np.abs(ref["grad"]).max())
    for name in ("plain", "partial"):
        _, ref, _ = FC.data(name)
        got = X.evaluate(dict(FC.case(name), catalogue=None), "fluxes")
        for k in ("log_like", "chi2", "S", "model"):
            assert np.allclose(got[k], ref[k], rtol=1e-13, equal_nan=True), (name, k)
        assert np.allclose(got["grad"], ref["grad"], rtol=1e-10, atol=1e-9 * np.abs(ref["grad"]).max())
    _, ref, _ = TC.data("two_fams")
    got = X.evaluate(TC.case("two_fams"), "delays")
    for k in ("log_like", "chi2", "scale", "offset", "model"):
        assert np.allclose(got[k], ref[k], rtol=1e-12, equal_nan=True), k
    assert np.allclose(got["grad"], ref["grad"], rtol=1e-9, atol=1e-9 * np.abs(ref["grad"]).max())
    assert (got["fam"][:, 1] == 0).all()  # the delay-less family
