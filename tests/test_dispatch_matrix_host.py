"""CPU half of the dispatch matrix (tests/dispatch_cases.py): the specialised main-kernel instantiations in the shipped library are
exactly the ones the matrix declares, so every one of them has a float64-oracle case (tests/test_gpu_dispatch_matrix.py).  Reads
the code-object metadata the way tests/test_kernel_resources.py does."""
import os
import sys
from collections import Counter

import pytest

from tests import dispatch_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def library_names():
    import isa_flops as isa
    if not os.path.exists(isa.LIB):
        pytest.skip("library not built")
    return {DC.short_name(k) for k in isa.kernel_metadata(isa.code_object())}


def test_specialised_families_equal_the_declared_matrix(library_names):
    shipped = {k for k in library_names if DC.family(k)}
    declared = {k for k in DC.declared_names() if DC.family(k)}
    assert shipped - declared == set(), f"instantiations without an oracle case in tests/dispatch_cases.py: {sorted(shipped - declared)}"
    assert declared - shipped == set(), f"declared but not in the library: {sorted(declared - shipped)}"


def test_every_declared_name_is_in_the_library(library_names):
    missing = sorted(DC.declared_names() - library_names)
    assert not missing, missing


def test_no_basis_mode_specialisations(library_names):
    """IMG_BASIS (mode 4) always runs the interpreter (launch_main: generic_first), so no specialised kernel is built for it."""
    assert not [k for k in library_names if DC.family(k) and k.split("<", 1)[1].startswith("4,")]


def test_matrix_is_well_formed():
    ids = Counter(c.id for c in DC.CASES)
    assert not [i for i, n in ids.items() if n > 1], ids
    for c in DC.CASES:
        assert len(c.kernels) == len(DC.MODES), c.id
        for m, k in enumerate(c.kernels):
            assert k.split("<", 1)[1].startswith(f"{m},"), (c.id, m, k)  # the leading template argument is the mode
        assert set(c.env) <= set(DC.ENV_KNOBS), c.id
        assert 20 <= c.num_pix <= 64 and 1 <= c.batch <= 5, c.id
        if "Shapelets" in c.sources:
            assert c.n_max <= 10, c.id  # above n_max = 10 the runtime-order interpreter serves, not a specialised kernel


def test_generic_families_equal_the_declared_matrix(library_names):
    """The interpreter, cluster and component-per-wave cluster instantiations of launch_generic, all five modes: exactly the
    declared ones (the interpreter fallbacks of the tile cases count)."""
    shipped = {k for k in library_names if DC.generic_family(k)}
    declared = {k for k in DC.declared_names() if DC.generic_family(k)}
    assert shipped - declared == set(), f"instantiations without an oracle case in tests/dispatch_cases.py: {sorted(shipped - declared)}"
    assert declared - shipped == set(), f"declared but not in the library: {sorted(declared - shipped)}"


def test_generic_matrix_is_well_formed():
    ids = Counter(c.id for c in DC.CASES + DC.GENERIC_CASES)
    assert not [i for i, n in ids.items() if n > 1], ids
    for c in DC.GENERIC_CASES:
        assert len(c.kernels) in (1, len(DC.MODES)), c.id
        modes = (4,) if c.basis else range(len(DC.MODES))
        for m, k in zip(modes, c.kernels):
            assert DC.generic_family(k), (c.id, k)
            assert k.split("<", 1)[1].startswith(f"{m},"), (c.id, m, k)  # the leading template argument is the mode
        assert c.basis == c.lstsq, c.id  # the basis stack needs least-squares lights; the other modes need amplitudes
        assert set(c.env) <= set(DC.GENERIC_ENV_KNOBS), c.id
        assert 20 <= c.num_pix <= 64 and 1 <= c.batch <= 5, c.id
        if "Shapelets" in c.sources:
            assert c.n_max <= 20, c.id
        if "cluster" in c.kernels[-1]:  # N x NFW + Sersic / SersicEllipse, within the 8 + 20 capacity
            assert set(c.lenses) == {"NFW"} and not c.lens_light and len(c.lenses) <= 8 and len(c.sources) <= 20, c.id


def test_cluster_kernels_have_pixel_region_cases():
    """The pixel-list path of both cluster kernels, and of the component-per-wave kernel with two halos per wave and three
    elliptical sources per wave, runs in at least one case each; so does the zeroing of the basis stack outside a region."""
    pix = [c.kernels for c in DC.GENERIC_CASES if c.pix_region]
    assert any("gl_cluster_kernel<" in k[1] for k in pix)
    assert any(k[1] == "gl_clusterw_kernel<1, glk::CwLensNfw<2>, 3, true, 3>" for k in pix)
    assert sum(1 for k in pix if "cluster" in k[-1]) >= 3
    assert sum(1 for k in pix if len(k) == 1) >= 2


def test_pair_kernels_have_whole_and_ragged_cases():
    """Every pair kernel is run on whole 512-pixel tiles with an error map and on a ragged grid without one."""
    by_kernel = {}
    for c in DC.CASES:
        if DC.family(c.kernels[0]) == "gl_pair_kernel":
            by_kernel.setdefault(c.kernels, []).append(c)
    assert len(by_kernel) == 8
    for names, cases in by_kernel.items():
        assert any(c.num_pix ** 2 % 512 == 0 and c.err and not c.pix_region for c in cases), names[0]
        assert any(c.num_pix ** 2 % 512 and not c.err for c in cases), names[0]
