"""Conditions on the case list of tests/shp_edge_cases.py itself, from the float64 oracle alone (no GPU): the cases sit on the
edges they are there for -- the wave-tile counts that select 0, 1 or 2 chain rounds, the rank offsets, the three slope branches
of the cull -- and far enough from the table boundary and the cull thresholds that float32 cannot decide otherwise, so that
tests/test_gpu_shp_edges.py may assert the kernels' own counters as equalities.  The output lists, per case, the wave-tile
counts it pins and its clearances."""
from dataclasses import replace

import numpy as np
import pytest

from tests import shp_edge_cases as SE

TABLE = [c for c in SE.ALL_CASES if c.interpolate]


@pytest.fixture(scope="module")
def geo():
    """geometry of every case, as the launch it is declared for sees it (the fused solve for the lstsq cases) -- computed once"""
    cache = {}

    def get(case, **kw):
        key = (case.id, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = SE.geometry(case, **kw)
        return cache[key]
    return get


def _pairs(g):
    return {(int(a), int(b)) for a, b in zip(g.c0.ravel(), g.c1.ravel())}


def test_slot_maps_cover_the_image_once():
    """Both restated orders are permutations of the image on whole tiles; a ragged end repeats the last pixel only."""
    for n, blk in ((32, True), (32, False), (64, True), (96, True), (96, False)):
        j, valid = SE.slot_map(n * n, n, blk)
        assert valid.all() and np.array_equal(np.sort(j.ravel()), np.arange(n * n)), (n, blk)
    for n, blk in ((30, False), (28, False), (16, True), (48, True), (80, True)):   # blocked + ragged: the fused solve only
        j, valid = SE.slot_map(n * n, n, blk)
        assert np.array_equal(np.sort(j[valid]), np.arange(n * n)), (n, blk)
        assert (j[~valid] == n * n - 1).all() and (~valid).sum() == j.size - n * n
    # 96 x 96: six blocks per block row, so a step's four blocks straddle block rows (blocks 4, 5 | 6, 7 of step 1)
    j, _ = SE.slot_map(96 * 96, 96, True)
    rows = j[4:8, 0, 0] // 96
    assert list(rows) == [0, 0, 8, 8] and list(j[4:8, 0, 0] % 96) == [64, 80, 0, 16]


@pytest.mark.parametrize("case", SE.ALL_CASES, ids=[c.id for c in SE.ALL_CASES])
def test_case_geometry(case, geo):
    """Per case: the pinned (c0, c1) are there, at least one sample has live pixels, table-mode classification
    is settled by the margin (no pixel is left out of any comparison: the cap of 0.5 % is met with zero), the cull decisions
    are settled by theirs, and a culled tile holds no live pixel (what the cull rests on, for these exact inputs)."""
    g = geo(case, fused=case.lstsq)
    pairs = _pairs(g)
    print(f"{case.id}: {'blocked' if g.blocked else 'linear'}, {g.tiles // case.batch} wave-tiles / sample, beta_s "
          f"{[s.src[0] for s in case.samples]}")
    for b in range(case.batch):
        live_pairs = sorted({(int(a), int(c)) for a, c in zip(g.c0[b], g.c1[b]) if a + c})
        print(f"  sample {b}: live {int(g.live[b].sum())}  (c0, c1) {live_pairs[:12]}{' ...' if len(live_pairs) > 12 else ''}  "
              f"culled {int(g.culled[b].sum())}  empty un-culled {int(((g.count[b] == 0) & ~g.culled[b]).sum())}  "
              f"clearance {g.clearance[b]:.4f}  near the boundary {int(g.near[b])}  cull clearance {g.cull_clearance[b]:.2e}  node clearance {g.node_clearance[b]:.1e}")
    assert set(case.pins) <= pairs, (case.pins, sorted(pairs))
    assert g.live.any(axis=1).any()
    assert min(s.src[0] for s in case.samples) >= SE.BETA_MIN
    if case.interpolate:
        assert (g.near == 0).all(), g.near
        assert (g.near <= 0.005 * g.live.sum(axis=1)).all()
        assert (g.cull_clearance >= SE.CULL_MARGIN).all(), g.cull_clearance
    if "count" in case.roles:
        assert (g.clearance >= SE.MARGIN).all(), g.clearance
        assert (g.node_clearance >= SE.NODE_MARGIN).all(), g.node_clearance
    # cull soundness: in every culled tile every float64 pixel is outside the table
    assert not (g.culled & (g.count > 0)).any()
    if "cull" in case.roles:
        for b, s in enumerate(case.samples):
            if s.lens[0] > 0.1:   # the realistic lenses
                assert g.culled[b].any() and ((g.count[b] == 0) & ~g.culled[b]).any(), b


def test_compaction_set(geo):
    """Across the table-mode main-kernel cases the wave-tile counts hit every value at which the compaction takes another path,
    in the blocked and in the linear order."""
    for order, cases in (("blocked", [c for c in SE.CASES if SE.blocked(c)]),
                         ("linear", [c for c in SE.CASES if c.interpolate and not SE.blocked(c)]
                          + [SE.variant(c, "linear", GIGALENS_HIP_SHP_BLOCKED=0) for c in SE.CASES if "count" in c.roles and SE.blocked(c)])):
        pairs = set()
        for c in cases:
            if "count" in c.roles:
                pairs |= _pairs(geo(c))
        counts = {a + b for a, b in pairs}
        print(order, "counts", sorted(counts))
        assert {0, 1, 63, 64, 65, 128} <= counts, (order, sorted(counts))
        assert any(a == 0 and b > 0 for a, b in pairs), order            # every rank of slot 1 is offset by c0 = 0
        assert any(a > 0 and b == 0 for a, b in pairs), order
        assert any(a == 64 and 0 < b < 64 for a, b in pairs), order      # round 2 starts exactly at the slot boundary
        assert any(0 < a < 64 and a + b > 64 for a, b in pairs), order   # round 1 mixes both slots, round 2 is slot 1 alone
    # ragged: a live pixel in the last, partial tile
    for cid in ("shp_cnt30", "shp_cnt28"):
        c = SE.BY_ID[cid]
        assert geo(c).count[:, -4:].any(), cid
    # the pixel region: live pixels are masked out
    c = SE.BY_ID["shp_pixregion32"]
    whole = SE.geometry(replace(c, id=c.id + "_whole", pix_region=False))
    assert (whole.live.sum(axis=1) > geo(c).live.sum(axis=1)).any()


def test_cull_set(geo):
    """One sample per slope branch of shp_cull_setup -- gamma > 2 (rb2), gamma = 2 exactly, gamma < 2 (grow) -- and q close
    to 1 beside q ~ 0.6, each with a culled tile and an un-culled tile without a live pixel; for gamma > 2 a tile that only the
    rb2 radius keeps un-culled."""
    seen = set()
    for c in SE.CASES:
        if "cull" not in c.roles:
            continue
        g = geo(c)
        for b, s in enumerate(c.samples):
            if s.lens[0] <= 0.1:
                continue
            gam = float(np.float32(s.lens[1]))
            e = float(np.hypot(s.lens[2], s.lens[3]))
            q = (1 - e) / (1 + e)
            ok = g.culled[b].any() and ((g.count[b] == 0) & ~g.culled[b]).any()
            if not ok:
                continue
            seen.add("gamma>2" if gam > 2 else "gamma<2" if gam < 2 else "gamma=2")
            seen.add("q~1" if q > 0.95 else "q~0.6" if abs(q - 0.6) < 0.05 else "q other")
            if gam > 2 and g.rb2_decides[b]:
                seen.add("rb2 decides")
    assert {"gamma>2", "gamma=2", "gamma<2", "q~1", "q~0.6", "rb2 decides"} <= seen, seen


def test_fused_solve_cases(geo):
    """The fused linear-solve cases: o = Dl & 3 covers 1 and 3, Dl = 15 fills a tile row, 16 / 48 / 80 px are blocked with a
    ragged end, the compact source leaves most wave-tiles without a live pixel."""
    dl = {c.id: (c.n_max + 1) * (c.n_max + 2) // 2 for c in SE.LSTSQ_CASES}
    assert {d & 3 for d in dl.values()} >= {1, 3} and 15 in dl.values() and {3, 15, 21, 55} <= set(dl.values())
    sizes = {c.num_pix for c in SE.LSTSQ_CASES if SE.blocked(c, fused=True) and c.num_pix ** 2 % 512}
    assert {16, 48, 80} <= sizes
    g = geo(SE.BY_ID["shp_lsq_compact64"], fused=True)
    assert (g.count == 0).mean() > 0.8 and g.live.any(axis=1).all()


def test_fused_solve_cases_are_well_posed():
    """The solve is pinv(X^T X, rcond = 1e-6): an eigenvalue near 1e-6 of the largest is kept or cut depending on rounding, and
    the fitted image jumps with that decision.  Every case keeps its smallest eigenvalue (float64 oracle) above 1e-4 of the
    largest: float32 normal matrices move eigenvalues by ~1e-6 of the largest, which leaves them two decades above the cut."""
    import torch
    from oracle import ref_torch as ref
    from tests.test_gpu_lstsq import _observation
    for case in SE.LSTSQ_CASES:
        wl = SE.workload(case)
        x64 = {g: [{k: v.double() for k, v in d.items()} for d in lst] for g, lst in SE.params(case).items()}
        obs, err = _observation(wl)
        rs = ref.RefSimulator(wl.phys_model, wl.sim_config, case.batch, dtype=torch.float64)
        st = ref.lstsq_simulate(rs, x64, obs, err, return_stacked=True).numpy()
        X = (st / err[None, :, :, None]).reshape(case.batch, -1, st.shape[-1])
        ev = np.linalg.eigvalsh(np.swapaxes(X, 1, 2) @ X)
        print(f"{case.id}: {st.shape[-1]} channels, smallest / largest eigenvalue {ev[:, 0] / ev[:, -1]}")
        assert (ev[:, 0] >= 1e-4 * ev[:, -1]).all(), case.id


def test_expected_kernel_names_are_shipped():
    """Every gl_shp_kernel name the cases declare is one the dispatch matrix declares too (tests/dispatch_cases.py)."""
    from tests import dispatch_cases as DC
    declared = DC.declared_names()
    for c in SE.CASES + SE.ORDER_CASES:
        assert set(c.kernels) <= declared, c.id
