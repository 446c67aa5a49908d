"""The float64 restatement of the flux-ratio likelihood (tests/flux_cases.py) and the host side of
``ForwardProbModel(centroids_fluxes=..., centroids_fluxes_errors=...)``, without a GPU: the restatement's autograd gradient against
central differences, the envelope property of the profiled amplitude, the scale invariance, the closed form of the SIS, unmeasured
images and flux-less families, the conditions every case must meet, and the validation of the constructor."""
import numpy as np
import pytest
import torch

from tests import flux_cases as FC
from tests import mp_positions_cases as PC
from tests import multilens_cases as MC

F64 = torch.float64


@pytest.mark.parametrize("name", ["mixed2", "single", "zoo_a"])
def test_autograd_gradient_equals_central_differences(name):
    c, ref, _ = FC.data(name)
    p0 = PC.GC.pack_np(c["phys"], c["params"]).numpy()
    g, h, worst = ref["grad"], 1e-6, 0.0
    for k in range(p0.shape[1]):
        up, dn = p0.copy(), p0.copy()
        up[:, k] += h
        dn[:, k] -= h
        fd = (FC.loglike_grad(c, F64, up)[0] - FC.loglike_grad(c, F64, dn)[0]) / (2 * h)
        worst = max(worst, float(np.abs(fd - g[:, k]).max() / max(np.abs(g[:, k]).max(), 1e-300)))
    print(f"{name}: autograd vs central differences {worst:.3e} of the column scale")
    assert worst <= 1e-5


@pytest.mark.parametrize("name", FC.GRAD_CASES + ("one_nan",))
def test_envelope_property(name):
    """``S_f`` minimises ``chi2_f``: the gradient at fixed ``S_f`` is the total gradient."""
    c, ref, _ = FC.data(name)
    g_fixed = FC.loglike_grad(c, F64, detach_amplitude=True)[2]
    err = np.abs(g_fixed - ref["grad"]).max() / np.abs(ref["grad"]).max()
    print(f"{name}: gradient at fixed S_f vs total {err:.3e}")
    assert np.abs(ref["grad"]).max() > 0 and err <= 1e-10


def test_scale_invariance():
    """``F, s -> c F, c s`` per family: ``chi2`` and the gradient stay, ``S_f`` scales by ``c``, ``log_like`` shifts by ``-n_f log c``."""
    c, ref, _ = FC.data("mixed2")
    cs = (7.0, 0.25)  # (powers of two would hide nothing here, but 7 rounds: the fluxes go in as float64)
    fams = [dict(fm, flux=fm["flux"].astype(np.float64) * k, flux_err=fm["flux_err"].astype(np.float64) * k) for fm, k in zip(c["fams"], cs)]
    ll, chi2, g, S, model, _ = FC.loglike_grad(c, F64, fams=fams)
    assert np.abs(chi2 - ref["chi2"]).max() <= 1e-12 * np.abs(ref["chi2"]).max()
    assert np.abs(g - ref["grad"]).max() <= 1e-12 * np.abs(ref["grad"]).max()
    assert np.abs(S / ref["S"] - np.asarray(cs)[None, :]).max() <= 1e-13
    shift = -sum(fm["flux"].size * np.log(k) for fm, k in zip(c["fams"], cs))
    assert np.abs(ll - ref["log_like"] - shift).max() <= 1e-11 * np.abs(ref["log_like"]).max()


def test_sis_closed_form():
    """A source at ``beta < theta_E`` on the axis of an SIS: images at ``beta +- theta_E`` with ``|mu| = theta_E / beta +- 1``.  Fluxes
    ``S |mu|`` give ``chi2 = 0`` to rounding and return ``S``."""
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.mass.sis import SIS
    tE, beta, S = np.asarray([1.0, 1.3, 0.8]), np.asarray([0.3, 0.5, 0.2]), 4.5
    phys, mp = PhysicalModel([SIS()], [], []), MC._mp([0.5])
    lp = [{"theta_E": torch.as_tensor(tE), "center_x": torch.zeros(3, dtype=F64), "center_y": torch.zeros(3, dtype=F64)}]
    for b in range(3):  # (one sample's images at a time: trace takes the same points for every sample)
        x = torch.as_tensor([[beta[b] + tE[b]], [beta[b] - tE[b]]], dtype=F64).repeat(1, 3)
        y = torch.zeros_like(x)
        _, _, A, _ = PC.trace(phys, mp, lp, x, y, np.ones(1))
        det = (A[0] * A[3] - A[1] * A[2]).detach()
        mu = np.asarray([tE[b] / beta[b] + 1.0, tE[b] / beta[b] - 1.0])
        assert det[0, b] > 0 > det[1, b]
        assert np.abs(1.0 / det[:, b].abs().numpy() - mu).max() <= 1e-12 * mu.max()
        flux = S * mu
        ll, chi2, S_f, model = FC.family_term(det, flux, 0.03 * flux)
        print(f"SIS sample {b}: chi2 {float(chi2[b]):.3e}, S {float(S_f[b]):.15f}")
        assert float(chi2[b]) <= 1e-20 and abs(float(S_f[b]) - S) <= 1e-13 * S
        assert np.abs(model[:, b].numpy() - flux).max() <= 1e-13 * flux.max()
        assert float(ll[b]) == pytest.approx(-0.5 * np.log(2 * np.pi * (0.03 * flux) ** 2).sum(), rel=1e-13)


def test_unmeasured_image_and_fluxless_family():
    """A NaN flux is that image removed from the sums; a family without fluxes contributes exactly 0."""
    c, ref, _ = FC.data("one_nan")
    full = FC.case("mixed2")
    assert np.isnan(c["fams"][1]["flux"][2]) and FC.n_flux(c) == FC.n_flux(full) - 1 == 7
    det = torch.as_tensor(ref["det"])
    ll = chi2 = 0.0
    for fm, rows in zip(c["fams"], (slice(0, 3), slice(3, 8))):
        keep = ~np.isnan(fm["flux"])
        t = FC.family_term(det[rows][torch.as_tensor(keep)], fm["flux"][keep], fm["flux_err"][keep])
        ll, chi2 = ll + t[0].numpy(), chi2 + t[1].numpy()
    assert np.array_equal(ll, ref["log_like"]) and np.array_equal(chi2, ref["chi2"])
    assert np.isfinite(ref["model"]).all()  # (the unmeasured image still has its model flux S_f m_j)
    # a flux-less family: exactly 0, NaN amplitude -- and the sum over the families is the other family's term alone
    c, ref, _ = FC.data("partial")
    assert c["fams"][1]["flux"] is None and FC.n_flux(c) == 2
    z = FC.family_term(det[3:8], None, None)
    assert (z[0] == 0).all() and (z[1] == 0).all() and torch.isnan(z[2]).all()
    z = FC.family_term(det[3:8], np.full(5, np.nan), np.full(5, np.nan))
    assert (z[0] == 0).all() and (z[1] == 0).all() and torch.isnan(z[2]).all()
    near = FC.family_term(det[0:3], c["fams"][0]["flux"], c["fams"][0]["flux_err"])
    assert np.array_equal(near[0].numpy(), ref["log_like"]) and np.array_equal(near[1].numpy(), ref["chi2"])
    assert np.isnan(ref["S"][:, 1]).all() and np.isnan(ref["model"][:, 3:]).all() and np.isfinite(ref["model"][:, :3]).all()
    # the SIE on the second plane meets the rays of the flux-less far family alone: exact zeros in its columns (8..12)
    assert (ref["grad"][:, 8:] == 0).all() and (np.abs(ref["grad"][:, :8]).max(axis=0) > 0).all()


@pytest.mark.parametrize("name", FC.CASES)
def test_conditions_hold(name):
    c, ref, yard = FC.data(name)
    min_det, min_r = PC.conditions(c)
    print(f"{name}: min |det A| {min_det:.3f}, nearest lens centre {min_r:.1f} px, n_flux {FC.n_flux(c)}; float32 yardstick log_like "
          f"{yard['log_like']:.2e}, chi2 {yard['chi2']:.2e}, S {yard['S']:.2e}, model flux {yard['model']:.2e}, gradient "
          f"{yard['grad']:.2e} of the gate")
    assert min_det >= PC.MIN_DET and min_r >= PC.MIN_PIX
    assert np.isfinite(ref["grad"]).all() and yard["grad"] <= 0.25
    if name in FC.MIXED_CASES + FC.VARIANTS:  # both parities, in every sample
        assert (ref["det"] <= -PC.MIN_DET).all(axis=1).sum() >= 2 and (ref["det"] >= PC.MIN_DET).all(axis=1).sum() >= 2
    else:
        assert (ref["det"] > 0).all()
    J = sum(fm["x"].size for fm in c["fams"])
    assert 6 <= J <= 9 and len(c["fams"]) in (2, 3)
    if name == "single":
        assert len(set(c["scales"])) == 2 and all(0 < s < 1 for s in c["scales"]) and c["mp"].K == 1
    if name == "plain":
        assert c["scales"] is None and all(np.array_equal(fm["T"], np.ones(1)) for fm in c["fams"])
    # sample 0 misses its fluxes by the pattern alone
    fm = c["fams"][0]
    assert np.allclose(fm["flux_err"][~np.isnan(fm["flux"])], 0.05 * fm["flux"][~np.isnan(fm["flux"])], rtol=1e-6)


# ---- ForwardProbModel(centroids_fluxes=..., centroids_fluxes_errors=...) ---------------------------------------------
def _prob_model(c, **kw):
    from gigalens_amd import prior as tfd
    from gigalens_amd.model import ForwardProbModel
    J, S = tfd.JointDistributionNamed, tfd.JointDistributionSequential
    prior = J(dict(lens_mass=S([J({k: tfd.Normal(float(v[0]), 0.01) for k, v in d.items()}) for d in c["params"]["lens_mass"]])))
    args = dict(FC.centroids(c), include_pixels=False)
    args.update(kw)
    return ForwardProbModel(prior, **args)


def test_constructor_takes_fluxes_and_validates_them():
    c = FC.case("mixed2")
    pm = _prob_model(c)
    assert pm.n_flux == 8.0 and pm.n_position == 16.0
    for got, fm in zip(pm.centroids_fluxes, c["fams"]):
        assert got.dtype == np.float32 and np.array_equal(got, fm["flux"])
    F = [fm["flux"] for fm in c["fams"]]
    s = [fm["flux_err"] for fm in c["fams"]]
    # errors broadcast as the position errors do
    b = _prob_model(c, centroids_fluxes_errors=[np.float32(0.1), s[1]])
    assert np.array_equal(b.centroids_fluxes_errors[0], np.full(3, 0.1, np.float32)) and b.n_flux == 8.0
    # None or all NaN: a family without fluxes; unmeasured images do not count (and their errors are not looked at)
    assert _prob_model(c, centroids_fluxes=[None, F[1]], centroids_fluxes_errors=[None, s[1]]).n_flux == 5.0
    assert _prob_model(c, centroids_fluxes=[np.full(3, np.nan), F[1]]).n_flux == 5.0
    assert _prob_model(c, centroids_fluxes=[None, None], centroids_fluxes_errors=[None, None]).n_flux == 0.0
    one = FC.case("one_nan")
    assert _prob_model(one).n_flux == 7.0
    plain = _prob_model(c, centroids_fluxes=None, centroids_fluxes_errors=None)
    assert plain.n_flux == 0.0 and plain.centroids_fluxes is None

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            _prob_model(c, **kw)
    bad("give both or neither", centroids_fluxes_errors=None)
    bad("give both or neither", centroids_fluxes=None)
    bad("one entry per image family", centroids_fluxes=F[:1])
    bad("without centroids_fluxes_errors", centroids_fluxes_errors=[None, s[1]])
    bad("shape", centroids_fluxes=[F[0][:2], F[1]])
    bad("broadcast", centroids_fluxes_errors=[s[0][:2], s[1]])
    lone = F[0].copy()
    lone[1:] = np.nan
    bad("one measured flux", centroids_fluxes=[lone, F[1]])
    inf = F[1].copy()
    inf[0] = np.inf
    bad("must be finite", centroids_fluxes=[F[0], inf])
    for v, match in ((np.nan, "must be finite"), (np.inf, "must be finite"), (0.0, "> 0"), (-0.1, "> 0")):
        e = s[1].copy()
        e[3] = v
        bad(match, centroids_fluxes_errors=[s[0], e])
    from gigalens_amd.model import ForwardProbModel
    with pytest.raises(ValueError, match="centroids_x"):  # fluxes without centroids
        ForwardProbModel(pm.prior, np.zeros((4, 4), np.float32), 0.1, 100.0, include_positions=False, centroids_fluxes=F,
                         centroids_fluxes_errors=s)
    with pytest.raises(ValueError, match="centroids_fluxes"):
        plain.stats_fluxes(None, None)
    with pytest.raises(ValueError, match="centroids_fluxes"):
        plain.predicted_fluxes(None, None)


def test_event_size_counts_the_fluxes():
    import types

    from gigalens_amd.inference import ModellingSequence
    c = FC.case("mixed2")
    pm = _prob_model(c)
    ms = ModellingSequence(c["phys"], pm, None)
    sim = types.SimpleNamespace(img_region=torch.ones(4, 4, dtype=torch.bool))
    assert ms._event_size(sim) == 16.0 + 8.0
    ms.prob_model = _prob_model(c, centroids_fluxes=None, centroids_fluxes_errors=None)
    assert ms._event_size(sim) == 16.0


def test_the_new_kernel_has_no_spill_and_no_private_segment():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_flops as isa
    if not os.path.exists(isa.LIB):
        pytest.skip("library not built")
    md = isa.kernel_metadata(isa.code_object())
    hits = [k for k in md if "gl_pos_flux_kernel" in k]
    assert len(hits) == 1, hits
    m = md[hits[0]]
    print(f"gl_pos_flux_kernel: {m['vgpr_count']} VGPRs, {m['sgpr_count']} SGPRs, {m['lds_bytes']} B LDS, {m['scratch_bytes']} B private")
    assert m["vgpr_spill_count"] == 0 and m["scratch_bytes"] == 0 and m["lds_bytes"] == 0
