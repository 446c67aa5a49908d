"""The dispatch matrix of the compile-time-specialised main kernels: one case per model / grid / environment, with the kernel
each of the four modes must launch.

`launch_static` (csrc/gl_launch.hip.h) picks a pixel-pair kernel (`gl_pair_kernel`), a shapelet kernel (`gl_shp_kernel`) or a tile
kernel (`gl_static_kernel`) from the composition `match_static` (csrc/gl_launch_mode0.hip) found, whether every light is
spherical, the tile sizes, the static variant, whole or ragged 512-pixel tiles and table or direct shapelets.  Each case below
names the instantiation that serves it in simulate [IMG_FWD = 0], its VJP [IMG_BWD = 1], the log-likelihood [LL_FWD = 2] and the
fused forward + gradient [LL_GRAD = 3], in the demangled spelling of tests/test_kernel_resources.py::DISPATCHED.

tests/test_gpu_dispatch_matrix.py runs every case against the float64 oracle and checks the kernel names live;
tests/test_dispatch_matrix_host.py checks on the CPU that the three families in the shipped library are exactly the declared
names -- a new instantiation without a case fails there.

A plain module (no GPU, no torch at import): the models are built by `workload(case)` on demand."""
import re
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

MODES = ("IMG_FWD", "IMG_BWD", "LL_FWD", "LL_GRAD")
FAMILIES = ("gl_pair_kernel", "gl_shp_kernel", "gl_static_kernel")
ENV_KNOBS = ("GIGALENS_HIP_PAIR", "GIGALENS_HIP_TILE", "GIGALENS_HIP_TILE_GRAD", "GIGALENS_HIP_STATIC_VARIANT",
             "GIGALENS_HIP_SHP_BLOCKED")

V2 = "float __vector(2)"


def _kl(*kinds):
    return "glk::KindList<" + ", ".join(str(k) for k in kinds) + ">"


# component kinds (include/gigalens_hip.h): EPL 1, SIE 2, SHEAR 4, SERSIC 16, SERSIC_ELLIPSE 17, SHAPELETS 18
EPLSHEAR, SIE, SIESHEAR = _kl(1, 4), _kl(2), _kl(2, 4)
NONE, SER, SERE, SHP = _kl(), _kl(16), _kl(17), _kl(18)
LENS_KINDS = {("EPL", "Shear"): EPLSHEAR, ("SIE",): SIE, ("SIE", "Shear"): SIESHEAR}


@dataclass(frozen=True)
class Case:
    id: str
    lenses: Tuple[str, ...]          # mass profiles: "EPL", "SIE", "Shear"
    lens_light: Tuple[str, ...]      # "Sersic" (spherical) or "SersicEllipse"
    sources: Tuple[str, ...]         # "Sersic", "SersicEllipse" or "Shapelets"
    num_pix: int
    batch: int
    err: bool                        # the likelihood uses an error map (else sigma^2 = bg^2 + model / t)
    kernels: Tuple[str, str, str, str]  # demangled instantiation per mode, MODES order
    pix_region: bool = False         # a circular pixel region: the pixel-list path (`a.pix`) and the mask
    n_max: int = 6
    interpolate: bool = True
    env: Dict[str, str] = field(default_factory=dict)


def short_name(demangled: str) -> str:
    """'void glk::gl_pair_kernel<...>(glk::MainArgs)' -> 'gl_pair_kernel<...>' (the spelling the cases use)."""
    m = re.match(r"^(?:void )?glk::(\w+<.*>)\(.*\)$", demangled)
    return m.group(1) if m else demangled


def family(name: str) -> Optional[str]:
    f = name.split("<", 1)[0]
    return f if f in FAMILIES else None


# ---- expected names ---------------------------------------------------------------------------------------------------
def pair(lk, ck, sk, w_grad):
    """Pair kernels: a 4-waves-per-SIMD budget in the forward modes, `w_grad` (W1 = 3 or W2 = 2) in the gradient modes."""
    return tuple(f"gl_pair_kernel<{m}, {V2}, {4 if m in (0, 2) else w_grad}, {lk}, {ck}, {sk} >" for m in range(4))


def shp(ck, interp, ragged):
    """Shapelet kernels: EPL+Shear lenses, NPS = SH_SQ / 2 = 6 order pairs per lane, every mode."""
    return tuple(f"gl_shp_kernel<{m}, 2, {EPLSHEAR}, {ck}, 6, {str(interp).lower()}, {str(ragged).lower()}>" for m in range(4))


def static(lk, ck, sk, fwd, grad):
    """Tile kernels: `fwd` = (T, waves) of the forward modes, `grad` = (T, waves) of the gradient modes; None = the table falls
    back to the interpreter (shapelet compositions at T = 4), which runs the forward modes at T = 4 and the gradient modes at T = 2."""
    out = []
    for m in range(4):
        tw = fwd if m in (0, 2) else grad
        if tw is None:
            out.append(f"gl_main_kernel<{m}, {4 if m in (0, 2) else 2}, true, 0, false>")
        else:
            out.append(f"gl_static_kernel<{m}, {tw[0]}, {tw[1]}, {lk}, {ck}, {sk} >")
    return tuple(out)


def _env(pair_=None, tile=None, tile_grad=None, variant=None, blocked=None):
    env = {}
    for k, v in zip(ENV_KNOBS, (pair_, tile, tile_grad, variant, blocked)):
        if v is not None:
            env[k] = str(v)
    return env


ES, SIE_, SS = ("EPL", "Shear"), ("SIE",), ("SIE", "Shear")
S, SE = ("Sersic",), ("SersicEllipse",)

CASES = []

# ---- pair kernels (default environment): 4 compositions x {all spherical -> KindList<16>, elliptical -> KindList<17>} ----------
# waves per SIMD in the gradient modes as launch_static declares them: W1 = 3, W2 = 2
for tag, lenses, ll, w_sph, w_ell in (("eplshear_s", ES, False, 3, 3), ("eplshear_ss", ES, True, 2, 2),
                                      ("sie_s", SIE_, False, 3, 3), ("sieshear_ss", SS, True, 3, 2)):
    lk = LENS_KINDS[lenses]
    for light, ck_kind, w in ((S, SER, w_sph), (SE, SERE, w_ell)):
        ck = ck_kind if ll else NONE
        names = pair(lk, ck, ck_kind, w)
        sph = "sph" if light == S else "ell"
        # whole 512-pixel tiles with an error map; a ragged grid without one, odd batch
        CASES.append(Case(f"pair_{tag}_{sph}_whole_err", lenses, light if ll else (), light, 32, 4, True, names))
        CASES.append(Case(f"pair_{tag}_{sph}_ragged", lenses, light if ll else (), light, 37, 3, False, names))
# mixed lights: the elliptical kernel serves a spherical member
CASES += [
    Case("pair_eplshear_mixed_S_SE", ES, S, SE, 33, 5, False, pair(EPLSHEAR, SERE, SERE, 2)),
    Case("pair_sieshear_mixed_SE_S", SS, SE, S, 32, 3, True, pair(SIESHEAR, SERE, SERE, 2)),
    # the pixel-list path, one per lens family
    Case("pair_eplshear_pixregion", ES, (), SE, 28, 3, False, pair(EPLSHEAR, NONE, SERE, 3), pix_region=True),
    Case("pair_sie_pixregion", SIE_, (), S, 30, 2, True, pair(SIE, NONE, SER, 3), pix_region=True),
    Case("pair_sieshear_pixregion", SS, S, S, 32, 4, False, pair(SIESHEAR, SER, SER, 3), pix_region=True),
    # one sample
    Case("pair_sieshear_batch1", SS, SE, SE, 40, 1, True, pair(SIESHEAR, SERE, SERE, 2)),
]

# ---- shapelet kernels (default environment): lens light none / Sersic / SersicEllipse (both KindList<17>), table or direct,
# whole (32^2, 64^2) or ragged (28^2, 30^2) tiles, error map or not.  Whole table-mode images use 8 x 16 pixel blocks (blk_w).
SHP_ = ("Shapelets",)
CASES += [
    Case("shp_none_table_whole_err", ES, (), SHP_, 32, 4, True, shp(NONE, True, False), n_max=6),
    Case("shp_none_table_whole_unblocked", ES, (), SHP_, 32, 3, True, shp(NONE, True, False), n_max=10, env=_env(blocked=0)),
    Case("shp_none_table_ragged", ES, (), SHP_, 30, 3, False, shp(NONE, True, True), n_max=8),
    Case("shp_none_direct_whole", ES, (), SHP_, 32, 3, False, shp(NONE, False, False), interpolate=False, n_max=4),
    Case("shp_none_direct_ragged_err", ES, (), SHP_, 30, 2, True, shp(NONE, False, True), interpolate=False, n_max=10),
    Case("shp_sersic_table_whole_err", ES, S, SHP_, 32, 4, True, shp(SERE, True, False), n_max=6),
    Case("shp_sersic_table_whole64", ES, S, SHP_, 64, 2, False, shp(SERE, True, False), n_max=10),
    Case("shp_sersice_table_ragged", ES, SE, SHP_, 28, 3, False, shp(SERE, True, True), n_max=5),
    Case("shp_sersice_direct_whole", ES, SE, SHP_, 32, 3, False, shp(SERE, False, False), interpolate=False, n_max=8),
    Case("shp_sersic_direct_ragged_err", ES, S, SHP_, 30, 3, True, shp(SERE, False, True), interpolate=False, n_max=6),
    Case("shp_sersice_table_pixregion", ES, SE, SHP_, 32, 2, True, shp(SERE, True, True), n_max=6, pix_region=True),
]

# ---- tile kernels (GIGALENS_HIP_PAIR=0): T = GIGALENS_HIP_TILE in the forward modes, GIGALENS_HIP_TILE_GRAD in the gradient
# modes, waves per SIMD from the tables of launch_static (and GIGALENS_HIP_STATIC_VARIANT where they branch on it).  Lights are
# KindList<16> whatever their ellipticity (the tile kernels fold SersicEllipse into the Sersic code).
CASES += [
    Case("tile_eplshear_s_t4v2_g1", ES, (), SE, 30, 3, False, static(EPLSHEAR, NONE, SER, (4, 2), (1, 4)),
         env=_env(0, 4, 1, 2)),
    Case("tile_eplshear_s_t4v0_g4", ES, (), S, 32, 2, True, static(EPLSHEAR, NONE, SER, (4, 3), (4, 3)),
         env=_env(0, 4, 4, 0)),
    Case("tile_eplshear_s_t1_g4v2", ES, (), SE, 32, 3, False, static(EPLSHEAR, NONE, SER, (1, 4), (4, 2)),
         env=_env(0, 1, 4, 2)),
    Case("tile_eplshear_s_t2v3_g2v3", ES, (), S, 37, 3, True, static(EPLSHEAR, NONE, SER, (2, 3), (2, 3)),
         env=_env(0, 2, 2, 3)),
    Case("tile_eplshear_s_t2_g2", ES, (), SE, 28, 4, False, static(EPLSHEAR, NONE, SER, (2, 4), (2, 4)),
         env=_env(0, 2, 2)),
    Case("tile_eplshear_ss_t4_g2", ES, SE, SE, 30, 3, True, static(EPLSHEAR, SER, SER, (4, 2), (2, 4)), env=_env(0, 4, 2)),
    Case("tile_eplshear_ss_t1_g4", ES, S, S, 32, 2, False, static(EPLSHEAR, SER, SER, (2, 4), (4, 2)), env=_env(0, 1, 4)),
    Case("tile_sie_s_t4_g2", SIE_, (), SE, 30, 3, False, static(SIE, NONE, SER, (4, 4), (2, 4)), env=_env(0, 4, 2)),
    Case("tile_sie_s_t2_g4", SIE_, (), S, 32, 2, True, static(SIE, NONE, SER, (2, 4), (4, 4)), env=_env(0, 2, 4)),
    Case("tile_sieshear_ss_t4_g1", SS, SE, SE, 32, 3, True, static(SIESHEAR, SER, SER, (4, 4), (2, 4)), env=_env(0, 4, 1)),
    Case("tile_sieshear_ss_t1_g4", SS, S, SE, 30, 2, False, static(SIESHEAR, SER, SER, (2, 4), (4, 4)), env=_env(0, 1, 4)),
    Case("tile_shp_t2_g1", ES, (), SHP_, 32, 3, True, static(EPLSHEAR, NONE, SHP, (2, 2), (1, 2)), n_max=6, env=_env(0, 2, 1)),
    Case("tile_shp_t1_g2_direct", ES, (), SHP_, 30, 2, False, static(EPLSHEAR, NONE, SHP, (1, 2), (2, 2)), n_max=5,
         interpolate=False, env=_env(0, 1, 2)),
    Case("tile_shp_t4_g4_fallback_direct", ES, (), SHP_, 28, 2, True, static(EPLSHEAR, NONE, SHP, None, None), n_max=4,
         interpolate=False, env=_env(0, 4, 4)),
    Case("tile_sersic_shp_t2_g1_direct", ES, SE, SHP_, 32, 2, True, static(EPLSHEAR, SER, SHP, (2, 2), (1, 2)), n_max=6,
         interpolate=False, env=_env(0, 2, 1)),
    Case("tile_sersic_shp_t1_g2", ES, S, SHP_, 30, 3, False, static(EPLSHEAR, SER, SHP, (1, 2), (2, 2)), n_max=8,
         env=_env(0, 1, 2)),
    Case("tile_sersic_shp_t4_g4_fallback", ES, SE, SHP_, 30, 2, False, static(EPLSHEAR, SER, SHP, None, None), n_max=5,
         env=_env(0, 4, 4)),
]


def declared_names():
    """Every kernel name the matrix declares (all families, the interpreter fallbacks included)."""
    return {k for c in CASES for k in c.kernels}


# ---- models ---------------------------------------------------------------------------------------------------------------
def workload(case: Case):
    """The case's Workload (gigalens_amd.workloads): physical model, prior, camera and batch.  Priors are the workloads' own
    (tests/conftest.py of the reference, shapelets-demo.ipynb)."""
    import math

    import numpy as np

    from gigalens_amd import prior as tfd
    from gigalens_amd import workloads as W
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import Sersic, SersicEllipse
    from gigalens_amd.profiles.light.shapelets import Shapelets
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE as SIEProfile
    from gigalens_amd.simulator import SimulatorConfig

    J = tfd.JointDistributionNamed

    def mass(name):
        if name == "EPL":
            return EPL(), W._epl_prior()
        if name == "SIE":
            return SIEProfile(), J(dict(theta_E=tfd.LogNormal(math.log(1.25), 0.25), e1=tfd.Normal(0, 0.1), e2=tfd.Normal(0, 0.1),
                                        center_x=tfd.Normal(0, 0.05), center_y=tfd.Normal(0, 0.05)))
        assert name == "Shear", name
        return Shear(), W._shear_prior()

    def lens_light(name):
        d = dict(R_sersic=tfd.LogNormal(math.log(1.0), 0.15), n_sersic=tfd.Uniform(2, 4), center_x=tfd.Normal(0, 0.05),
                 center_y=tfd.Normal(0, 0.05), Ie=tfd.LogNormal(math.log(50.0), 0.3))
        if name == "Sersic":
            return Sersic(), J(d)
        assert name == "SersicEllipse", name
        d.update(e1=tfd.TruncatedNormal(0, 0.1, -0.3, 0.3), e2=tfd.TruncatedNormal(0, 0.1, -0.3, 0.3))
        return SersicEllipse(), J(d)

    def source(name):
        if name == "Shapelets":
            prof = Shapelets(case.n_max, interpolate=case.interpolate)
            d = dict(beta=tfd.LogNormal(math.log(0.1), 0.15), center_x=tfd.Normal(0, 0.01), center_y=tfd.Normal(0, 0.01))
            d.update({nm: tfd.Normal(0, 500.0 / math.sqrt(i + 1)) for i, nm in enumerate(prof._amp_names)})
            return prof, J(d)
        if name == "Sersic":
            return Sersic(), W._sersic_src_prior()
        assert name == "SersicEllipse", name
        d = dict(R_sersic=tfd.LogNormal(math.log(0.25), 0.15), n_sersic=tfd.Uniform(0.5, 4), center_x=tfd.Normal(0, 0.25),
                 center_y=tfd.Normal(0, 0.25), Ie=tfd.LogNormal(math.log(150.0), 0.5), e1=tfd.Normal(0, 0.15),
                 e2=tfd.Normal(0, 0.15))
        return SersicEllipse(), J(d)

    groups = {}
    profs = {}
    for key, names, fn in (("lens_mass", case.lenses, mass), ("lens_light", case.lens_light, lens_light),
                           ("source_light", case.sources, source)):
        made = [fn(n) for n in names]
        profs[key] = [p for p, _ in made]
        if made:
            groups[key] = tfd.JointDistributionSequential([d for _, d in made])
    phys = PhysicalModel(profs["lens_mass"], profs["lens_light"], profs["source_light"])
    region = None
    if case.pix_region:
        n = case.num_pix
        yy, xx = np.mgrid[:n, :n]
        c = (n - 1) / 2
        region = (((xx - c) ** 2 + (yy - c) ** 2) < (0.42 * n) ** 2).astype(np.float32)
    cfg = SimulatorConfig(delta_pix=0.065, num_pix=case.num_pix, pix_region=region)
    # shapelet images dip to about -4 here: without an error map, sigma^2 = bg^2 + model / t would come near zero or below it (a
    # NaN likelihood) at the workloads' bg = 0.2, t = 100, so the shapelet cases are given bg = 1
    bg = 1.0 if "Shapelets" in case.sources else 0.2
    return W.Workload(case.id, phys, J(groups), cfg, case.batch, background_rms=bg, use_error_map=case.err)
