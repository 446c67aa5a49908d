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

The second half of the matrix, GENERIC_CASES, covers `launch_generic` (csrc/gl_launch_generic.hip.h): the interpreter
(`gl_main_kernel<MODE, T, SHAPELETS, FAM, BIG>`, every composition without a specialised kernel, shapelets above n_max = 10, the
basis stack of lstsq [IMG_BASIS = 4]) and the two cluster kernels (`gl_cluster_kernel`, `gl_clusterw_kernel`) of N x NFW + Sersic
models, whose forward modes run the interpreter.  A basis case declares the one IMG_BASIS name.

A plain module (no GPU, no torch at import): the models are built by `workload(case)` on demand."""
import re
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

MODES = ("IMG_FWD", "IMG_BWD", "LL_FWD", "LL_GRAD")
FAMILIES = ("gl_pair_kernel", "gl_shp_kernel", "gl_static_kernel")
ENV_KNOBS = ("GIGALENS_HIP_PAIR", "GIGALENS_HIP_TILE", "GIGALENS_HIP_TILE_GRAD", "GIGALENS_HIP_STATIC_VARIANT",
             "GIGALENS_HIP_SHP_BLOCKED")
BASIS_MODE = "IMG_BASIS"
GENERIC_FAMILIES = ("gl_main_kernel", "gl_cluster_kernel", "gl_clusterw_kernel")
# the knobs of the generic paths (a list of their own: the specialised cases may set ENV_KNOBS only)
GENERIC_ENV_KNOBS = ("GIGALENS_HIP_STATIC", "GIGALENS_HIP_CLUSTER", "GIGALENS_HIP_TILE")

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
    lenses: Tuple[str, ...]          # mass profiles: "EPL", "SIE", "Shear"; generic cases also "SIS", "NFW", "NFW_ELLIPSE",
                                     # "TNFW", "dPIS", "dPIE", "dPIEP"
    lens_light: Tuple[str, ...]      # "Sersic" (spherical) or "SersicEllipse"; generic cases also "CoreSersic"
    sources: Tuple[str, ...]         # "Sersic", "SersicEllipse" or "Shapelets"; generic cases also "CoreSersic"
    num_pix: int
    batch: int
    err: bool                        # the likelihood uses an error map (else sigma^2 = bg^2 + model / t)
    kernels: Tuple[str, ...]         # demangled instantiation per mode, MODES order; a basis case: the IMG_BASIS one only
    pix_region: bool = False         # a circular pixel region: the pixel-list path (`a.pix`) and the mask
    n_max: int = 6
    interpolate: bool = True
    env: Dict[str, str] = field(default_factory=dict)
    lstsq: bool = False              # every light built with use_lstsq=True (no amplitude parameters): the basis cases

    @property
    def basis(self) -> bool:
        return len(self.kernels) == 1


def short_name(demangled: str) -> str:
    """'void glk::gl_pair_kernel<...>(glk::MainArgs)' -> 'gl_pair_kernel<...>' (the spelling the cases use)."""
    m = re.match(r"^(?:void )?glk::(\w+<.*>)\(.*\)$", demangled)
    return m.group(1) if m else demangled


def family(name: str) -> Optional[str]:
    f = name.split("<", 1)[0]
    return f if f in FAMILIES else None


def generic_family(name: str) -> Optional[str]:
    f = name.split("<", 1)[0]
    return f if f in GENERIC_FAMILIES else None


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


# ==== the generic launcher (launch_generic) ==============================================================================
def main(m, t, shp_, fam, big=False):
    return f"gl_main_kernel<{m}, {t}, {str(shp_).lower()}, {fam}, {str(big).lower()}>"


def interp(shp_, fam, t, big=False):
    """The interpreter in modes 0-3: T = `t` in the forward modes (4 for cheap profiles -- no EPL, no shapelets, FAM 0 -- or with
    GIGALENS_HIP_TILE=4), T = 2 in the gradient modes.  FAM = the highest profile level of the model (0 basic, 1 dPIE family,
    2 NFW_ELLIPSE / TNFW / CoreSersic); BIG = shapelets above n_max = 10, always T = 2 and FAM 0."""
    return tuple(main(m, 2 if (big or m in (1, 3)) else t, shp_, fam, big) for m in range(4))


def basis(shp_, fam, big=False):
    """The basis stack of lstsq (IMG_BASIS): the interpreter at T = 2."""
    return (main(4, 2, shp_, fam, big),)


# gl_clusterw_kernel instantiations of launch_generic by size (0: <= 4 halos and <= 8 sources, 1: <= 12 sources, 2: else):
# (lens dealing, sources per wave, waves per SIMD)
_CW = {False: (("CwLensNfw<1>", 2, 4), ("CwLensNfw<2>", 3, 4), ("CwLensNfw<2>", 5, 3)),
       True: (("CwLensNfw<1>", 2, 4), ("CwLensNfw<2>", 3, 3), ("CwLensNfw<2>", 5, 2))}


def cluster(ell, small):
    """The pixel-split cluster kernel in the gradient modes (capacity 4 + 8 or 8 + 20); the forward modes run the interpreter at
    T = 4 (NFW + Sersic: cheap profiles)."""
    nh, ns, w = (4, 8, 3) if small else (8, 20, 2)
    e = str(ell).lower()
    return (main(0, 4, False, 0), f"gl_cluster_kernel<1, {nh}, {ns}, {e}, {w}>", main(2, 4, False, 0),
            f"gl_cluster_kernel<3, {nh}, {ns}, {e}, {w}>")


def clusterw(ell, size):
    lens, spw, w = _CW[ell][size]
    e = str(ell).lower()
    return (main(0, 4, False, 0), f"gl_clusterw_kernel<1, glk::{lens}, {spw}, {e}, {w}>", main(2, 4, False, 0),
            f"gl_clusterw_kernel<3, glk::{lens}, {spw}, {e}, {w}>")


def _genv(static=None, cluster_=None, tile=None):
    env = {}
    for k, v in zip(GENERIC_ENV_KNOBS, (static, cluster_, tile)):
        if v is not None:
            env[k] = str(v)
    return env


def _cl(n_halos, sources):
    """A cluster model: `n_halos` NFW halos, no lens light, the given Sersic / SersicEllipse sources."""
    return ("NFW",) * n_halos, (), tuple(sources)


def _srcs(n, n_ell):
    """n sources, the last n_ell of them elliptical (mixed lists: the spherical path pairs sources)"""
    return ("Sersic",) * (n - n_ell) + ("SersicEllipse",) * n_ell


GENERIC_CASES = []

# ---- the interpreter, modes 0-3: the six (SHAPELETS, FAM) pairs at T = 4 and T = 2 in the forward modes -------------------------
SISSH, DPIESH = ("SIS", "Shear"), ("dPIE", "Shear")
FAM2 = ("NFW_ELLIPSE", "TNFW", "dPIE", "SIS")  # kinds of all three levels under one FAM 2 kernel
GENERIC_CASES += [
    # natural compositions (default environment)
    Case("int_sisshear_s_se_t4", SISSH, S, SE, 32, 3, True, interp(False, 0, 4)),
    Case("int_sis_se_t4_pixregion", ("SIS",), (), SE, 30, 2, False, interp(False, 0, 4), pix_region=True),
    Case("int_eplnfw_s_t2", ("EPL", "NFW"), (), S, 37, 3, False, interp(False, 0, 2)),
    Case("int_eplshear_se_static0", ES, (), SE, 32, 3, True, interp(False, 0, 2), env=_genv(static=0)),
    Case("int_sisshear_shp_t2", SISSH, (), SHP_, 32, 3, True, interp(True, 0, 2), n_max=6),
    Case("int_dpieshear_s_t2", DPIESH, (), S, 33, 3, False, interp(False, 1, 2)),
    Case("int_dpieshear_s_t2_pixregion", DPIESH, (), SE, 32, 2, True, interp(False, 1, 2), pix_region=True),
    # (n_max = 5 on this grid gives one VJP element beyond GRAD_RTOL_COL, 3.4e-4: theta_E, whose pixel sum cancels 46-fold; the
    # float32 evaluation of the oracle itself is 3.1e-4 off there, and the grid-rounding bound does not model it)
    Case("int_dpie_shp_t2", ("dPIE",), (), SHP_, 32, 2, True, interp(True, 1, 2), n_max=6),
    Case("int_fam2_all_levels_t2", FAM2, ("CoreSersic",), ("Sersic", "SersicEllipse"), 36, 3, False, interp(False, 2, 2)),
    Case("int_fam2_shp_t2_batch1", ("TNFW", "SIS"), ("CoreSersic",), SHP_, 32, 1, True, interp(True, 2, 2), n_max=6),
    # GIGALENS_HIP_TILE=4 where no natural composition runs the forward modes at T = 4
    Case("int_sisshear_shp_t4_direct", SISSH, (), SHP_, 30, 2, False, interp(True, 0, 4), n_max=5, interpolate=False,
         env=_genv(tile=4)),
    Case("int_dpisdpiep_shear_s_se_t4", ("dPIS", "dPIEP", "Shear"), SE, S, 32, 3, True, interp(False, 1, 4), env=_genv(tile=4)),
    Case("int_dpie_s_shp_t4", ("dPIE",), S, SHP_, 30, 2, True, interp(True, 1, 4), n_max=6, env=_genv(tile=4)),
    Case("int_fam2_t4_pixregion", ("NFW_ELLIPSE", "TNFW"), (), ("CoreSersic", "Sersic"), 33, 3, True, interp(False, 2, 4),
         pix_region=True, env=_genv(tile=4)),
    Case("int_fam2_shp_t4_direct", ("NFW_ELLIPSE",), (), SHP_, 32, 2, False, interp(True, 2, 4), n_max=4, interpolate=False,
         env=_genv(tile=4)),
    # shapelets above n_max = 10: the runtime-order variant in every mode, whatever GIGALENS_HIP_TILE says
    Case("int_big_table_n12", ES, SE, SHP_, 32, 2, True, interp(True, 0, 2, big=True), n_max=12),
    Case("int_big_direct_n11_t4", ES, (), SHP_, 30, 2, False, interp(True, 0, 4, big=True), n_max=11, interpolate=False,
         env=_genv(tile=4)),
]

# ---- cluster models, modes 1 and 3: the 60 % fill rule of gl_model_create picks the component-per-wave kernel when n_lens + n_src
# >= 0.6 x the slots of its size (12, 20, 28); the cases sit on the capacity boundaries of both kernels ----------------------------
GENERIC_CASES += [
    # pixel-split, 4 + 8 capacity: 2 + 5 is below 60 % of 12 slots
    Case("cl_2h5s_sph", *_cl(2, _srcs(5, 0)), 33, 3, True, cluster(False, True)),
    Case("cl_2h5s_mixed_pixregion", *_cl(2, _srcs(5, 2)), 36, 2, False, cluster(True, True), pix_region=True),
    # pixel-split, 8 + 20 capacity: 5 + 6 and 6 + 5 are below 60 % of 20 slots; 8 + 20 full (GIGALENS_HIP_CLUSTER=1)
    Case("cl_6h5s_sph_batch1", *_cl(6, _srcs(5, 0)), 37, 1, False, cluster(False, False)),
    Case("cl_5h6s_mixed_pixregion", *_cl(5, _srcs(6, 3)), 33, 2, True, cluster(True, False), pix_region=True),
    Case("cl_8h20s_sph_forced", *_cl(8, _srcs(20, 0)), 32, 2, True, cluster(False, False), env=_genv(cluster_=1)),
    Case("cl_8h20s_ell_forced", *_cl(8, _srcs(20, 20)), 33, 2, False, cluster(True, False), env=_genv(cluster_=1)),
    # component-per-wave, size 0: 3 + 5 is above 60 % of 12; 4 + 8 full; 1 + 1 (GIGALENS_HIP_CLUSTER=2): mostly neutral slots
    Case("cl_3h5s_sph", *_cl(3, _srcs(5, 0)), 33, 3, False, clusterw(False, 0)),
    Case("cl_4h8s_mixed", *_cl(4, _srcs(8, 3)), 32, 2, True, clusterw(True, 0)),
    Case("cl_4h8s_sph_pixregion", *_cl(4, _srcs(8, 0)), 36, 2, True, clusterw(False, 0), pix_region=True),
    Case("cl_1h1s_ell_forced", *_cl(1, _srcs(1, 1)), 33, 2, True, clusterw(True, 0), env=_genv(cluster_=2)),
    # size 1: 5 + 8 and 4 + 9 (one past the small capacity), 8 + 12 (full)
    Case("cl_5h8s_sph", *_cl(5, _srcs(8, 0)), 37, 2, True, clusterw(False, 1)),
    Case("cl_4h9s_mixed", *_cl(4, _srcs(9, 4)), 33, 2, False, clusterw(True, 1)),
    Case("cl_8h12s_sph_batch1", *_cl(8, _srcs(12, 0)), 32, 1, False, clusterw(False, 1)),
    Case("cl_5h9s_mixed_pixregion", *_cl(5, _srcs(9, 5)), 37, 2, True, clusterw(True, 1), pix_region=True),
    Case("cl_8h11s_ell", *_cl(8, _srcs(11, 11)), 32, 2, True, clusterw(True, 1)),
    # size 2: 8 + 13 (one past size 1), 8 + 20 (full)
    Case("cl_8h13s_sph", *_cl(8, _srcs(13, 0)), 33, 2, True, clusterw(False, 2)),
    Case("cl_8h13s_mixed", *_cl(8, _srcs(13, 6)), 32, 2, False, clusterw(True, 2)),
    Case("cl_8h20s_sph", *_cl(8, _srcs(20, 0)), 37, 1, True, clusterw(False, 2)),
    Case("cl_8h20s_mixed_pixregion", *_cl(8, _srcs(20, 7)), 33, 2, True, clusterw(True, 2), pix_region=True),
]

# ---- the basis stack of lstsq (IMG_BASIS): every light a least-squares component -------------------------------------------------
GENERIC_CASES += [
    Case("basis_eplshear_se_s", ES, SE, ("Sersic", "Sersic"), 32, 3, True, basis(False, 0), lstsq=True),
    Case("basis_sis_s_pixregion", ("SIS",), (), S, 30, 2, True, basis(False, 0), lstsq=True, pix_region=True),
    Case("basis_dpieshear_s", DPIESH, (), S, 33, 3, True, basis(False, 1), lstsq=True),
    Case("basis_fam2_core_s", ("NFW_ELLIPSE", "TNFW"), ("CoreSersic",), S, 32, 2, True, basis(False, 2), lstsq=True),
    Case("basis_eplshear_shp_direct", ES, (), SHP_, 30, 2, True, basis(True, 0), lstsq=True, n_max=4, interpolate=False),
    Case("basis_eplshear_se_shp12", ES, SE, SHP_, 32, 2, True, basis(True, 0, big=True), lstsq=True, n_max=12),
    Case("basis_dpie_shp_pixregion", ("dPIE",), (), SHP_, 32, 2, True, basis(True, 1), lstsq=True, n_max=5, pix_region=True),
    Case("basis_tnfw_core_shp", ("TNFW",), ("CoreSersic",), SHP_, 32, 2, True, basis(True, 2), lstsq=True, n_max=6),
]


def declared_names():
    """Every kernel name the matrix declares (all families, the interpreter fallbacks and the generic cases included)."""
    return {k for c in CASES + GENERIC_CASES for k in c.kernels}


# ---- models ---------------------------------------------------------------------------------------------------------------
def workload(case: Case):
    """The case's Workload (gigalens_amd.workloads): physical model, prior, camera and batch.  Priors are the workloads' own
    (tests/conftest.py of the reference, shapelets-demo.ipynb); those of the generic cases come from the suites that first used
    the profiles (test_gpu_extra._model, test_gpu_dpie._mixed_cluster, test_cluster_kernel_matches_interpreter,
    test_gpu_lstsq._model, test_edge_compositions).  A least-squares case (`lstsq`) has no amplitude parameters."""
    import math

    import numpy as np

    from gigalens_amd import prior as tfd
    from gigalens_amd import workloads as W
    from gigalens_amd.model import PhysicalModel
    from gigalens_amd.profiles.light.sersic import CoreSersic, Sersic, SersicEllipse
    from gigalens_amd.profiles.light.shapelets import Shapelets
    from gigalens_amd.profiles.mass.epl import EPL
    from gigalens_amd.profiles.mass.nfw import NFW, NFW_ELLIPSE
    from gigalens_amd.profiles.mass.piemd import DPIE, DPIS
    from gigalens_amd.profiles.mass.piep import DPIEP
    from gigalens_amd.profiles.mass.shear import Shear
    from gigalens_amd.profiles.mass.sie import SIE as SIEProfile
    from gigalens_amd.profiles.mass.sis import SIS
    from gigalens_amd.profiles.mass.tnfw import TNFW
    from gigalens_amd.simulator import SimulatorConfig

    J = tfd.JointDistributionNamed
    LN, N, U = tfd.LogNormal, tfd.Normal, tfd.Uniform
    cluster_model = set(case.lenses) == {"NFW"} and not case.lens_light

    def amp(d, ie):
        """d with the amplitude Ie, unless the light is a least-squares component"""
        if not case.lstsq:
            d["Ie"] = ie
        return d

    def mass(name):
        if name == "EPL":
            return EPL(), W._epl_prior()
        if name == "SIE":
            return SIEProfile(), J(dict(theta_E=tfd.LogNormal(math.log(1.25), 0.25), e1=tfd.Normal(0, 0.1), e2=tfd.Normal(0, 0.1),
                                        center_x=tfd.Normal(0, 0.05), center_y=tfd.Normal(0, 0.05)))
        if name == "SIS":
            return SIS(), J(dict(theta_E=LN(math.log(0.5), 0.1), center_x=N(0, 0.02), center_y=N(0, 0.02)))
        if name == "NFW":
            return NFW(), J(dict(Rs=LN(math.log(2.0), 0.3), alpha_Rs=LN(math.log(0.5), 0.3), center_x=U(-1.5, 1.5),
                                 center_y=U(-1.5, 1.5)))
        if name == "NFW_ELLIPSE":
            return NFW_ELLIPSE(), J(dict(Rs=LN(math.log(1.5), 0.1), alpha_Rs=LN(math.log(0.9), 0.1), e1=N(0.15, 0.05),
                                         e2=N(-0.1, 0.05), center_x=N(0, 0.03), center_y=N(0, 0.03)))
        if name == "TNFW":
            return TNFW(), J(dict(Rs=LN(math.log(0.4), 0.1), alpha_Rs=LN(math.log(0.15), 0.1), r_trunc=LN(math.log(1.2), 0.2),
                                  center_x=N(0.6, 0.03), center_y=N(-0.4, 0.03)))
        if name == "dPIS":
            return DPIS(), J(dict(theta_E=LN(math.log(0.5), 0.1), r_core=LN(math.log(0.05), 0.2), r_cut=LN(math.log(1.5), 0.2),
                                  center_x=N(0.4, 0.05), center_y=N(-0.3, 0.05)))
        if name in ("dPIE", "dPIEP"):  # the dPIEP halo of _mixed_cluster; dPIE with (r_core, r_cut) in place of (Ra, Rs)
            radii = dict(r_core=LN(math.log(0.1), 0.2), r_cut=LN(math.log(4.0), 0.2)) if name == "dPIE" else \
                dict(Ra=LN(math.log(0.1), 0.2), Rs=LN(math.log(4.0), 0.2))
            return (DPIE() if name == "dPIE" else DPIEP()), J(dict(theta_E=LN(math.log(0.9), 0.1), **radii, center_x=N(0, 0.05),
                                                                 center_y=N(0, 0.05), e1=N(0.15, 0.05), e2=N(-0.1, 0.05)))
        assert name == "Shear", name
        return Shear(), W._shear_prior()

    def core_sersic():
        return CoreSersic(use_lstsq=case.lstsq), J(amp(dict(
            R_sersic=LN(math.log(0.25), 0.1), n_sersic=U(1, 3), Rb=LN(math.log(0.08), 0.2), alpha=U(1.0, 3.0),
            gamma=U(0.05, 0.5), e1=N(0, 0.1), e2=N(0, 0.1), center_x=N(0, 0.1), center_y=N(0, 0.1)), LN(math.log(60.0), 0.3)))

    def lens_light(name):
        if name == "CoreSersic":
            return core_sersic()
        d = amp(dict(R_sersic=tfd.LogNormal(math.log(1.0), 0.15), n_sersic=tfd.Uniform(2, 4), center_x=tfd.Normal(0, 0.05),
                     center_y=tfd.Normal(0, 0.05)), tfd.LogNormal(math.log(50.0), 0.3))
        if name == "Sersic":
            return Sersic(use_lstsq=case.lstsq), J(d)
        assert name == "SersicEllipse", name
        d.update(e1=tfd.TruncatedNormal(0, 0.1, -0.3, 0.3), e2=tfd.TruncatedNormal(0, 0.1, -0.3, 0.3))
        return SersicEllipse(use_lstsq=case.lstsq), J(d)

    def source(name):
        if name == "Shapelets":
            prof = Shapelets(case.n_max, use_lstsq=case.lstsq, interpolate=case.interpolate)
            d = dict(beta=tfd.LogNormal(math.log(0.1), 0.15), center_x=tfd.Normal(0, 0.01), center_y=tfd.Normal(0, 0.01))
            if not case.lstsq:
                d.update({nm: tfd.Normal(0, 500.0 / math.sqrt(i + 1)) for i, nm in enumerate(prof._amp_names)})
            return prof, J(d)
        if name == "CoreSersic":
            return core_sersic()
        if cluster_model:  # the sources of test_cluster_kernel_matches_interpreter, spread over the halos' field
            d = amp(dict(R_sersic=LN(math.log(0.25), 0.15), n_sersic=U(0.5, 4), center_x=U(-1, 1), center_y=U(-1, 1)),
                    LN(math.log(150.0), 0.5))
            if name == "Sersic":
                return Sersic(), J(d)
            assert name == "SersicEllipse", name
            d.update(e1=N(0, 0.15), e2=N(0, 0.15))
            return SersicEllipse(), J(d)
        if name == "Sersic":
            if case.lstsq:
                return Sersic(use_lstsq=True), J(dict(R_sersic=LN(math.log(0.25), 0.1), n_sersic=U(1, 3), center_x=N(0, 0.1),
                                                      center_y=N(0, 0.1)))
            return Sersic(), W._sersic_src_prior()
        assert name == "SersicEllipse", name
        d = amp(dict(R_sersic=tfd.LogNormal(math.log(0.25), 0.15), n_sersic=tfd.Uniform(0.5, 4), center_x=tfd.Normal(0, 0.25),
                     center_y=tfd.Normal(0, 0.25)), tfd.LogNormal(math.log(150.0), 0.5))
        d.update(e1=tfd.Normal(0, 0.15), e2=tfd.Normal(0, 0.15))
        return SersicEllipse(use_lstsq=case.lstsq), J(d)

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
    # NaN likelihood) at the workloads' bg = 0.2, t = 100, so the shapelet cases are given bg = 1.  So are the cluster cases without
    # an error map: in their faint field sigma^2 < 1/2pi at bg = 0.2, where the chi^2 and the log-normalisation of the
    # log-likelihood have opposite signs and can cancel
    bg = 1.0 if "Shapelets" in case.sources or (cluster_model and not case.err) else 0.2
    return W.Workload(case.id, phys, J(groups), cfg, case.batch, background_rms=bg, use_error_map=case.err)
