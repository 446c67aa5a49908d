// gl_model.h -- the library-internal model descriptor, the owner type of its device buffers (DevBuf) and the error helper shared
// by the translation units of libgigalens_hip.so (gigalens_hip.hip: models, launch plan, front end / finalize / PSF launchers, the
// render, likelihood and log-prob entries; gl_api_points.hip, gl_api_lstsq.hip, gl_api_pixsrc.hip, gl_api_ptimg.hip, gl_api_plugin.hip: the entry
// points of one feature family each, sharing gl_host.hip.h; gl_launch_mode*.hip / gl_generic_noslp_mode*.hip: one instantiation of
// a main-kernel launcher per mode; gl_user.hip: the run-time compiler of user-written profiles -- all compiled in parallel).  The
// model owns every device allocation it holds: destroying it frees them.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gigalens_hip.h"
#include "gl_kernels.hip.h"

namespace glk {
// sets the thread-local message gl_last_error() returns; returns `code`
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);
}  // namespace glk

#define GL_HIP(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) return glk::fail(GL_ELAUNCH, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

using glk::CompDesc;
using glk::CatDev;
using glk::SeriesDev;
using glk::InterpDev;
using glk::InterpMassDev;
using glk::ZCol;

namespace glk {
// One device allocation with an owner: freed with it, replaced as a whole by alloc() / upload().  Reads as the raw pointer, so
// kernel arguments and argument structs take it as they would a T*.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p_, o.p_);
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  // a fresh allocation of n elements (the old one is freed first)
  hipError_t alloc(size_t n) {
    reset();
    return hipMalloc((void**)&p_, sizeof(T) * n);
  }
  // overwrites the first n elements of the allocation in place
  hipError_t write(const T* src, size_t n, hipMemcpyKind kind = hipMemcpyHostToDevice) {
    return hipMemcpy(p_, src, sizeof(T) * n, kind);
  }
  // replaces the contents: a fresh allocation holding src[0..n)
  hipError_t upload(const T* src, size_t n) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : write(src, n);
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// plans of gl_corr_pair_kernel (gl_post.hip.h)
struct CorrClass {  // one ROW class; its column classes (ncj of them) are computed by the same thread
  int koff;        // offset of this class's [KH][ncj][KWP] kernel block in the kernel buffer
  int KH, pt, pl;  // taps per column, top / left padding of the window (common to the column classes: kernels are shifted)
  int Ho, Wo[4];   // outputs of the class (rows; columns per column class)
  int oo_r, oo_c[4];  // placement of output (0, 0) in the output image
};
struct CorrArgs {
  const float* k;
  int n_class, ncj, B;  // row classes (one per workgroup along z), column classes per thread
  int Hi, Wi;          // input image
  int Hout, Wout, os;  // output image and the placement stride of a class's outputs
  float scale;
  int vec;  // image widths multiples of four and 16-byte aligned buffers: float4 tile fill and output stores
  int dbg;  // -DGL_EXPERIMENTS builds only (GIGALENS_HIP_DBGFLAGS): 16 skip the tile fill, 32 skip the multiply-add loop, 64 skip the output stores
  CorrClass cls[16];
};
}  // namespace glk

struct gl_model {
  std::vector<CompDesc> comps;
  int n_lens = 0, n_ll = 0, n_src = 0;
  int P = 0, D = 0, A = 0, Apad = 0, ncols = 64;
  bool has_shapelets = false, has_table = false;
  bool shp_big = false;  // some shapelet component has n_max > SH_CAP: wide table, runtime-order interpreter variant for all of them
  // user-written profiles inside the model (K_USER_MASS / K_USER_LIGHT): the interpreter kernel compiled at run time with their bodies
  bool has_user = false;
  hipModule_t user_module = nullptr;
  hipFunction_t user_fn[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // per Mode (IMG_BASIS: none)
  // ... and, for the compositions the pair kernel serves (EPL / SIE / Shear / SIS / user lenses | Sersic / user lights), that kernel
  // specialised on the model's component list with the user bodies inside (gl_pair_kernel<MODE, v2f, 2, KindList<...>, ...>)
  hipFunction_t user_pair_fn[4] = {nullptr, nullptr, nullptr, nullptr};
  // ... and the point kernels (gl_positions.hip.h: image-position likelihood P1-P4, lens maps; gl_images.hip.h: map and Newton
  // kernels of the lens-equation solver) with the bodies on nested duals, compiled from user_point_src when first asked for
  // (gl_user.hip compile_user_points)
  std::string user_point_src;
  hipModule_t user_point_module = nullptr;
  hipFunction_t user_point_fn[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int height = 0, width = 0, supersample = 1, N = 0;
  float conversion_factor = 1.f;
  // device-resident, immutable (every glk::DevBuf below: owned by the model)
  glk::DevBuf<CompDesc> d_comps;
  glk::DevBuf<float> d_gx;
  glk::DevBuf<float> d_gy;
  glk::DevBuf<int> d_pix;
  glk::DevBuf<float> d_shp_tab;
  glk::DevBuf<float> d_nfw_tab;  // models with NFW lenses: h(X) = g(X) / X^2 on the float format's own grid (gl_host_tables.h)
  int chunk_px_override = 0;  // -DGL_EXPERIMENTS builds only
  int dbg_flags = 0;          // -DGL_EXPERIMENTS builds only
  float grid_rmax = 0.f;      // max |(x, y)| over the pixel grid
  int shp_blocked = 1;        // GIGALENS_HIP_SHP_BLOCKED: wave-tiles of the table-mode shapelet kernel are 8 x 16 blocks of the image
  int shp_cull = 1;           // GIGALENS_HIP_SHP_CULL: wave-tiles provably outside the shapelet table skip the lens (gl_shp.hip.h)
  int corr_max_pairs = 0;     // GIGALENS_HIP_CORR_MAXPAIRS, read once at gl_model_create
  int corr_wide = 1;          // GIGALENS_HIP_CORR_WIDE, read once at gl_model_create
  int careful_tiles = 0;      // GIGALENS_HIP_CAREFUL_TILES, read once at gl_model_create (MainArgs::careful_tiles)
  bool has_nfw = false;
  size_t nfw_lds = 0;          // bytes of that table in a main kernel's LDS
  int shp_stride = 0;
  glk::DevBuf<float> d_psf;  // effective kernel flip(psf) (*) box(ss)/ss^2, see gl_post.hip.h
  // the register-blocked pair kernel's plans (gl_post.hip.h gl_corr_pair_kernel): class tables, padded kernels on the device
  struct CorrPlan { glk::CorrArgs args{}; int KWP = 0, ST = 0, max_Ho = 0, max_Wo = 0, max_KH = 0; bool ok = false; };
  CorrPlan corr_fwd, corr_bwd;
  glk::DevBuf<float> d_corr_k;
  int psf_h = 0, psf_w = 0;
  // the PSF as given (not flipped, not pooled; [[1]] without one) with a two-node zero apron, [(psf_h + 4)][(psf_w + 4)]: the table
  // the point-image kernels interpolate (gl_ptimg.hip.h)
  glk::DevBuf<float> d_ptimg_tab;
  int KH = 1, KW = 1, pad_t = 0, pad_l = 0;
  bool has_post = false;
  // unconstrained-space front end (gl_model_set_prior)
  int d_z = 0;
  glk::DevBuf<ZCol> d_zcols;
  glk::DevBuf<int> d_src;
  glk::DevBuf<float> d_const;
  int static_id = 0;   // 0 = generic interpreter kernel, >0 = compile-time-specialised composition
  int static_matched = 0;  // ... as matched at creation: static_id is 0 while the sources carry deflection scales (src_scaled)
  int static_variant = 0;
  int pair = 1;        // pixel-pair (packed fp32) form of the specialised kernels
  bool light_spherical = false;  // every light profile is the spherical Sersic: the pair kernels take their fast path
  int cluster_w = 0;   // ... in its component-per-wave form (gl_clusterw_kernel)
  int cluster = 0;     // gl_cluster_kernel serves the gradient modes: 1 = halos + spherical Sersic sources, 2 = elliptical sources
  // image-position likelihood (gl_model_set_positions)
  int pos_J = 0, pos_F = 0, lens_params = 0;
  glk::DevBuf<float> d_pos;  // [4][J]: x, y, err_x, err_y
  glk::DevBuf<int> d_fam;    // [F+1]
  std::vector<int> pos_fam_off;  // ... on the host
  // per-source / per-family deflection scales c = [D_LS/D_S](z_source) / [D_LS/D_S](z_ref): sources and image families at their own
  // redshifts behind one lens plane (gl_model_set_source_scales, gl_model_set_position_scales).  Empty buffers: every scale is 1 and
  // every kernel runs as it did before the scales existed.
  bool src_scaled = false;             // some source light has a scale != 1
  glk::DevBuf<float> d_src_scale;      // [n_src], allocated only while src_scaled
  bool pos_scaled = false;             // some image family has a scale != 1
  glk::DevBuf<float> d_pos_scale;      // [J]: the scale of every image's family, allocated only while pos_scaled
  // lens planes at redshifts of their own (gl_model_set_lens_planes, gl_multiplane.hip.h).  mp_K = 0: one plane, and every entry
  // point runs as it did before the planes existed; mp_K >= 2: the multi-plane entries serve the model, the single-plane ones refuse
  int mp_K = 0;
  glk::DevBuf<int> d_mp_lens;     // [2][n_lens]: the lenses sorted by plane, the plane of every lens
  glk::DevBuf<float> d_mp_scale;  // [4][4] plane couplings, then [4][n_src] source couplings (zero-padded rows)
  // image families behind lens planes (gl_model_set_position_targets): the couplings T_f of every image's family
  bool pos_targets = false;
  glk::DevBuf<float> d_pos_target;  // [J][4], zero-padded rows; allocated only while pos_targets
  std::vector<float> pos_target_rows;  // [F][mp_K] on the host: the rows as given (empty without targets)
  // measured arrival times of the images on lens planes (gl_model_set_position_plane_delays, gl_multiplane_tdelays.hip.h); a state
  // of its own, apart from the single-plane one below.  Cleared by gl_model_set_positions, gl_model_set_lens_planes and
  // gl_model_set_position_targets
  int mpd_n_delay = 0;              // measured times over all families; 0: the model holds none, and its workspace is as without
  glk::DevBuf<float> d_mpd_delay;   // [2][J] time (NaN = not measured), error, then [F] lambda_f (NaN = profiled); only while mpd_n_delay
  glk::DevBuf<double> d_mpd_weight;  // [J][4] g_f of every image's family, zero-padded, then [4] v_i; only while mpd_n_delay
  void clear_plane_delays() {
    mpd_n_delay = 0;
    d_mpd_delay.reset();
    d_mpd_weight.reset();
  }
  // measured fluxes of the images (gl_model_set_position_fluxes, gl_fluxes.hip.h): the flux-ratio term of the point-image likelihood
  int pos_n_flux = 0;              // measured fluxes over all families; 0: the model holds none and every call runs as without them
  glk::DevBuf<float> d_pos_flux;   // [2][J]: flux (NaN = not measured), flux error; allocated only while pos_n_flux
  // measured arrival times of the images (gl_model_set_position_delays, gl_tdelays.hip.h): the time-delay term of the same likelihood
  int pos_n_delay = 0;             // measured times over all families; 0: the model holds none and every call runs as without them
  glk::DevBuf<float> d_pos_delay;  // [2][J] time (NaN = not measured), error, then [F] lambda_f (NaN = profiled); only while pos_n_delay
  std::vector<char> pos_fam_delay;   // [F] on the host: the family has measured times (empty without delays)
  std::vector<float> pos_fam_scale;  // [F] on the host: the scales of gl_model_set_position_scales (empty: all 1)
  bool has_epl = false;
  int epl_comp = -1;     // the model's only EPL component, or -1 (none / several)
  int fam = 0;  // family level of the interpreter variant (gl_main_kernel FAM): 1 dPIE family / catalogues / series, 2 gl_extra.h
  bool use_order = true;
  int tail_rows = -1, tail_n = -1;  // tapered end of the cost-ordered dispatch (tail_plan); rows 0 = off, -1 = automatic
  bool prep_lds = true;     // gl_prep_wave_kernel keeps each sample's parameter row in LDS
  bool order_fused = true;  // the front end's extra workgroup sorts (gl_prep_wave_kernel); else a launch of gl_order_kernel
  bool wave_prep = true;  // EPL models: one wavefront per sample in the front end (GIGALENS_HIP_WAVE_PREP=0: thread per component)
  int lstsq_wgs = 2048;     // workgroups the normal-matrix kernels of the linear solve aim for (pixel chunks per sample = this / B)
  bool lstsq_chol = true;   // linear solve: Cholesky attempt first (gl_chol_solve_kernel), eigenvalue solve for what it leaves
  bool lstsq_fused = true;  // one-shapelet-source linear solves form the normal matrix from the bases (gl_shp_normal_kernel), no stack
  // measurement hooks (gl_model_set_timing): a ring of event pairs around the main-kernel launches, and the host
  // function of the most recent main launch (gl_model_last_main_kernel)
  int timing_slots = 0, timing_stride = 1;
  // (atomics: two host threads may drive one model on different streams; each timed launch claims its ring slot)
  mutable std::atomic<long long> timing_count{0}, timing_calls{0};
  std::vector<hipEvent_t> evs;  // 2 * timing_slots
  mutable std::atomic<const void*> last_main_fn{nullptr};
  mutable std::atomic<const void*> last_post_fn[2] = {{nullptr}, {nullptr}};  // ... of the most recent forward / transposed PSF + pooling launch
  mutable std::atomic<int> last_main_user{-1};  // mode of the run-time compiled kernel the most recent main launch dispatched, or -1
  // galaxy catalogues of the GL_SCALED components (gl_model_set_catalogue)
  struct Cat { CatDev dev; std::vector<float> table; };
  std::vector<Cat> cats;
  int G = 0;           // galaxies over all catalogues
  int n_scaled = 0;    // GL_SCALED components
  glk::DevBuf<CatDev> d_cats;
  glk::DevBuf<float> d_gal_table;   // [G][7]
  glk::DevBuf<float> d_gal_static;  // [G][DP_NS]
  // series-expansion lenses (gl_model_set_series): one coefficient field per GL_SERIES component
  std::vector<SeriesDev> series;      // what the kernels read (d_series is its copy on the device): pointers into series_buf
  struct SeriesBuf { glk::DevBuf<float> coef, hcoef; };
  std::vector<SeriesBuf> series_buf;  // the owners of each slot's two fields
  std::vector<int> series_comp;       // component of each slot
  int n_series = 0, n_series_set = 0;
  glk::DevBuf<SeriesDev> d_series;
  // interpolated light components (gl_model_set_light_image): one image table per GL_INTERPOL component, CompDesc::iparam = its slot
  std::vector<InterpDev> interp;               // what the kernels read (d_interp is its copy on the device): pointers into interp_buf
  std::vector<glk::DevBuf<float>> interp_buf;  // the owner of each slot's table, [(h + 4)][(w + 4)] with its zero apron
  int n_interp = 0, n_interp_set = 0;
  glk::DevBuf<InterpDev> d_interp;
  // interpolated lenses (gl_model_set_lens_maps): the same per GL_INTERPOL_MASS component; one buffer holds both maps of a slot
  std::vector<InterpMassDev> interp_mass;
  std::vector<glk::DevBuf<float>> interp_mass_buf;  // [2][(h + 4)][(w + 4)]: alpha_x, alpha_y, each with its zero apron
  int n_interp_mass = 0, n_interp_mass_set = 0;
  int n_multipole = 0;  // GL_MULTIPOLE lenses: the point kernels take the builds that carry the case (gl_positions.hip.h lens_point)
  glk::DevBuf<InterpMassDev> d_interp_mass;
  // linear amplitudes (lstsq_simulate): channel k of the basis stack <-> packed parameter column
  std::vector<int> lin_cols;
  glk::DevBuf<int> d_lin_cols;
  int shp_kernel = 0;    // lenses | [Sersic lens lights] | one shapelet source: served by gl_shp.hip.h (GIGALENS_HIP_SHP=0: the round-2 kernels)
  int tile = 2;          // pixels per thread per tile (template T) for forward-only launches
  int tile_grad = 2;     // ... and for launches that also produce gradients
  int target_wgs = 2048;  // work decomposition target of GIGALENS_HIP_TARGET_WGS (see chunking())
  bool target_wgs_set = false;
};

namespace glk {
// launches the dominant kernel of a call for one mode (gl_launch.hip.h); explicit instantiations live in gl_launch_mode*.hip
template <int MODE>
int launch_main(const gl_model* m, const MainArgs& a, int B, int n_chunks, hipStream_t stream);
// gl_user.hip: compile gl_main_kernel with the model's user bodies (n_bodies HIP C++ sources), fill user_module / user_fn
__attribute__((visibility("hidden"))) int compile_user_model(gl_model* m, const char* const* bodies, int n_bodies);
__attribute__((visibility("hidden"))) int compile_user_points(const gl_model* m);
int match_static(const gl_model* m);
extern template int launch_main<IMG_FWD>(const gl_model*, const MainArgs&, int, int, hipStream_t);
extern template int launch_main<IMG_BWD>(const gl_model*, const MainArgs&, int, int, hipStream_t);
extern template int launch_main<LL_FWD>(const gl_model*, const MainArgs&, int, int, hipStream_t);
extern template int launch_main<LL_GRAD>(const gl_model*, const MainArgs&, int, int, hipStream_t);
extern template int launch_main<IMG_BASIS>(const gl_model*, const MainArgs&, int, int, hipStream_t);
}  // namespace glk
