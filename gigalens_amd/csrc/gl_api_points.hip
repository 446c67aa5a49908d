// gl_api_points.hip -- the entry points of the point family: everything that evaluates the lenses of a model (or one free-standing
// profile) at points through gl_positions.hip.h -- image-position likelihood, lens maps, Hessians, potential, the lens-equation
// solver, critical curves, the Hessian VJP with the weak-lensing shear likelihood, the image-plane position likelihood, and the lens
// planes (maps, render and its VJP, solver, arrival times).
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "gl_host.hip.h"
#include "gl_positions.hip.h"
#include "gl_fluxes.hip.h"
#include "gl_tdelays.hip.h"
#include "gl_images.hip.h"
#include "gl_critical.hip.h"
#include "gl_potential.hip.h"
#include "gl_multiplane.hip.h"
#include "gl_multiplane_bwd.hip.h"
#include "gl_multiplane_pos.hip.h"
#include "gl_multiplane_images.hip.h"
#include "gl_multiplane_fermat.hip.h"
#include "gl_multiplane_tdelays.hip.h"
#include "gl_multiplane_critical.hip.h"
#include "gl_lens_vjp.hip.h"
#include "gl_hessian_vjp.hip.h"
#include "gl_imgplane.hip.h"

using namespace glk;

namespace {
// What every point kernel reads of a model (gl_positions.hip.h PosArgs): the lenses, the packed rows, the catalogues, the series
// fields.  `series` is set for every user; it is non-null only in gl_lens_maps on the model's own grid, the one user that serves
// series-expansion lenses -- the others (run_positions, gl_lens_potential, gl_image_positions, gl_critical_curves) refuse a model
// that holds one before they launch, and a model without one has no d_series.
PosArgs point_args(const gl_model* m, const float* params, int B) {
  PosArgs a{};
  a.comps = m->d_comps;
  a.n_lens = m->n_lens;
  a.P = m->P;
  a.B = B;
  a.params = params;
  a.cats = m->d_cats;
  a.gal_table = m->d_gal_table;
  a.gal_static = m->d_gal_static;
  a.series = m->d_series;
  a.interp_mass = m->d_interp_mass;
  return a;
}

// the window of the lens-equation solver (`search` wording) and of the critical curves
int check_window(bool search, float x_lo, float x_hi, float y_lo, float y_hi) {
  if ((x_hi > x_lo) && (y_hi > y_lo) && std::isfinite(x_hi - x_lo) && std::isfinite(y_hi - y_lo)) return GL_OK;
  return search ? fail(GL_EINVAL, "empty or non-finite search window [%g, %g] x [%g, %g]", x_lo, x_hi, y_lo, y_hi)
                : fail(GL_EINVAL, "empty or non-finite window [%g, %g] x [%g, %g]", x_lo, x_hi, y_lo, y_hi);
}

bool potential_kind(int kind) {
  return (kind >= GL_EPL && kind <= GL_DPIEP) || kind == GL_NFW_ELLIPSE || kind == GL_TNFW || kind == GL_MULTIPOLE;
}

// the lenses without a potential: what gl_lens_potential and the time-delay term (gl_model_set_position_delays) refuse
int refuse_potential_lenses(const gl_model* m) {
  for (int l = 0; l < m->n_lens; ++l) {
    const int kind = m->comps[l].kind;
    if (kind == GL_SERIES)
      return fail(GL_EUNSUPPORTED, "lens %d is a series expansion: its precomputed field holds the deflection, no potential", l);
    if (kind == GL_USER_MASS)
      return fail(GL_EUNSUPPORTED, "lens %d is a user-written body (or a run-time compiled ScalingRelation member loop): "
                                   "a body defines the deflection only, no potential", l);
    if (kind == GL_INTERPOL_MASS)
      return fail(GL_EUNSUPPORTED, "lens %d is an interpolated lens (INTERPOL_SCALED): its maps hold the deflection, no potential", l);
    if (!potential_kind(kind) && kind != GL_SCALED) return fail(GL_EUNSUPPORTED, "lens %d: kind %d has no potential", l, kind);
  }
  return GL_OK;
}

// the lenses the ray-shoot VJP (gl_lens_maps_vjp) and what is built on it or on its Hessian twin refuse, after the lens planes
int refuse_vjp_lenses(const gl_model* m, const char* fn, const char* what) {
  if (int rp = refuse_planes(m, fn)) return rp;
  for (int l = 0; l < m->n_lens; ++l) {
    const int kind = m->comps[l].kind;
    if (kind == GL_SERIES)
      return fail(GL_EUNSUPPORTED, "lens %d is a series expansion: its field lives on the model grid and has no parameter derivative here", l);
    if (kind == GL_USER_MASS)
      return fail(GL_EUNSUPPORTED, "lens %d is a user-written body (or a run-time compiled ScalingRelation member loop): "
                                   "not served by %s", l, what);
  }
  return GL_OK;
}

struct ImgLayout { size_t map, cand, n_cand, n_over, scale, bytes; };
ImgLayout img_layout(int B, int n_src, int n_cells, int n_maps = 1) {
  ImgLayout l{};
  const size_t V = (size_t)(n_cells + 1) * (size_t)(n_cells + 1), BS = (size_t)B * (size_t)n_src;
  l.map = 0;
  l.cand = l.map + (size_t)n_maps * align_up((size_t)B * V * sizeof(float2), 256);
  l.n_cand = l.cand + align_up(BS * IMG_MAXC * sizeof(float2), 256);
  l.n_over = l.n_cand + align_up(BS * sizeof(int), 256);
  l.scale = l.n_over + align_up(BS * sizeof(int), 256);  // [n_src] deflection scales of gl_image_positions_scaled
  l.bytes = l.scale + align_up((size_t)n_src * sizeof(float), 256);
  return l;
}
constexpr int IMG_MAX_CELLS = 8192;
// ... on K lens planes (gl_multiplane_image_positions): the single-plane layout with K maps -- the plane sums [B][K][(n+1)^2] of
// gl_multiplane_images.hip.h, contiguous from `map` -- and behind it the coupling rows [n_src][K] of the sources
struct MpImgLayout { ImgLayout img; size_t tgt, bytes; };
MpImgLayout mp_img_layout(int B, int n_src, int n_cells, int K) {
  MpImgLayout l{};
  l.img = img_layout(B, n_src, n_cells, K);
  l.tgt = l.img.bytes;
  l.bytes = l.tgt + align_up((size_t)n_src * (size_t)K * sizeof(float), 256);
  return l;
}

// the two stage-count entries: the shared size rules, and the copy of the scan's two planes out of a workspace of layout `lay`
// (`bytes_needed`: the whole workspace of the call that filled it)
int check_stage_counts_sizes(int B, int n_src, int n_cells) {
  if (B <= 0 || n_src <= 0) return fail(GL_EINVAL, "B (%d) and n_src (%d) must be positive", B, n_src);
  if (n_cells <= 0 || n_cells > IMG_MAX_CELLS) return fail(GL_EINVAL, "n_cells %d outside [1, %d]", n_cells, IMG_MAX_CELLS);
  return GL_OK;
}
int copy_stage_counts(const ImgLayout& lay, size_t bytes_needed, const void* workspace, size_t workspace_bytes, int B, int n_src,
                      int* n_cand, int* n_over, void* hip_stream) {
  if (workspace_bytes < bytes_needed) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, bytes_needed);
  const size_t bytes = sizeof(int) * (size_t)B * (size_t)n_src;
  const char* base = (const char*)workspace;
  hipStream_t stream = (hipStream_t)hip_stream;
  GL_HIP(hipMemcpyAsync(n_cand, base + lay.n_cand, bytes, hipMemcpyDeviceToDevice, stream));
  GL_HIP(hipMemcpyAsync(n_over, base + lay.n_over, bytes, hipMemcpyDeviceToDevice, stream));
  return GL_OK;
}

// ... and of the arrival times on K lens planes (gl_multiplane_fermat): the weight rows [n_src][K] and [K], as doubles
struct MpFermatLayout { size_t geom, pot, bytes; };
MpFermatLayout mp_fermat_layout(int n_src, int K) {
  MpFermatLayout l{};
  l.geom = 0;
  l.pot = l.geom + align_up((size_t)n_src * (size_t)K * sizeof(double), 256);
  l.bytes = l.pot + align_up((size_t)K * sizeof(double), 256);
  return l;
}

struct CritLayout { size_t dmap, edge_id, edge_pt, edge_omk, n_edges, n_edge_over, bytes; };
CritLayout crit_layout(int B, int n_cells, int max_segments) {
  CritLayout l{};
  const size_t V = (size_t)(n_cells + 1) * (size_t)(n_cells + 1), BE = (size_t)B * 2 * (size_t)max_segments;
  l.dmap = 0;
  l.edge_id = l.dmap + align_up((size_t)B * V * sizeof(float), 256);
  l.edge_pt = l.edge_id + align_up(BE * sizeof(int), 256);
  l.edge_omk = l.edge_pt + align_up(BE * sizeof(float4), 256);
  l.n_edges = l.edge_omk + align_up(BE * sizeof(float), 256);
  l.n_edge_over = l.n_edges + align_up((size_t)B * sizeof(int), 256);
  l.bytes = l.n_edge_over + align_up((size_t)B * sizeof(int), 256);
  return l;
}
constexpr int CRIT_MAX_SEGMENTS = 1 << 20;
// ... on K lens planes (gl_multiplane_critical_curves): the single-plane layout with the rows (sample, source) in the place of the
// samples, and behind it the coupling rows [n_src][K] of the sources
struct MpCritLayout { CritLayout crit; size_t tgt, bytes; };
MpCritLayout mp_crit_layout(int B, int n_src, int n_cells, int max_segments, int K) {
  MpCritLayout l{};
  l.crit = crit_layout(B * n_src, n_cells, max_segments);
  l.tgt = l.crit.bytes;
  l.bytes = l.tgt + align_up((size_t)n_src * (size_t)K * sizeof(float), 256);
  return l;
}

// the coupling rows [n_src][K] of the sources of a call on lens planes: the rules of gl_model_set_position_targets
int check_target_rows(const float* targets, int n_src, int K) {
  for (int s = 0; s < n_src; ++s) {
    const float* T = targets + (size_t)s * K;
    for (int i = 0; i < K; ++i)
      if (!(std::isfinite(T[i]) && T[i] >= 0.f) || (i > 0 && T[i] != 0.f && T[i - 1] == 0.f))
        return fail(GL_EINVAL, "targets[%d][%d] = %g: finite and >= 0, 0 from the first plane at or behind the source on", s, i, T[i]);
    if (T[0] == 0.f) return fail(GL_EINVAL, "source %d: every coupling is zero (the source lies behind no lens plane)", s);
  }
  return GL_OK;
}

// what the kernels of a model with lens planes read of them (gl_multiplane.hip.h MpArgs)
MpArgs mp_args(const gl_model* m) {
  MpArgs a{};
  a.order = m->d_mp_lens;
  a.plane = m->d_mp_lens + m->n_lens;
  a.scale = m->d_mp_scale;
  return a;
}
}  // namespace

namespace glk {

// P1 of a model that holds a multipole: the build of the kernel that carries the case (gl_positions.hip.h pos_p1_body), on the grid
// run_positions hands in -- the one it gives gl_pos_p1_kernel
static void launch_pos_p1_mpl(dim3 grid, hipStream_t stream, const PosArgs& a) {
  hipLaunchKernelGGL(gl_pos_p1_mpl_kernel, grid, dim3(64), 0, stream, a);
}

// The time-delay term on lens planes (gl_multiplane_tdelays.hip.h) in the plane branch of run_positions: the tables the model
// holds and the scratch of the workspace, then -- after the flux kernel -- the rays and the family statistics, and -- after P3 -- the
// direct part of the gradient.  One thread per (sample, image), per (sample, family) and per (sample, image, lens-parameter column).
static MpDelayArgs mp_delay_args(const gl_model* m, const Workspace& w) {
  MpDelayArgs q{};
  const float* tab = m->d_mpd_delay.get();
  q.delay = tab;
  q.delay_err = tab + m->pos_J;
  q.lam_given = tab + 2 * m->pos_J;
  q.geom = m->d_mpd_weight.get();
  q.pot = q.geom + (size_t)m->pos_J * MP_MAXK;
  q.trace = w.mpd_trace;
  q.src = w.mpd_src;
  q.aj = w.mpd_aj;
  return q;
}
static unsigned mp_delay_blocks(long long n) { return (unsigned)((n + MP_TDELAY_WG - 1) / MP_TDELAY_WG); }
static void launch_mp_tdelay_stats(const gl_model* m, const PosArgs& a, const Workspace& w, int accumulate, const DelayOut* delay_out,
                                   hipStream_t stream) {
  const DelayOut none{nullptr, nullptr, nullptr};
  const DelayOut& o = delay_out ? *delay_out : none;
  const MpDelayArgs q = mp_delay_args(m, w);
  hipLaunchKernelGGL(gl_mp_pos_tdelay_trace_kernel, dim3(mp_delay_blocks((long long)a.B * a.J)), dim3(MP_TDELAY_WG), 0, stream, a,
                     mp_args(m), (const float*)m->d_pos_target, q);
  hipLaunchKernelGGL(gl_mp_pos_tdelay_kernel, dim3(mp_delay_blocks((long long)a.B * a.F)), dim3(MP_TDELAY_WG), 0, stream, a, q, accumulate,
                     o.scale, o.offset, o.model_delay);
}
static void launch_mp_tdelay_grad(const gl_model* m, const PosArgs& a, const Workspace& w, hipStream_t stream) {
  hipLaunchKernelGGL(gl_mp_pos_tdelay_grad_kernel, dim3(mp_delay_blocks((long long)a.B * a.J * m->lens_params)), dim3(MP_TDELAY_WG), 0,
                     stream, a, mp_args(m), mp_delay_args(m, w), m->lens_params);
}

int run_positions(const gl_model* m, const float* params, int B, const Workspace& w, bool want_grad, hipStream_t stream, int what,
                  float* amp, float* model_flux, const DelayOut* delay_out) {
  if (m->n_series) return fail(GL_EUNSUPPORTED, "a series-expansion lens lives on the pixel grid only (series_profile.py:76-81): no image-position likelihood");
  if ((what & POS_FLUXES) && !m->pos_n_flux) return fail(GL_EINVAL, "gl_model_set_position_fluxes has not been called on this model");
  if ((what & POS_DELAYS) && !m->pos_n_delay) return fail(GL_EINVAL, "gl_model_set_position_delays has not been called on this model");
  // (gl_model_set_position_delays, gl_model_set_position_scales and gl_model_set_lens_planes see to it that a model with delays is
  // one plane of built-in lenses whose families with delays lie on the reference plane)
  if ((what & POS_DELAYS) && (m->mp_K >= 2 || m->has_user))
    return fail(GL_EUNSUPPORTED, "the time-delay term serves one lens plane of built-in lenses");
  if ((what & POS_PLANE_DELAYS) && !(m->mp_K >= 2 && m->mpd_n_delay))
    return fail(GL_EINVAL, "gl_model_set_position_plane_delays has not been called on this model");
  if (m->has_user)  // the four kernels below, compiled at run time with the user's bodies on the nested duals (once per model text)
    if (int rc = compile_user_points(m)) return rc;
  PosArgs a = point_args(m, params, B);  // + the position tables and the likelihood's workspace
  a.J = m->pos_J;
  a.F = m->pos_F;
  a.px = m->d_pos;
  a.py = m->d_pos + m->pos_J;
  a.ex = m->d_pos + 2 * m->pos_J;
  a.ey = m->d_pos + 3 * m->pos_J;
  a.fam_off = m->d_fam;
  const bool planes = m->mp_K >= 2;  // families at redshifts of their own behind lens planes (gl_multiplane_pos.hip.h)
  a.fam_scale = !planes && m->pos_scaled ? m->d_pos_scale.get() : nullptr;
  a.w_pos = w.pos_w;
  a.w_adj = w.pos_adj;
  a.w_g = w.pos_g;
  a.w_fam = w.pos_fam;
  a.ll = w.pos_ll;
  a.chi2 = w.pos_chi2;
  a.grad = want_grad ? w.pos_grad : nullptr;
  auto blocks = [](long long n) { return dim3((unsigned)((n + 63) / 64)); };
  // P2 of the terms asked for: the position statistics, the flux ratios (gl_fluxes.hip.h; from the static library for every model --
  // it evaluates no lens) or the former with the latter added by the thread that owns the same elements
  auto fluxes = [&]() {
    if (what & POS_FLUXES)
      hipLaunchKernelGGL(gl_pos_flux_kernel, blocks((long long)B * a.F), dim3(64), 0, stream, a, (const float*)m->d_pos_flux.get(),
                         (const float*)(m->d_pos_flux.get() + m->pos_J), (what & POS_POSITIONS) ? 1 : 0, amp, model_flux);
  };
  if (planes) {  // P1 and P3 through the plane recursion, P2 and P4 as on one plane
    if (!m->pos_targets)
      return fail(GL_EINVAL, "the image positions of a model with lens planes need the couplings of their families: "
                             "gl_model_set_position_targets has not been called");
    if (want_grad && m->lens_params && m->n_multipole)
      return fail(GL_EUNSUPPORTED, "the gradient of the point likelihoods of a model with lens planes is not served with a GL_MULTIPOLE "
                                   "lens: gl_mp_pos_p3_kernel is built without that case (with it the kernel spills)");
    const float* tg = m->d_pos_target;
    hipLaunchKernelGGL(gl_mp_pos_p1_kernel, blocks((long long)B * a.J), dim3(MP_POS_WG), 0, stream, a, mp_args(m), tg);
    if (what & POS_POSITIONS) hipLaunchKernelGGL(gl_pos_p2_kernel, blocks((long long)B * a.F), dim3(64), 0, stream, a);
    fluxes();
    // the time delays on planes (gl_multiplane_tdelays.hip.h): the rays on double, then statistics and beta adjoints by the thread
    // that owns the family's elements; the direct d T / d params part is added to what P3 wrote, before P4 sums it
    if (what & POS_PLANE_DELAYS) launch_mp_tdelay_stats(m, a, w, (what & (POS_POSITIONS | POS_FLUXES)) ? 1 : 0, delay_out, stream);
    if (want_grad && m->lens_params) {
      hipLaunchKernelGGL(gl_mp_pos_p3_kernel, blocks((long long)B * a.J * m->lens_params), dim3(MP_POS_WG), 0, stream, a, mp_args(m),
                         tg, m->lens_params);
      if (what & POS_PLANE_DELAYS) launch_mp_tdelay_grad(m, a, w, stream);
    }
    hipLaunchKernelGGL(gl_pos_p4_kernel, blocks((long long)B * (a.P + 1)), dim3(64), 0, stream, a, m->lens_params);
    GL_HIP(hipGetLastError());
    return GL_OK;
  }
  if (m->has_user) {
    int lens_params = m->lens_params;
    void* args1[] = {&a};
    void* args2[] = {&a, &lens_params};
    auto go = [&](int k, long long n, void** args) {
      return hipModuleLaunchKernel(m->user_point_fn[k], blocks(n).x, 1, 1, 64, 1, 1, 0, stream, args, nullptr);
    };
    GL_HIP(go(0, (long long)B * a.J, args1));
    if (what & POS_POSITIONS) GL_HIP(go(1, (long long)B * a.F, args1));
    fluxes();
    if (want_grad && m->lens_params) GL_HIP(go(2, (long long)B * a.J * m->lens_params, args2));
    GL_HIP(go(3, (long long)B * (a.P + 1), args2));
    if (what & POS_FLUXES) GL_HIP(hipGetLastError());  // (the flux launch between the module's kernels)
    return GL_OK;
  }
  if (m->n_multipole) launch_pos_p1_mpl(blocks((long long)B * a.J), stream, a);
  else hipLaunchKernelGGL(gl_pos_p1_kernel, blocks((long long)B * a.J), dim3(64), 0, stream, a);
  if (what & POS_POSITIONS) hipLaunchKernelGGL(gl_pos_p2_kernel, blocks((long long)B * a.F), dim3(64), 0, stream, a);
  fluxes();
  // the time delays (gl_tdelays.hip.h): statistics and beta adjoints by the thread that owns the family's elements, the direct
  // d psi / d params part added to what P3 wrote, before P4 sums it
  if (what & POS_DELAYS) {
    const float* tab = m->d_pos_delay.get();
    const DelayOut none{nullptr, nullptr, nullptr};
    const DelayOut& o = delay_out ? *delay_out : none;
    hipLaunchKernelGGL(gl_pos_tdelay_kernel, blocks((long long)B * a.F), dim3(64), 0, stream, a, tab, tab + m->pos_J, tab + 2 * m->pos_J,
                       (what & (POS_POSITIONS | POS_FLUXES)) ? 1 : 0, w.pos_dadj, o.scale, o.offset, o.model_delay);
  }
  if (want_grad && m->lens_params) {
    hipLaunchKernelGGL(gl_pos_p3_kernel, blocks((long long)B * a.J * m->lens_params), dim3(64), 0, stream, a,
                       m->lens_params);
    if (what & POS_DELAYS)
      hipLaunchKernelGGL(gl_pos_tdelay_grad_kernel, blocks((long long)B * a.J * m->lens_params), dim3(64), 0, stream, a,
                         (const float*)w.pos_dadj, m->lens_params);
  }
  hipLaunchKernelGGL(gl_pos_p4_kernel, blocks((long long)B * (a.P + 1)), dim3(64), 0, stream, a, m->lens_params);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // namespace glk

namespace {
// What the four point-likelihood entries share after their own refusals: the call checks (then the lens planes, where the entry
// needs them), the terms `what` through run_positions, and the results copied out of the workspace.
int point_term_call(const gl_model* m, const float* params, int B, float* loglike, float* chi2, float* grad_params_or_null,
                    void* workspace, size_t workspace_bytes, void* hip_stream, bool need_planes = false, int what = POS_POSITIONS,
                    float* amp = nullptr, float* model_flux = nullptr, const DelayOut* delay_out = nullptr) {
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w);
  if (rc) return rc;
  if (need_planes && (rc = check_planes_set(m))) return rc;
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if (!loglike || !chi2) return fail(GL_EINVAL, "loglike / chi2 is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = run_positions(m, params, B, w, grad_params_or_null != nullptr, stream, what, amp, model_flux, delay_out))) return rc;
  GL_HIP(hipMemcpyAsync(loglike, w.pos_ll, sizeof(float) * B, hipMemcpyDeviceToDevice, stream));
  GL_HIP(hipMemcpyAsync(chi2, w.pos_chi2, sizeof(float) * B, hipMemcpyDeviceToDevice, stream));
  if (grad_params_or_null)
    GL_HIP(hipMemcpyAsync(grad_params_or_null, w.pos_grad, sizeof(float) * (size_t)B * m->P, hipMemcpyDeviceToDevice, stream));
  return GL_OK;
}
}  // namespace

extern "C" {

int gl_positions_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                         float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rp = refuse_planes(m, "gl_positions_fwd_bwd")) return rp;
  return point_term_call(m, params, B, loglike, chi2, grad_params_or_null, workspace, workspace_bytes, hip_stream);
}

int gl_multiplane_positions_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                                    float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return point_term_call(m, params, B, loglike, chi2, grad_params_or_null, workspace, workspace_bytes, hip_stream, true);
}

int gl_position_fluxes_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2, float* grad_params_or_null,
                               float* amplitude_or_null, float* model_flux_or_null, void* workspace, size_t workspace_bytes,
                               void* hip_stream) {
  return point_term_call(m, params, B, loglike, chi2, grad_params_or_null, workspace, workspace_bytes, hip_stream, false, POS_FLUXES,
                         amplitude_or_null, model_flux_or_null);
}

// ---- time delays of the image families (gl_tdelays.hip.h) ---------------------------------------------------------------
int gl_model_set_position_delays(gl_model* m, const float* delay, const float* delay_err, int n_images, const float* scale_per_family,
                                 int n_families) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  auto clear = [&]() {
    m->pos_n_delay = 0;
    m->d_pos_delay.reset();
    m->pos_fam_delay.clear();
    return GL_OK;
  };
  if (!delay) return clear();  // no delays: the model as gl_model_set_positions left it
  if (!delay_err || !scale_per_family) return fail(GL_EINVAL, "delay_err / scale_per_family is null");
  if (n_images != m->pos_J) return fail(GL_EINVAL, "%d arrival times for %d image(s)", n_images, m->pos_J);
  if (n_families != m->pos_F) return fail(GL_EINVAL, "%d delay scales for %d image famil(ies)", n_families, m->pos_F);
  int n_delay = 0;
  std::vector<char> has(m->pos_F, 0);
  for (int f = 0; f < m->pos_F; ++f) {
    int n = 0;
    for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) {
      if (std::isnan(delay[j])) continue;  // not measured
      if (!std::isfinite(delay[j])) return fail(GL_EINVAL, "arrival time %d (%g) is not finite", j, delay[j]);
      if (!(std::isfinite(delay_err[j]) && delay_err[j] > 0.f))
        return fail(GL_EINVAL, "arrival-time error %d (%g) is not finite and > 0", j, delay_err[j]);
      ++n;
    }
    if (n == 1)
      return fail(GL_EINVAL, "image family %d has one measured arrival time: the term constrains delay differences, a family takes two "
                             "or more, or none", f);
    if (n && std::isinf(scale_per_family[f])) return fail(GL_EINVAL, "delay scale %d (%g) is not finite (NaN: profiled out)", f, scale_per_family[f]);
    if (n == 2 && std::isnan(scale_per_family[f]))
      return fail(GL_EINVAL, "image family %d has two measured arrival times and a profiled delay scale: the fit is exact and "
                             "constrains nothing, a profiled scale takes three or more", f);
    has[f] = n > 0;
    n_delay += n;
  }
  if (!n_delay) return clear();  // every time is NaN: none
  if (m->mp_K >= 2) return fail(GL_EUNSUPPORTED, "the time-delay term is not served on lens planes (gl_model_set_lens_planes)");
  for (int f = 0; f < m->pos_F; ++f)
    if (has[f] && f < (int)m->pos_fam_scale.size() && m->pos_fam_scale[f] != 1.f)
      return fail(GL_EUNSUPPORTED, "image family %d has a deflection scale of %g (gl_model_set_position_scales): the Fermat potential "
                                   "of a scaled source plane is not served", f, m->pos_fam_scale[f]);
  if (int rc = refuse_potential_lenses(m)) return rc;
  std::vector<float> tab((size_t)2 * m->pos_J + m->pos_F);
  std::copy(delay, delay + m->pos_J, tab.begin());
  std::copy(delay_err, delay_err + m->pos_J, tab.begin() + m->pos_J);
  std::copy(scale_per_family, scale_per_family + m->pos_F, tab.begin() + 2 * (size_t)m->pos_J);
  glk::DevBuf<float> fresh;  // (a failed upload leaves the model as it was)
  GL_HIP(fresh.upload(tab.data(), tab.size()));
  m->d_pos_delay = std::move(fresh);
  m->pos_fam_delay = has;
  m->pos_n_delay = n_delay;
  return GL_OK;
}

int gl_position_delays_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2, float* grad_params_or_null,
                               float* scale_or_null, float* offset_or_null, float* model_delay_or_null, void* workspace,
                               size_t workspace_bytes, void* hip_stream) {
  const DelayOut out{scale_or_null, offset_or_null, model_delay_or_null};
  return point_term_call(m, params, B, loglike, chi2, grad_params_or_null, workspace, workspace_bytes, hip_stream, false, POS_DELAYS,
                         nullptr, nullptr, &out);
}

// ---- ... on lens planes (gl_multiplane_tdelays.hip.h) ---------------------------------------------------------------------
int gl_model_set_position_plane_delays(gl_model* m, const float* delay, const float* delay_err, int n_images, const double* geom,
                                       const double* pot, const float* scale_per_family, int n_families, int n_planes) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if (!delay) {  // no delays: the model as gl_model_set_position_targets left it
    m->clear_plane_delays();
    return GL_OK;
  }
  if (!delay_err || !scale_per_family || !geom || !pot) return fail(GL_EINVAL, "delay_err / geom / pot / scale_per_family is null");
  if (n_images != m->pos_J) return fail(GL_EINVAL, "%d arrival times for %d image(s)", n_images, m->pos_J);
  if (n_families != m->pos_F) return fail(GL_EINVAL, "%d delay scales for %d image famil(ies)", n_families, m->pos_F);
  int n_delay = 0;
  for (int f = 0; f < m->pos_F; ++f) {  // (the rules of gl_model_set_position_delays)
    int n = 0;
    for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) {
      if (std::isnan(delay[j])) continue;  // not measured
      if (!std::isfinite(delay[j])) return fail(GL_EINVAL, "arrival time %d (%g) is not finite", j, delay[j]);
      if (!(std::isfinite(delay_err[j]) && delay_err[j] > 0.f))
        return fail(GL_EINVAL, "arrival-time error %d (%g) is not finite and > 0", j, delay_err[j]);
      ++n;
    }
    if (n == 1)
      return fail(GL_EINVAL, "image family %d has one measured arrival time: the term constrains delay differences, a family takes two "
                             "or more, or none", f);
    if (n && std::isinf(scale_per_family[f])) return fail(GL_EINVAL, "delay scale %d (%g) is not finite (NaN: profiled out)", f, scale_per_family[f]);
    if (n == 2 && std::isnan(scale_per_family[f]))
      return fail(GL_EINVAL, "image family %d has two measured arrival times and a profiled delay scale: the fit is exact and "
                             "constrains nothing, a profiled scale takes three or more", f);
    n_delay += n;
  }
  if (m->mp_K < 2) return fail(GL_EINVAL, "gl_model_set_lens_planes has not been called on this model (one plane: gl_model_set_position_delays)");
  if (!m->pos_targets) return fail(GL_EINVAL, "gl_model_set_position_targets has not been called on this model");
  if (n_planes != m->mp_K) return fail(GL_EINVAL, "delay weights of %d planes for %d lens planes", n_planes, m->mp_K);
  const int K = n_planes;
  for (int i = 0; i < K; ++i)
    if (!(std::isfinite(pot[i]) && pot[i] >= 0.)) return fail(GL_EINVAL, "pot[%d] = %g: finite and >= 0", i, pot[i]);
  for (int f = 0; f < m->pos_F; ++f) {  // a row of MultiPlane.delay_weights: the zeros are those of the family's coupling row
    const double* g = geom + (size_t)f * K;
    const float* T = m->pos_target_rows.data() + (size_t)f * K;
    for (int i = 0; i < K; ++i) {
      if (!(std::isfinite(g[i]) && g[i] >= 0.)) return fail(GL_EINVAL, "geom[%d][%d] = %g: finite and >= 0", f, i, g[i]);
      if ((g[i] != 0.) != (T[i] != 0.f))
        return fail(GL_EINVAL, "geom[%d][%d] = %g against the coupling %g of gl_model_set_position_targets: the planes in front of a "
                               "family are the same in both rows", f, i, g[i], T[i]);
    }
  }
  if (int rc = refuse_potential_lenses(m)) return rc;
  if (!n_delay) {  // every time is NaN: none
    m->clear_plane_delays();
    return GL_OK;
  }
  std::vector<float> tab((size_t)2 * m->pos_J + m->pos_F);
  std::copy(delay, delay + m->pos_J, tab.begin());
  std::copy(delay_err, delay_err + m->pos_J, tab.begin() + m->pos_J);
  std::copy(scale_per_family, scale_per_family + m->pos_F, tab.begin() + 2 * (size_t)m->pos_J);
  std::vector<double> wt((size_t)(m->pos_J + 1) * MP_MAXK, 0.);
  for (int f = 0; f < m->pos_F; ++f)
    for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) std::copy(geom + (size_t)f * K, geom + (size_t)(f + 1) * K, wt.begin() + (size_t)j * MP_MAXK);
  std::copy(pot, pot + K, wt.begin() + (size_t)m->pos_J * MP_MAXK);
  glk::DevBuf<float> fresh;  // (a failed upload leaves the model as it was)
  glk::DevBuf<double> fresh_wt;
  GL_HIP(fresh.upload(tab.data(), tab.size()));
  GL_HIP(fresh_wt.upload(wt.data(), wt.size()));
  m->d_mpd_delay = std::move(fresh);
  m->d_mpd_weight = std::move(fresh_wt);
  m->mpd_n_delay = n_delay;
  return GL_OK;
}

int gl_multiplane_position_delays_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                                          float* grad_params_or_null, float* scale_or_null, float* offset_or_null,
                                          float* model_delay_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const DelayOut out{scale_or_null, offset_or_null, model_delay_or_null};
  return point_term_call(m, params, B, loglike, chi2, grad_params_or_null, workspace, workspace_bytes, hip_stream, true, POS_PLANE_DELAYS,
                         nullptr, nullptr, &out);
}

// ---- per-family read-back: w_fam of the most recent point-likelihood call on this workspace -----------------------------
int gl_position_family_terms(const gl_model* m, void* workspace, size_t workspace_bytes, int B, float* out, void* hip_stream) {
  if (!out) return fail(GL_EINVAL, "out is null");
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, out, B, workspace, workspace_bytes, &plan, &w);  // (no packed rows here: `out` stands in for the null check)
  if (rc) return rc;
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  GL_HIP(hipMemcpyAsync(out, w.pos_fam, sizeof(float) * (size_t)B * m->pos_F * 2, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return GL_OK;
}

int gl_profile_hessian(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                       const float* params, float* out, void* hip_stream) {
  if (!comp || !x || !y || !params || !out) return fail(GL_EINVAL, "null argument");
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  if (!potential_kind(comp->kind))
    return fail(GL_EINVAL, "kind %d is not a free-standing mass profile", comp->kind);
  const CompDesc cd = point_comp(comp);
  const long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_profile_hessian_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream,
                     cd, x, y, (long long)n_pts, B, xy_batched, params, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_interpol_mass_eval(const gl_component* comp, int h, int w, const float* alpha_x_dev, const float* alpha_y_dev, double pitch,
                          const float* x, const float* y, int64_t n_pts, int B, int xy_batched, const float* params, float* out0,
                          float* out1, int hessian, void* hip_stream) {
  if (!comp || !alpha_x_dev || !alpha_y_dev || !x || !y || !params || !out0 || (!hessian && !out1)) return fail(GL_EINVAL, "null argument");
  if (comp->kind != GL_INTERPOL_MASS) return fail(GL_EINVAL, "kind %d is not GL_INTERPOL_MASS", comp->kind);
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  if (h < 1 || h > GL_INTERPOL_MAX_SIDE || w < 1 || w > GL_INTERPOL_MAX_SIDE)
    return fail(GL_EINVAL, "deflection maps of %d x %d pixels: height and width must lie in 1..%d", h, w, GL_INTERPOL_MAX_SIDE);
  if (!(std::isfinite(pitch) && pitch > 0.0 && std::isfinite((float)(1.0 / pitch)) && (float)(1.0 / pitch) > 0.f))
    return fail(GL_EINVAL, "pitch %g is not finite and > 0", pitch);
  const InterpMassDev tb{alpha_x_dev, alpha_y_dev, h, w, (float)(1.0 / pitch)};
  const long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_interpol_mass_point_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, tb, x,
                     y, (long long)n_pts, B, xy_batched, params, out0, out1, hessian);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_scaled_hessian(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev, const float* x,
                      const float* y, int64_t n_pts, int B, int xy_batched, const float* scales, int n_scales,
                      float* out, void* hip_stream) {
  if (!scale_col || !table_dev || !x || !y || !scales || !out) return fail(GL_EINVAL, "null argument");
  if (int rc = check_catalogue_args(false, base_kind, n_galaxies > 0 && n_pts > 0 && B > 0, 0, scale_col, n_scales)) return rc;
  ScaledDesc sd{base_kind, n_galaxies, {scale_col[0], scale_col[1], scale_col[2]}};
  long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_scaled_hessian_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream,
                     sd, table_dev, x, y, (long long)n_pts, B, xy_batched, scales, n_scales, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_lens_maps(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts,
                 int xy_batched, float* out, void* hip_stream) {
  if (!m || !params || !out) return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_lens_maps")) return rp;
  if (m->has_user)  // the kernel below compiled at run time with the user's bodies (Hessians from the duals)
    if (int rc = compile_user_points(m)) return rc;
  if ((x == nullptr) != (y == nullptr)) return fail(GL_EINVAL, "x and y must both be given or both be null");
  if (B <= 0 || n_pts <= 0) return fail(GL_EINVAL, "B and n_pts must be positive");
  if (int rc = check_ready(m, false, false)) return rc;
  if (!x) {
    if (n_pts != m->N || xy_batched) return fail(GL_EINVAL, "the model grid has %d points and is not batched", m->N);
    x = m->d_gx;
    y = m->d_gy;
    for (const SeriesDev& sv : m->series)
      if (!sv.coef || !sv.hcoef)
        return fail(GL_EINVAL, "GL_SERIES lens without its deflection / Hessian field (gl_model_set_series, gl_model_set_series_hessian)");
  } else if (m->n_series) {
    return fail(GL_EUNSUPPORTED, "a series-expansion lens lives on the model grid only (series_profile.py:76-89): pass x = y = NULL");
  }
  PosArgs a = point_args(m, params, B);
  const long long total = (long long)n_pts * B;
  if (m->has_user) {
    long long n_pts_ll = (long long)n_pts;
    void* args[] = {&a, &x, &y, &n_pts_ll, &xy_batched, &out};
    GL_HIP(hipModuleLaunchKernel(m->user_point_fn[4], (unsigned)((total + 63) / 64), 1, 1, 64, 1, 1, 0, (hipStream_t)hip_stream, args, nullptr));
    return GL_OK;
  }
  if (m->n_multipole)  // (the build that carries the multipole: gl_positions.hip.h lens_maps_body)
    hipLaunchKernelGGL(gl_lens_maps_mpl_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, a,
                       x, y, (long long)n_pts, xy_batched, out);
  else
    hipLaunchKernelGGL(gl_lens_maps_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, a,
                       x, y, (long long)n_pts, xy_batched, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- VJP of the ray-shoot (gl_lens_vjp.hip.h) ------------------------------------------------------------------
namespace {
// blocks of VJP_PTS points per (sample, lens column); 0: a size the call refuses
long long vjp_blocks(const gl_model* m, int B, int64_t n_pts) {
  if (!m || B <= 0 || n_pts <= 0) return 0;
  const long long n_blocks = ((long long)n_pts + VJP_PTS - 1) / VJP_PTS;
  const long long rows = (long long)B * std::max(m->lens_params, 1);
  return n_blocks <= 0x7fffffffLL / rows && (long long)B * std::max(m->P, 1) <= 0x7fffffffLL ? n_blocks : 0;
}

// The launch pair of a lens VJP: `kernel` -- gl_lens_vjp_kernel (the ray-shoot) or gl_hessian_vjp_kernel, one signature -- writes
// one partial per (sample, lens column, block of points), gl_lens_vjp_sum_kernel sums them into grad_params.
using VjpKernel = void (*)(PosArgs, const float*, const float*, long long, int, const float*, int, int, float*);
void launch_vjp(VjpKernel kernel, const gl_model* m, const float* params, int B, const float* x, const float* y, long long n_pts,
                int xy_batched, const float* cot, float* grad_params, float* partial, long long n_blocks, hipStream_t stream) {
  if (m->lens_params)
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)B * m->lens_params * n_blocks)), dim3(VJP_WG), 0, stream,
                       point_args(m, params, B), x, y, n_pts, xy_batched, cot, m->lens_params, (int)n_blocks, partial);
  hipLaunchKernelGGL(gl_lens_vjp_sum_kernel, dim3((unsigned)((long long)B * m->P)), dim3(VJP_WG), 0, stream, (const float*)partial,
                     m->P, m->lens_params, (int)n_blocks, grad_params);
}
}  // namespace

size_t gl_lens_maps_vjp_workspace_bytes(const gl_model* m, int B, int64_t n_pts) {
  const long long n_blocks = vjp_blocks(m, B, n_pts);
  if (!n_blocks) return 0;
  return align_up((size_t)B * (size_t)std::max(m->lens_params, 1) * (size_t)n_blocks * sizeof(float), 256);
}

int gl_lens_maps_vjp(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts, int xy_batched,
                     const float* cot, float* grad_params, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !x || !y || !cot || !grad_params || !workspace) return fail(GL_EINVAL, "null argument");
  if (B <= 0 || n_pts <= 0) return fail(GL_EINVAL, "B and n_pts must be positive");
  if (int rc = refuse_vjp_lenses(m, "gl_lens_maps_vjp", "the ray-shoot VJP")) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const long long n_blocks = vjp_blocks(m, B, n_pts);
  if (!n_blocks) return fail(GL_EINVAL, "too many points x samples for one call");
  const size_t need = gl_lens_maps_vjp_workspace_bytes(m, B, n_pts);
  if (workspace_bytes < need) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
  launch_vjp(gl_lens_vjp_kernel, m, params, B, x, y, (long long)n_pts, xy_batched, cot, grad_params, (float*)workspace, n_blocks,
             (hipStream_t)hip_stream);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- VJP of the Hessian, reduced-shear likelihood (gl_hessian_vjp.hip.h) ------------------------------------------
namespace {
// the parts of the shear likelihood's workspace: block partials, cotangents [4][n_gal][B], the partials of the Hessian VJP
struct ShearLayout { size_t part, cot, vjp, bytes; long long n_blocks; };
bool shear_layout(const gl_model* m, int B, int n_gal, bool want_grad, ShearLayout* l) {
  if (!m || B <= 0 || n_gal <= 0) return false;
  l->n_blocks = ((long long)n_gal + VJP_PTS - 1) / VJP_PTS;
  if (l->n_blocks > 0x7fffffffLL / B) return false;
  l->part = 0;
  l->cot = l->part + align_up((size_t)B * (size_t)l->n_blocks * 2 * sizeof(float), 256);
  l->vjp = l->cot;
  l->bytes = l->cot;
  if (want_grad) {
    const size_t vjp = gl_lens_hessian_vjp_workspace_bytes(m, B, n_gal);
    if (!vjp) return false;
    l->vjp = l->cot + align_up((size_t)4 * (size_t)n_gal * (size_t)B * sizeof(float), 256);
    l->bytes = l->vjp + vjp;
  }
  return true;
}
}  // namespace

size_t gl_lens_hessian_vjp_workspace_bytes(const gl_model* m, int B, int64_t n_pts) {
  return gl_lens_maps_vjp_workspace_bytes(m, B, n_pts);  // one partial per (sample, lens column, block of points), as the ray-shoot VJP
}

int gl_lens_hessian_vjp(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts, int xy_batched,
                        const float* cot, float* grad_params, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !x || !y || !cot || !grad_params || !workspace) return fail(GL_EINVAL, "null argument");
  if (B <= 0 || n_pts <= 0) return fail(GL_EINVAL, "B and n_pts must be positive");
  if (int rc = refuse_vjp_lenses(m, "gl_lens_hessian_vjp", "the Hessian VJP")) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const long long n_blocks = vjp_blocks(m, B, n_pts);
  if (!n_blocks) return fail(GL_EINVAL, "too many points x samples for one call");
  const size_t need = gl_lens_hessian_vjp_workspace_bytes(m, B, n_pts);
  if (workspace_bytes < need) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
  launch_vjp(gl_hessian_vjp_kernel, m, params, B, x, y, (long long)n_pts, xy_batched, cot, grad_params, (float*)workspace, n_blocks,
             (hipStream_t)hip_stream);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

size_t gl_shear_loglike_workspace_bytes(const gl_model* m, int B, int n_gal, int want_grad) {
  ShearLayout lay;
  return shear_layout(m, B, n_gal, want_grad != 0, &lay) ? lay.bytes : 0;
}

int gl_shear_loglike(const gl_model* m, const float* params, int B, const float* x, const float* y, const float* scale_or_null,
                     const float* e1, const float* e2, const float* sigma, int n_gal, float* ll, float* chi2, float* model_g_or_null,
                     float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !x || !y || !e1 || !e2 || !sigma || !ll || !chi2 || !workspace) return fail(GL_EINVAL, "null argument");
  if (B <= 0 || n_gal <= 0) return fail(GL_EINVAL, "B and n_gal must be positive");
  if (int rc = refuse_vjp_lenses(m, "gl_shear_loglike", "the shear likelihood")) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const bool want_grad = grad_params_or_null != nullptr;
  ShearLayout lay;
  if (!shear_layout(m, B, n_gal, want_grad, &lay)) return fail(GL_EINVAL, "too many galaxies x samples for one call");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  ShearArgs s{};
  s.x = x;
  s.y = y;
  s.scale = scale_or_null;
  s.e1 = e1;
  s.e2 = e2;
  s.sigma = sigma;
  s.n_gal = n_gal;
  s.n_blocks = (int)lay.n_blocks;
  s.part = (float*)(base + lay.part);
  s.model_g = model_g_or_null;
  s.cot = want_grad ? (float*)(base + lay.cot) : nullptr;
  hipLaunchKernelGGL(gl_shear_fwd_kernel, dim3((unsigned)((long long)B * lay.n_blocks)), dim3(VJP_WG), 0, stream, point_args(m, params, B), s);
  hipLaunchKernelGGL(gl_shear_sum_kernel, dim3((unsigned)B), dim3(VJP_WG), 0, stream, (const float*)s.part, s.n_blocks, ll, chi2);
  if (want_grad)
    launch_vjp(gl_hessian_vjp_kernel, m, params, B, x, y, (long long)n_gal, 0, s.cot, grad_params_or_null, (float*)(base + lay.vjp),
               lay.n_blocks, stream);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- image-plane position likelihood of image families (gl_imgplane.hip.h) ------------------------------------------
namespace {
// the parts of the workspace: the point list [2][n_pts][B], u [2][J][B], chi2_j and the lost flags [J][B], the cotangents
// [2][n_pts][B] and the partials of the ray-shoot VJP (the last two with a gradient only)
struct ImgPlaneLayout { size_t pts, u, chi2_j, lost, cot, vjp, bytes; long long n_pts, n_blocks; };
bool imgplane_layout(const gl_model* m, int B, int J, bool with_source, bool want_grad, ImgPlaneLayout* l) {
  if (!m || B <= 0 || J <= 0) return false;
  l->n_pts = with_source ? (long long)J : 2LL * J;
  if ((l->n_pts * B + VJP_WG - 1) / VJP_WG > 0x7fffffffLL) return false;
  const size_t JB = (size_t)J * (size_t)B, NB = (size_t)l->n_pts * (size_t)B;
  l->pts = 0;
  l->u = l->pts + align_up(2 * NB * sizeof(float), 256);
  l->chi2_j = l->u + align_up(2 * JB * sizeof(float), 256);
  l->lost = l->chi2_j + align_up(JB * sizeof(float), 256);
  l->cot = l->lost + align_up(JB * sizeof(int), 256);
  l->vjp = l->cot;
  l->bytes = l->cot;
  l->n_blocks = 0;
  if (want_grad) {
    l->n_blocks = vjp_blocks(m, B, l->n_pts);
    if (!l->n_blocks) return false;
    l->vjp = l->cot + align_up(2 * NB * sizeof(float), 256);
    l->bytes = l->vjp + gl_lens_maps_vjp_workspace_bytes(m, B, l->n_pts);
  }
  return true;
}
}  // namespace

size_t gl_imgplane_loglike_workspace_bytes(const gl_model* m, int B, int n_images, int with_source, int want_grad) {
  ImgPlaneLayout lay;
  return imgplane_layout(m, B, n_images, with_source != 0, want_grad != 0, &lay) ? lay.bytes : 0;
}

int gl_imgplane_loglike(const gl_model* m, const float* params, int B, const float* image_table, const int32_t* family_table,
                        const int32_t* family_offsets_host, int n_images, int n_families, const float* source_or_null, float tol,
                        int max_iter, float* ll, float* chi2, int32_t* n_lost, float* pred_or_null, float* grad_params_or_null,
                        float* grad_source_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !image_table || !family_table || !family_offsets_host || !ll || !chi2 || !n_lost || !workspace)
    return fail(GL_EINVAL, "null argument");
  const int J = n_images, F = n_families;
  if (B <= 0 || J <= 0 || F <= 0) return fail(GL_EINVAL, "B, n_images and n_families must be positive");
  if (grad_source_or_null && !source_or_null) return fail(GL_EINVAL, "grad_source without explicit sources");
  if (family_offsets_host[0] != 0 || family_offsets_host[F] != J)
    return fail(GL_EINVAL, "family offsets run from %d to %d for %d image(s)", family_offsets_host[0], family_offsets_host[F], J);
  for (int f = 0; f < F; ++f) {
    const int n = family_offsets_host[f + 1] - family_offsets_host[f];
    if (n < 1) return fail(GL_EINVAL, "image family %d holds no image", f);
    if (n > IMGP_MAX_FAMILY) return fail(GL_EINVAL, "image family %d holds %d images: at most %d", f, n, IMGP_MAX_FAMILY);
    if (n == 1 && !source_or_null)
      return fail(GL_EINVAL, "image family %d holds one image: the barycentre source takes two or more (or give the sources)", f);
  }
  if (!(tol > 0.f) || max_iter < 1) return fail(GL_EINVAL, "tol must be > 0 and max_iter >= 1 (got %g, %d)", tol, max_iter);
  if (int rc = refuse_vjp_lenses(m, "gl_imgplane_loglike", "the image-plane position likelihood")) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const bool want_grad = grad_params_or_null != nullptr;
  ImgPlaneLayout lay;
  if (!imgplane_layout(m, B, J, source_or_null != nullptr, want_grad, &lay)) return fail(GL_EINVAL, "too many images x samples for one call");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  ImgPlaneArgs g{};
  g.tab = image_table;
  g.fam = family_table;
  g.source = source_or_null;
  g.J = J;
  g.F = F;
  g.max_iter = max_iter;
  g.tol = tol;
  g.pts = (float*)(base + lay.pts);
  g.u = (float*)(base + lay.u);
  g.chi2_j = (float*)(base + lay.chi2_j);
  g.lost = (int*)(base + lay.lost);
  g.cot = want_grad ? (float*)(base + lay.cot) : nullptr;
  g.n_pts = lay.n_pts;
  const PosArgs a = point_args(m, params, B);
  const size_t JB = (size_t)J * (size_t)B, NB = (size_t)lay.n_pts * (size_t)B;
  const dim3 newton_grid((unsigned)((JB + VJP_WG - 1) / VJP_WG));
  hipLaunchKernelGGL(gl_imgp_newton_kernel, newton_grid, dim3(VJP_WG), 0, stream, a, g);
  hipLaunchKernelGGL(gl_imgp_sum_kernel, dim3((unsigned)B), dim3(VJP_WG), 0, stream, g, B, ll, chi2, (int*)n_lost, grad_source_or_null);
  if (pred_or_null) {  // [2][J][B]: the first J points of the list, x then y
    GL_HIP(hipMemcpyAsync(pred_or_null, g.pts, JB * sizeof(float), hipMemcpyDeviceToDevice, stream));
    GL_HIP(hipMemcpyAsync(pred_or_null + JB, g.pts + NB, JB * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  if (want_grad) {
    hipLaunchKernelGGL(gl_imgp_cot_kernel, dim3((unsigned)((NB + VJP_WG - 1) / VJP_WG)), dim3(VJP_WG), 0, stream, g, B);
    launch_vjp(gl_lens_vjp_kernel, m, params, B, g.pts, g.pts + NB, lay.n_pts, 1, g.cot, grad_params_or_null, (float*)(base + lay.vjp),
               lay.n_blocks, stream);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- lensing potential (gl_potential.hip.h) --------------------------------------------------------------------
int gl_lens_potential(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts,
                      int xy_batched, float* out, void* hip_stream) {
  if (!m || !params || !out) return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_lens_potential")) return rp;
  if ((x == nullptr) != (y == nullptr)) return fail(GL_EINVAL, "x and y must both be given or both be null");
  if (B <= 0 || n_pts <= 0) return fail(GL_EINVAL, "B and n_pts must be positive");
  if (int rc = refuse_potential_lenses(m)) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  if (!x) {
    if (n_pts != m->N || xy_batched) return fail(GL_EINVAL, "the model grid has %d points and is not batched", m->N);
    x = m->d_gx;
    y = m->d_gy;
  }
  const long long total = (long long)n_pts * B, blocks = (total + POT_WG - 1) / POT_WG;
  if (blocks > 0x7fffffffLL) return fail(GL_EINVAL, "too many points x samples for one call");
  PosArgs a = point_args(m, params, B);
  hipLaunchKernelGGL(gl_lens_potential_kernel, dim3((unsigned)blocks), dim3(POT_WG), 0, (hipStream_t)hip_stream, a, x, y,
                     (long long)n_pts, xy_batched, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_profile_potential(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                         const float* params, float* out, void* hip_stream) {
  if (!comp || !x || !y || !params || !out) return fail(GL_EINVAL, "null argument");
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  if (comp->kind == GL_SCALED || comp->kind == GL_SERIES || comp->kind == GL_USER_MASS)
    return fail(GL_EUNSUPPORTED, "kind %d has no plugin-level potential (free-standing built-in mass kinds only; catalogues: "
                                 "gl_lens_potential on a model)", comp->kind);
  if (!potential_kind(comp->kind)) return fail(GL_EINVAL, "kind %d is not a free-standing mass profile", comp->kind);
  const long long total = (long long)n_pts * B, blocks = (total + POT_WG - 1) / POT_WG;
  if (blocks > 0x7fffffffLL) return fail(GL_EINVAL, "too many points x samples for one call");
  const CompDesc cd = point_comp(comp);
  hipLaunchKernelGGL(gl_profile_potential_kernel, dim3((unsigned)blocks), dim3(POT_WG), 0, (hipStream_t)hip_stream, cd, x, y,
                     (long long)n_pts, B, xy_batched, params, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- lens-equation solver (gl_images.hip.h) -----------------------------------------------------------------
size_t gl_image_positions_workspace_bytes(const gl_model* m, int B, int n_src, int n_cells, int max_images) {
  if (!m || B <= 0 || n_src <= 0 || n_cells <= 0 || n_cells > IMG_MAX_CELLS || max_images < 1) return 0;
  return img_layout(B, n_src, n_cells).bytes;
}

int gl_image_positions(const gl_model* m, const float* params, int B, const float* src_x, const float* src_y, int n_src,
                       float x_lo, float x_hi, float y_lo, float y_hi, int n_cells, int max_images, float tol, int max_iter,
                       float* out, int* n_images, int* n_dropped, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return gl_image_positions_scaled(m, params, B, src_x, src_y, n_src, nullptr, x_lo, x_hi, y_lo, y_hi, n_cells, max_images, tol,
                                   max_iter, out, n_images, n_dropped, workspace, workspace_bytes, hip_stream);
}

int gl_image_positions_scaled(const gl_model* m, const float* params, int B, const float* src_x, const float* src_y, int n_src,
                              const float* src_scale, float x_lo, float x_hi, float y_lo, float y_hi, int n_cells, int max_images,
                              float tol, int max_iter, float* out, int* n_images, int* n_dropped, void* workspace,
                              size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !src_x || !src_y || !out || !n_images || !n_dropped) return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_image_positions")) return rp;
  if (B <= 0 || n_src <= 0) return fail(GL_EINVAL, "B (%d) and n_src (%d) must be positive", B, n_src);
  if (n_cells <= 0 || n_cells > IMG_MAX_CELLS) return fail(GL_EINVAL, "n_cells %d outside [1, %d]", n_cells, IMG_MAX_CELLS);
  if (max_images < 1 || max_images > IMG_MAXC) return fail(GL_EINVAL, "max_images %d outside [1, %d]", max_images, IMG_MAXC);
  if (int rc = check_window(true, x_lo, x_hi, y_lo, y_hi)) return rc;
  if (!(tol > 0.f) || max_iter < 1) return fail(GL_EINVAL, "tol must be > 0 and max_iter >= 1 (got %g, %d)", tol, max_iter);
  if (m->n_series)
    return fail(GL_EUNSUPPORTED, "a series-expansion lens lives on the pixel grid only (series_profile.py:76-81): no image finder");
  if (int rc = check_ready(m, false, false)) return rc;
  const ImgLayout lay = img_layout(B, n_src, n_cells);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  const long long V = (long long)(n_cells + 1) * (n_cells + 1);
  const long long map_blocks = (V * B + 255) / 256, pairs = (long long)B * n_src;
  if (map_blocks > 0x7fffffffLL || pairs > 0x7fffffffLL) return fail(GL_EINVAL, "too many samples / vertices / sources for one call");
  if (m->has_user)  // map and Newton kernels compiled at run time with the user's bodies (the scan does not touch the lens)
    if (int rc = compile_user_points(m)) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  PosArgs a = point_args(m, params, B);
  ImgArgs g{};
  if (src_scale) {  // one scale per source, host -> the call's own workspace on the caller's stream (all 1: the unscaled path)
    bool any;
    if (int rc = check_scales(src_scale, n_src, n_src, "source(s)", &any)) return rc;
    if (any) {
      float* d_scale = (float*)((char*)workspace + lay.scale);
      GL_HIP(hipMemcpyAsync(d_scale, src_scale, sizeof(float) * (size_t)n_src, hipMemcpyHostToDevice, stream));
      g.src_scale = d_scale;
    }
  }
  g.src_x = src_x;
  g.src_y = src_y;
  g.S = n_src;
  g.n = n_cells;
  g.x_lo = x_lo; g.x_hi = x_hi; g.y_lo = y_lo; g.y_hi = y_hi;
  g.hx = (x_hi - x_lo) / (float)n_cells;
  g.hy = (y_hi - y_lo) / (float)n_cells;
  g.max_images = max_images;
  g.max_iter = max_iter;
  g.tol = tol;
  char* base = (char*)workspace;
  g.map = (float2*)(base + lay.map);
  g.cand = (float2*)(base + lay.cand);
  g.n_cand = (int*)(base + lay.n_cand);
  g.n_over = (int*)(base + lay.n_over);
  g.out = out;
  g.n_images = n_images;
  g.n_dropped = n_dropped;
  if (m->has_user) {
    void* args[] = {&a, &g};
    GL_HIP(hipModuleLaunchKernel(m->user_point_fn[5], (unsigned)map_blocks, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
  } else if (m->n_interp_mass || m->n_multipole) {  // (the build that carries the interpolated lens and the multipole: gl_images.hip.h)
    hipLaunchKernelGGL(gl_img_map_im_kernel, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  } else {
    hipLaunchKernelGGL(gl_img_map_kernel, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  }
  hipLaunchKernelGGL(gl_img_scan_kernel, dim3((unsigned)pairs), dim3(IMG_SCAN_WG), 0, stream, g);
  if (m->has_user) {
    void* args[] = {&a, &g};
    GL_HIP(hipModuleLaunchKernel(m->user_point_fn[6], (unsigned)pairs, 1, 1, 64, 1, 1, 0, stream, args, nullptr));
  } else if (m->n_interp_mass || m->n_multipole) {
    hipLaunchKernelGGL(gl_img_newton_im_kernel, dim3((unsigned)pairs), dim3(64), 0, stream, a, g);
  } else {
    hipLaunchKernelGGL(gl_img_newton_kernel, dim3((unsigned)pairs), dim3(64), 0, stream, a, g);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// read-only: the scan stage's two planes out of a workspace the solver has just filled (same layout arguments, same stream)
int gl_image_positions_stage_counts(const gl_model* m, int B, int n_src, int n_cells, const void* workspace, size_t workspace_bytes,
                                    int* n_cand, int* n_over, void* hip_stream) {
  if (!m || !workspace || !n_cand || !n_over) return fail(GL_EINVAL, "null argument");
  // (a workspace of the solver on lens planes holds K maps in front of the counts: gl_multiplane_image_positions_stage_counts)
  if (int rp = refuse_planes(m, "gl_image_positions_stage_counts")) return rp;
  if (int rc = check_stage_counts_sizes(B, n_src, n_cells)) return rc;
  const ImgLayout lay = img_layout(B, n_src, n_cells);
  return copy_stage_counts(lay, lay.bytes, workspace, workspace_bytes, B, n_src, n_cand, n_over, hip_stream);
}

// ---- ... on lens planes (gl_multiplane_images.hip.h) -----------------------------------------------------------
size_t gl_multiplane_image_positions_workspace_bytes(const gl_model* m, int B, int n_src, int n_cells, int max_images) {
  if (!m || m->mp_K < 2 || B <= 0 || n_src <= 0 || n_cells <= 0 || n_cells > IMG_MAX_CELLS || max_images < 1) return 0;
  return mp_img_layout(B, n_src, n_cells, m->mp_K).bytes;
}

int gl_multiplane_image_positions(const gl_model* m, const float* params, int B, const float* src_x, const float* src_y, int n_src,
                                  const float* targets, int n_planes, float x_lo, float x_hi, float y_lo, float y_hi, int n_cells,
                                  int max_images, float tol, int max_iter, float* out, int* n_images, int* n_dropped, void* workspace,
                                  size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !src_x || !src_y || !targets || !out || !n_images || !n_dropped) return fail(GL_EINVAL, "null argument");
  if (int rc = check_planes_set(m)) return rc;
  if (B <= 0 || n_src <= 0) return fail(GL_EINVAL, "B (%d) and n_src (%d) must be positive", B, n_src);
  if (n_planes != m->mp_K) return fail(GL_EINVAL, "%d target couplings per source for %d lens planes", n_planes, m->mp_K);
  if (n_cells <= 0 || n_cells > IMG_MAX_CELLS) return fail(GL_EINVAL, "n_cells %d outside [1, %d]", n_cells, IMG_MAX_CELLS);
  if (max_images < 1 || max_images > IMG_MAXC) return fail(GL_EINVAL, "max_images %d outside [1, %d]", max_images, IMG_MAXC);
  if (int rc = check_window(true, x_lo, x_hi, y_lo, y_hi)) return rc;
  if (!(tol > 0.f) || max_iter < 1) return fail(GL_EINVAL, "tol must be > 0 and max_iter >= 1 (got %g, %d)", tol, max_iter);
  const int K = n_planes;
  if (int rc = check_target_rows(targets, n_src, K)) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const MpImgLayout lay = mp_img_layout(B, n_src, n_cells, K);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  const long long V = (long long)(n_cells + 1) * (n_cells + 1);
  const long long map_blocks = (V * B + 255) / 256, pairs = (long long)B * n_src;
  if (map_blocks > 0x7fffffffLL || pairs > 0x7fffffffLL) return fail(GL_EINVAL, "too many samples / vertices / sources for one call");
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  // the coupling rows, host -> the call's own workspace on the caller's stream (as the scales of gl_image_positions_scaled)
  float* d_tgt = (float*)(base + lay.tgt);
  GL_HIP(hipMemcpyAsync(d_tgt, targets, sizeof(float) * (size_t)n_src * (size_t)K, hipMemcpyHostToDevice, stream));
  PosArgs a = point_args(m, params, B);
  const MpArgs mp = mp_args(m);
  ImgArgs g{};
  g.src_x = src_x;
  g.src_y = src_y;
  g.S = n_src;
  g.n = n_cells;
  g.x_lo = x_lo; g.x_hi = x_hi; g.y_lo = y_lo; g.y_hi = y_hi;
  g.hx = (x_hi - x_lo) / (float)n_cells;
  g.hy = (y_hi - y_lo) / (float)n_cells;
  g.max_images = max_images;
  g.max_iter = max_iter;
  g.tol = tol;
  g.cand = (float2*)(base + lay.img.cand);
  g.n_cand = (int*)(base + lay.img.n_cand);
  g.n_over = (int*)(base + lay.img.n_over);
  g.out = out;
  g.n_images = n_images;
  g.n_dropped = n_dropped;
  MpImgArgs q{};
  q.tgt = d_tgt;
  q.K = K;
  q.pmap = (float2*)(base + lay.img.map);
  hipLaunchKernelGGL(gl_mpimg_map_kernel, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, mp, g, q);
  hipLaunchKernelGGL(gl_mpimg_scan_kernel, dim3((unsigned)pairs), dim3(IMG_SCAN_WG), 0, stream, g, q);
  hipLaunchKernelGGL(gl_mpimg_newton_kernel, dim3((unsigned)pairs), dim3(MP_MAPS_WG), 0, stream, a, mp, g, q);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// read-only, as gl_image_positions_stage_counts: the counts lie behind the K maps of the model's planes
int gl_multiplane_image_positions_stage_counts(const gl_model* m, int B, int n_src, int n_cells, const void* workspace,
                                               size_t workspace_bytes, int* n_cand, int* n_over, void* hip_stream) {
  if (!m || !workspace || !n_cand || !n_over) return fail(GL_EINVAL, "null argument");
  if (int rc = check_planes_set(m)) return rc;
  if (int rc = check_stage_counts_sizes(B, n_src, n_cells)) return rc;
  const MpImgLayout lay = mp_img_layout(B, n_src, n_cells, m->mp_K);
  return copy_stage_counts(lay.img, lay.bytes, workspace, workspace_bytes, B, n_src, n_cand, n_over, hip_stream);
}

// ---- arrival times on lens planes (gl_multiplane_fermat.hip.h) ----------------------------------------------------
size_t gl_multiplane_fermat_workspace_bytes(const gl_model* m, int n_src) {
  if (!m || m->mp_K < 2 || n_src <= 0) return 0;
  return mp_fermat_layout(n_src, m->mp_K).bytes;
}

int gl_multiplane_fermat(const gl_model* m, const float* params, int B, const float* x, const float* y, const float* src_x,
                         const float* src_y, int n_src, int n_points, const double* geom, const double* pot, int n_planes,
                         double* out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !x || !y || !src_x || !src_y || !geom || !pot || !out) return fail(GL_EINVAL, "null argument");
  if (int rc = check_planes_set(m)) return rc;
  if (B <= 0 || n_src <= 0 || n_points <= 0)
    return fail(GL_EINVAL, "B (%d), n_src (%d) and n_points (%d) must be positive", B, n_src, n_points);
  if (n_planes != m->mp_K) return fail(GL_EINVAL, "%d delay weights per source for %d lens planes", n_planes, m->mp_K);
  const int K = n_planes;
  for (int i = 0; i < K; ++i)
    if (!(std::isfinite(pot[i]) && pot[i] >= 0.)) return fail(GL_EINVAL, "pot[%d] = %g: finite and >= 0", i, pot[i]);
  for (int s = 0; s < n_src; ++s) {  // a row of MultiPlane.delay_weights: the zeros are those of the source's coupling row
    const double* g = geom + (size_t)s * K;
    for (int i = 0; i < K; ++i)
      if (!(std::isfinite(g[i]) && g[i] >= 0.) || (i > 0 && g[i] != 0. && g[i - 1] == 0.))
        return fail(GL_EINVAL, "geom[%d][%d] = %g: finite and >= 0, 0 from the first plane at or behind the source on", s, i, g[i]);
    if (g[0] == 0.) return fail(GL_EINVAL, "source %d: every geometric weight is zero (the source lies behind no lens plane)", s);
  }
  if (int rc = refuse_potential_lenses(m)) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const MpFermatLayout lay = mp_fermat_layout(n_src, K);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_EINVAL, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  const long long total = (long long)B * n_src * n_points, blocks = (total + MP_FERMAT_WG - 1) / MP_FERMAT_WG;
  if (blocks > 0x7fffffffLL) return fail(GL_EINVAL, "too many samples x sources x points for one call");
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  // the weight rows, host -> the call's own workspace on the caller's stream (as the coupling rows of the solver)
  double* d_geom = (double*)(base + lay.geom);
  double* d_pot = (double*)(base + lay.pot);
  GL_HIP(hipMemcpyAsync(d_geom, geom, sizeof(double) * (size_t)n_src * (size_t)K, hipMemcpyHostToDevice, stream));
  GL_HIP(hipMemcpyAsync(d_pot, pot, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, stream));
  MpFermatArgs q{};
  q.x = x;
  q.y = y;
  q.src_x = src_x;
  q.src_y = src_y;
  q.geom = d_geom;
  q.pot = d_pot;
  q.n_src = n_src;
  q.M = n_points;
  q.K = K;
  q.out = out;
  hipLaunchKernelGGL(gl_mp_fermat_kernel, dim3((unsigned)blocks), dim3(MP_FERMAT_WG), 0, stream, point_args(m, params, B), mp_args(m), q);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- critical curves and caustics (gl_critical.hip.h) ----------------------------------------------------------
size_t gl_critical_curves_workspace_bytes(const gl_model* m, int B, int n_cells, int max_segments) {
  if (!m || B <= 0 || n_cells <= 0 || n_cells > IMG_MAX_CELLS || max_segments < 1 || max_segments > CRIT_MAX_SEGMENTS) return 0;
  return crit_layout(B, n_cells, max_segments).bytes;
}

int gl_critical_curves(const gl_model* m, const float* params, int B, float x_lo, float x_hi, float y_lo, float y_hi, int n_cells,
                       int max_segments, float* seg, float* cau, int* kind, int* n_seg, int* n_dropped, int* n_flagged, int* open,
                       float* area, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return gl_critical_curves_scaled(m, params, B, x_lo, x_hi, y_lo, y_hi, n_cells, max_segments, 1.f, seg, cau, kind, n_seg, n_dropped,
                                   n_flagged, open, area, workspace, workspace_bytes, hip_stream);
}

int gl_critical_curves_scaled(const gl_model* m, const float* params, int B, float x_lo, float x_hi, float y_lo, float y_hi,
                              int n_cells, int max_segments, float scale, float* seg, float* cau, int* kind, int* n_seg,
                              int* n_dropped, int* n_flagged, int* open, float* area, void* workspace, size_t workspace_bytes,
                              void* hip_stream) {
  if (!m || !params || !seg || !cau || !kind || !n_seg || !n_dropped || !n_flagged || !open || !area)
    return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_critical_curves")) return rp;
  if (!(std::isfinite(scale) && scale > 0.f)) return fail(GL_EINVAL, "scale (%g) is not finite and > 0", scale);
  if (B <= 0) return fail(GL_EINVAL, "B (%d) must be positive", B);
  if (n_cells <= 0 || n_cells > IMG_MAX_CELLS) return fail(GL_EINVAL, "n_cells %d outside [1, %d]", n_cells, IMG_MAX_CELLS);
  if (max_segments < 1 || max_segments > CRIT_MAX_SEGMENTS)
    return fail(GL_EINVAL, "max_segments %d outside [1, %d]", max_segments, CRIT_MAX_SEGMENTS);
  if (int rc = check_window(false, x_lo, x_hi, y_lo, y_hi)) return rc;
  if (m->n_series)
    return fail(GL_EUNSUPPORTED, "a series-expansion lens lives on the pixel grid only (series_profile.py:76-81): no critical curves");
  if (m->has_user)
    return fail(GL_EUNSUPPORTED, "user-written bodies (and the run-time compiled ScalingRelation member loops) are not served by the "
                                 "critical-curve kernels");
  if (int rc = check_ready(m, false, false)) return rc;
  const CritLayout lay = crit_layout(B, n_cells, max_segments);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  const long long V = (long long)(n_cells + 1) * (n_cells + 1);
  const long long map_blocks = (V * B + 255) / 256;
  const int max_edges = 2 * max_segments;
  const long long refine_blocks = (long long)B * ((max_edges + 63) / 64);
  if (map_blocks > 0x7fffffffLL || refine_blocks > 0x7fffffffLL)
    return fail(GL_EINVAL, "too many samples x vertices (or x max_segments) for one call");
  hipStream_t stream = (hipStream_t)hip_stream;
  PosArgs a = point_args(m, params, B);
  CritArgs g{};
  g.n = n_cells;
  g.scale = scale;
  g.max_segments = max_segments;
  g.max_edges = max_edges;
  g.x_lo = x_lo; g.x_hi = x_hi; g.y_lo = y_lo; g.y_hi = y_hi;
  g.hx = (x_hi - x_lo) / (float)n_cells;
  g.hy = (y_hi - y_lo) / (float)n_cells;
  g.bracket = CRIT_BRACKET_ULP * std::numeric_limits<float>::epsilon() *
              std::max(std::max(std::fabs(x_lo), std::fabs(x_hi)), std::max(std::fabs(y_lo), std::fabs(y_hi)));
  char* base = (char*)workspace;
  g.dmap = (float*)(base + lay.dmap);
  g.edge_id = (int*)(base + lay.edge_id);
  g.edge_pt = (float4*)(base + lay.edge_pt);
  g.edge_omk = (float*)(base + lay.edge_omk);
  g.n_edges = (int*)(base + lay.n_edges);
  g.n_edge_over = (int*)(base + lay.n_edge_over);
  g.seg = seg; g.cau = cau; g.kind = kind;
  g.n_seg = n_seg; g.n_dropped = n_dropped; g.n_flagged = n_flagged; g.open = open;
  g.area = area;
  // catalogues and interpolated lenses take the build whose evaluation is a function call (gl_critical.hip.h, crit_eval)
  const bool cat = m->n_scaled > 0 || m->n_interp_mass > 0 || m->n_multipole > 0;
  if (cat) hipLaunchKernelGGL(gl_crit_map_kernel<true>, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  else hipLaunchKernelGGL(gl_crit_map_kernel<false>, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  hipLaunchKernelGGL(gl_crit_scan_kernel, dim3((unsigned)B), dim3(CRIT_WG), 0, stream, g);
  if (cat) hipLaunchKernelGGL(gl_crit_refine_kernel<true>, dim3((unsigned)refine_blocks), dim3(64), 0, stream, a, g);
  else hipLaunchKernelGGL(gl_crit_refine_kernel<false>, dim3((unsigned)refine_blocks), dim3(64), 0, stream, a, g);
  hipLaunchKernelGGL(gl_crit_cells_kernel, dim3((unsigned)B), dim3(CRIT_WG), 0, stream, g);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- ... on lens planes (gl_multiplane_critical.hip.h) ------------------------------------------------------------
size_t gl_multiplane_critical_curves_workspace_bytes(const gl_model* m, int B, int n_src, int n_cells, int max_segments) {
  if (!m || m->mp_K < 2 || B <= 0 || n_src <= 0 || n_cells <= 0 || n_cells > IMG_MAX_CELLS || max_segments < 1 ||
      max_segments > CRIT_MAX_SEGMENTS || (long long)B * n_src > 0x7fffffffLL)
    return 0;
  return mp_crit_layout(B, n_src, n_cells, max_segments, m->mp_K).bytes;
}

int gl_multiplane_critical_curves(const gl_model* m, const float* params, int B, const float* targets, int n_src, int n_planes,
                                  float x_lo, float x_hi, float y_lo, float y_hi, int n_cells, int max_segments, float* seg, float* cau,
                                  int* kind, int* n_seg, int* n_dropped, int* n_flagged, int* open, float* area, void* workspace,
                                  size_t workspace_bytes, void* hip_stream) {
  if (!m || !params || !targets || !seg || !cau || !kind || !n_seg || !n_dropped || !n_flagged || !open || !area)
    return fail(GL_EINVAL, "null argument");
  if (int rc = check_planes_set(m)) return rc;
  if (B <= 0 || n_src <= 0) return fail(GL_EINVAL, "B (%d) and n_src (%d) must be positive", B, n_src);
  if (n_planes != m->mp_K) return fail(GL_EINVAL, "%d target couplings per source for %d lens planes", n_planes, m->mp_K);
  if (n_cells <= 0 || n_cells > IMG_MAX_CELLS) return fail(GL_EINVAL, "n_cells %d outside [1, %d]", n_cells, IMG_MAX_CELLS);
  if (max_segments < 1 || max_segments > CRIT_MAX_SEGMENTS)
    return fail(GL_EINVAL, "max_segments %d outside [1, %d]", max_segments, CRIT_MAX_SEGMENTS);
  if (int rc = check_window(false, x_lo, x_hi, y_lo, y_hi)) return rc;
  const int K = n_planes;
  if (int rc = check_target_rows(targets, n_src, K)) return rc;
  if (int rc = check_ready(m, false, false)) return rc;
  const long long V = (long long)(n_cells + 1) * (n_cells + 1), rows = (long long)B * n_src;
  const long long map_blocks = (V * B + MP_MAPS_WG - 1) / MP_MAPS_WG;
  const int max_edges = 2 * max_segments;
  const long long refine_blocks = rows * ((max_edges + 63) / 64);
  if (map_blocks > 0x7fffffffLL || rows > 0x7fffffffLL || refine_blocks > 0x7fffffffLL)
    return fail(GL_EINVAL, "too many samples x vertices (or x sources x max_segments) for one call");
  const MpCritLayout lay = mp_crit_layout(B, n_src, n_cells, max_segments, K);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  // the coupling rows, host -> the call's own workspace on the caller's stream (as in gl_multiplane_image_positions)
  float* d_tgt = (float*)(base + lay.tgt);
  GL_HIP(hipMemcpyAsync(d_tgt, targets, sizeof(float) * (size_t)n_src * (size_t)K, hipMemcpyHostToDevice, stream));
  PosArgs a = point_args(m, params, B);
  const MpArgs mp = mp_args(m);
  CritArgs g{};  // every array [B n_src][...]: row b n_src + s is the "sample" of the scan and cells kernels
  g.n = n_cells;
  g.scale = 1.f;  // (not read: the couplings carry the scales)
  g.max_segments = max_segments;
  g.max_edges = max_edges;
  g.x_lo = x_lo; g.x_hi = x_hi; g.y_lo = y_lo; g.y_hi = y_hi;
  g.hx = (x_hi - x_lo) / (float)n_cells;
  g.hy = (y_hi - y_lo) / (float)n_cells;
  g.bracket = CRIT_BRACKET_ULP * std::numeric_limits<float>::epsilon() *
              std::max(std::max(std::fabs(x_lo), std::fabs(x_hi)), std::max(std::fabs(y_lo), std::fabs(y_hi)));
  g.dmap = (float*)(base + lay.crit.dmap);
  g.edge_id = (int*)(base + lay.crit.edge_id);
  g.edge_pt = (float4*)(base + lay.crit.edge_pt);
  g.edge_omk = (float*)(base + lay.crit.edge_omk);
  g.n_edges = (int*)(base + lay.crit.n_edges);
  g.n_edge_over = (int*)(base + lay.crit.n_edge_over);
  g.seg = seg; g.cau = cau; g.kind = kind;
  g.n_seg = n_seg; g.n_dropped = n_dropped; g.n_flagged = n_flagged; g.open = open;
  g.area = area;
  MpCritArgs q{};
  q.tgt = d_tgt;
  q.K = K;
  q.S = n_src;
  hipLaunchKernelGGL(gl_mpcrit_map_kernel, dim3((unsigned)map_blocks), dim3(MP_MAPS_WG), 0, stream, a, mp, g, q);
  hipLaunchKernelGGL(gl_crit_scan_kernel, dim3((unsigned)rows), dim3(CRIT_WG), 0, stream, g);
  hipLaunchKernelGGL(gl_mpcrit_refine_kernel, dim3((unsigned)refine_blocks), dim3(MP_MAPS_WG), 0, stream, a, mp, g, q);
  hipLaunchKernelGGL(gl_crit_cells_kernel, dim3((unsigned)rows), dim3(CRIT_WG), 0, stream, g);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"

// ---- lens planes at redshifts of their own (gl_multiplane.hip.h, gl_multiplane_bwd.hip.h) ------------------------------
namespace glk {

int mp_render(const gl_model* m, const float* params, int B, unsigned parts, float* img, const Workspace& w, hipStream_t stream) {
  MpRender r{};
  r.gx = m->d_gx;
  r.gy = m->d_gy;
  r.pix = m->d_pix;
  r.N = m->N;
  r.n_ll = m->n_ll;
  r.n_src = m->n_src;
  r.parts = parts;
  r.img_stride = (long long)m->height * m->width;
  r.img = m->has_post ? w.img_ss : img;
  r.out_scale = m->has_post ? 1.f : m->conversion_factor;  // (with a PSF the det(T) scale is applied after pooling, as in render_ss)
  if (m->d_pix) GL_HIP(hipMemsetAsync(r.img, 0, sizeof(float) * (size_t)B * m->height * m->width, stream));
  hipLaunchKernelGGL(gl_mp_render_kernel, dim3((unsigned)((m->N + MP_WG - 1) / MP_WG), (unsigned)B), dim3(MP_WG), 0, stream,
                     point_args(m, params, B), mp_args(m), r);
  GL_HIP(hipGetLastError());
  return m->has_post ? post_fwd(m, B, w.img_ss, img, stream, m->conversion_factor) : GL_OK;
}

int mp_render_bwd(const gl_model* m, int B, const LaunchPlan& plan, const Workspace& w, const float* gimg, float out_scale,
                  hipStream_t stream) {
  MpBwd r{};
  r.comps = m->d_comps;
  r.n_lens = m->n_lens;
  r.n_ll = m->n_ll;
  r.n_src = m->n_src;
  r.derived = w.derived;
  r.D = m->D;
  r.A = m->A;
  r.Apad = m->Apad;
  r.ncols = m->ncols;
  r.gx = m->d_gx;
  r.gy = m->d_gy;
  r.pix = m->d_pix;
  r.N = m->N;
  r.chunk = plan.chunk;
  r.gimg = gimg;
  r.img_stride = (long long)m->height * m->width;
  r.out_scale = out_scale;
  r.partial = w.partial;
  bool xf = false;  // the instantiation that carries the NFW_ELLIPSE / TNFW / CoreSersic VJPs
  for (const CompDesc& c : m->comps) xf = xf || c.kind == K_NFW_ELLIPSE || c.kind == K_TNFW || c.kind == K_CORE_SERSIC || c.kind == K_MULTIPOLE;
  const size_t shmem = (size_t)(((m->D + 3) & ~3) + m->ncols * m->Apad) * sizeof(float);
  const dim3 grid((unsigned)plan.n_chunks, (unsigned)B), block(MP_WG);
  if (xf) hipLaunchKernelGGL(gl_mp_bwd_kernel<true>, grid, block, shmem, stream, mp_args(m), r);
  else hipLaunchKernelGGL(gl_mp_bwd_kernel<false>, grid, block, shmem, stream, mp_args(m), r);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // namespace glk

extern "C" {

int gl_model_set_lens_planes(gl_model* m, const int* plane_of_lens, int n_lens, int n_planes, const float* lens_scales,
                             const float* source_scales, int n_src) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (n_planes > MP_MAXK) return fail(GL_EUNSUPPORTED, "%d lens planes: at most %d are served", n_planes, MP_MAXK);
  if (n_planes < 2) return fail(GL_EINVAL, "%d lens plane(s): two or more (one plane: gl_model_set_source_scales)", n_planes);
  if (!plane_of_lens || !lens_scales || (!source_scales && n_src > 0)) return fail(GL_EINVAL, "null argument");
  if (n_lens != m->n_lens) return fail(GL_EINVAL, "%d plane indices for %d lens(es)", n_lens, m->n_lens);
  if (n_src != m->n_src) return fail(GL_EINVAL, "source couplings of %d source(s) for %d source light component(s)", n_src, m->n_src);
  const int K = n_planes;
  if (m->has_user) return fail(GL_EUNSUPPORTED, "lens planes are not served for models with user-written profiles");
  if (m->n_series)
    return fail(GL_EUNSUPPORTED, "a series-expansion lens stores its field on the image-plane grid theta, not on the ray's position "
                                 "theta_j on its own plane: not served on lens planes");
  if (m->pos_n_delay)
    return fail(GL_EUNSUPPORTED, "the model holds arrival times (gl_model_set_position_delays): the time-delay term is not served on "
                                 "lens planes");
  if (m->src_scaled) return fail(GL_EINVAL, "the model carries per-source deflection scales (gl_model_set_source_scales): the source couplings of the planes replace them");
  for (int l = 0; l < m->n_lens; ++l)
    if (m->comps[l].kind == K_SCALED)
      return fail(GL_EUNSUPPORTED, "lens %d: galaxy catalogues (GL_SCALED) are not served on lens planes", l);
  for (int l = 0; l < m->n_lens; ++l)
    if (m->comps[l].kind == K_INTERPOL_MASS)
      return fail(GL_EUNSUPPORTED, "lens %d: an interpolated lens (GL_INTERPOL_MASS) is not served on lens planes", l);
  for (int c = m->n_lens; c < (int)m->comps.size(); ++c) {
    const int kind = m->comps[c].kind;
    if (kind != K_SERSIC && kind != K_SERSIC_ELLIPSE && kind != K_CORE_SERSIC)
      return fail(GL_EUNSUPPORTED, "light component %d (kind %d): lens planes serve Sersic, SersicEllipse and CoreSersic lights", c, kind);
  }
  std::vector<int> count(K, 0);
  for (int l = 0; l < n_lens; ++l) {
    if (plane_of_lens[l] < 0 || plane_of_lens[l] >= K) return fail(GL_EINVAL, "plane_of_lens[%d] = %d outside [0, %d)", l, plane_of_lens[l], K);
    ++count[plane_of_lens[l]];
  }
  for (int i = 0; i < K; ++i)
    if (!count[i]) return fail(GL_EINVAL, "lens plane %d holds no lens", i);
  std::vector<float> scale((size_t)MP_MAXK * MP_MAXK + (size_t)MP_MAXK * std::max(n_src, 0), 0.f);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) {
      const float c = lens_scales[i * K + j];
      if (i >= j ? c != 0.f : !(std::isfinite(c) && c > 0.f))
        return fail(GL_EINVAL, "lens_scales[%d][%d] = %g: strictly upper triangular, finite and > 0 above the diagonal", i, j, c);
      scale[(size_t)i * MP_MAXK + j] = c;
    }
  for (int s = 0; s < n_src; ++s)
    for (int i = 0; i < K; ++i) {
      const float c = source_scales[(size_t)i * n_src + s];
      // a plane at or behind a source does not deflect it: zero from that plane on; the first plane lies in front of every source
      const bool ok = std::isfinite(c) && c >= 0.f && (i == 0 ? c > 0.f : (c == 0.f || source_scales[(size_t)(i - 1) * n_src + s] > 0.f));
      if (!ok) return fail(GL_EINVAL, "source_scales[%d][%d] = %g: finite, > 0 on the first plane, 0 from the first plane behind the source on", i, s, c);
      scale[(size_t)MP_MAXK * MP_MAXK + (size_t)i * n_src + s] = c;
    }
  std::vector<int> lens((size_t)2 * std::max(n_lens, 1));
  int t = 0;
  for (int i = 0; i < K; ++i)
    for (int l = 0; l < n_lens; ++l)
      if (plane_of_lens[l] == i) lens[t++] = l;
  for (int l = 0; l < n_lens; ++l) lens[(size_t)n_lens + l] = plane_of_lens[l];
  GL_HIP(m->d_mp_lens.upload(lens.data(), lens.size()));
  GL_HIP(m->d_mp_scale.upload(scale.data(), scale.size()));
  m->mp_K = K;
  m->pos_targets = false;  // new planes: the couplings of the image families are given again
  m->d_pos_target.reset();
  m->pos_target_rows.clear();
  m->clear_plane_delays();  // ... and with them the arrival times of gl_model_set_position_plane_delays
  return GL_OK;
}

int gl_model_set_position_targets(gl_model* m, const float* targets, int n_families, int n_planes) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (int rc = check_planes_set(m)) return rc;
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if (!targets) return fail(GL_EINVAL, "targets is null");
  if (n_families != m->pos_F || n_planes != m->mp_K)
    return fail(GL_EINVAL, "target couplings [%d][%d] for %d image famil(ies) and %d lens planes", n_families, n_planes, m->pos_F, m->mp_K);
  std::vector<float> per_image((size_t)m->pos_J * MP_MAXK, 0.f);
  for (int f = 0; f < n_families; ++f) {
    const float* T = targets + (size_t)f * n_planes;
    for (int i = 0; i < n_planes; ++i)
      if (!(std::isfinite(T[i]) && T[i] >= 0.f) || (i > 0 && T[i] != 0.f && T[i - 1] == 0.f))
        return fail(GL_EINVAL, "targets[%d][%d] = %g: finite and >= 0, 0 from the first plane at or behind the family on", f, i, T[i]);
    if (T[0] == 0.f) return fail(GL_EINVAL, "image family %d: every coupling is zero (the family lies behind no lens plane)", f);
    for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) std::copy(T, T + n_planes, per_image.begin() + (size_t)j * MP_MAXK);
  }
  GL_HIP(m->d_pos_target.upload(per_image.data(), per_image.size()));
  m->pos_targets = true;
  m->pos_target_rows.assign(targets, targets + (size_t)n_families * n_planes);
  m->clear_plane_delays();  // new couplings: the arrival times of gl_model_set_position_plane_delays are given again
  return GL_OK;
}

int gl_multiplane_maps(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts, int xy_batched,
                       const float* target_scales, int n_planes, float* out, void* hip_stream) {
  if (!m || !params || !x || !y || !target_scales || !out) return fail(GL_EINVAL, "null argument");
  if (int rc = check_planes_set(m)) return rc;
  if (B <= 0 || n_pts <= 0) return fail(GL_EINVAL, "B and n_pts must be positive");
  if (n_planes != m->mp_K) return fail(GL_EINVAL, "%d target couplings for %d lens planes", n_planes, m->mp_K);
  if (int rc = check_ready(m, false, false)) return rc;
  MpTarget tg{};
  for (int i = 0; i < n_planes; ++i) {
    const float c = target_scales[i];
    if (!(std::isfinite(c) && c >= 0.f) || (i > 0 && c != 0.f && target_scales[i - 1] == 0.f))
      return fail(GL_EINVAL, "target_scales[%d] = %g: finite and >= 0, 0 from the first plane at or behind the target on", i, c);
    tg.c[i] = c;
  }
  const long long total = (long long)n_pts * B, blocks = (total + MP_MAPS_WG - 1) / MP_MAPS_WG;
  if (blocks > 0x7fffffffLL) return fail(GL_EINVAL, "too many points x samples for one call");
  hipLaunchKernelGGL(gl_mp_maps_kernel, dim3((unsigned)blocks), dim3(MP_MAPS_WG), 0, (hipStream_t)hip_stream, point_args(m, params, B),
                     mp_args(m), tg, x, y, (long long)n_pts, xy_batched, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
