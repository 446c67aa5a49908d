// gigalens_hip.hip -- C ABI (include/gigalens_hip.h) over the kernels in gl_kernels.hip.h.
// gfx950 only.  No per-call allocation, no host synchronisation: every entry point enqueues on
// the caller's stream and returns (hipGraph-capturable).
#include "../../include/gigalens_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#define GL_AUX_KERNELS 1
#include "gl_host_tables.h"
#include "gl_model.h"
#include "gl_static.hip.h"
#include "gl_post.hip.h"
#include "gl_positions.hip.h"
#include "gl_images.hip.h"
#include "gl_critical.hip.h"
#include "gl_pixsrc.hip.h"
#include "gl_multiplane.hip.h"
#include "gl_multiplane_bwd.hip.h"
#include "gl_potential.hip.h"
#include "gl_lstsq.hip.h"
#include "gl_shp.hip.h"

using namespace glk;

namespace {
thread_local char g_err[512] = "";
}

namespace glk {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace glk

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

}  // namespace


namespace {

// number of pixel chunks per sample: enough workgroups to fill 256 CUs several times over
// (dynamic load balance: EPL trip counts differ per sample), but whole tiles per chunk.
void chunking(const gl_model* m, int B, int* chunk, int* n_chunks) {
  const long long tile_px = (long long)WG * 4;  // whole tiles for every T in {1, 2, 4}
  // chunks per sample: enough workgroups for one resident round of the chip (768 = 256 CUs x 3), and at most ~8192 pixels
  // (16 pair tiles) per workgroup so the tail of the launch stays short -- measured at B = 64 .. 1024, 60^2 .. 256^2 px:
  // never behind the older "2048 workgroups" rule, 2-5 % ahead of it at small batches.  GIGALENS_HIP_TARGET_WGS restores that rule.
  long long want = std::max<long long>((768 + B - 1) / B, ((long long)m->N + 8191) / 8192);
  // (the specialised compositions only: with hundreds to thousands of instructions per pixel -- interpreter and cluster
  // kernels -- a workgroup's fixed costs vanish and more, smaller workgroups balance better: C6 4.83 vs 4.98 ms)
  if (m->target_wgs_set || !m->static_id) want = std::max<long long>(1, (m->target_wgs + B - 1) / B);
  long long per = ((long long)m->N + want - 1) / want;
  per = std::max(tile_px, (per + tile_px - 1) / tile_px * tile_px);
  if (m->chunk_px_override > 0) per = m->chunk_px_override;  // experiments: GIGALENS_HIP_CHUNK_PX (a multiple of the kernel's tile)
  *chunk = (int)per;
  *n_chunks = (int)(((long long)m->N + per - 1) / per);
}

// the wavefront-per-sample front end (gl_prep_wave_kernel) carries the sort of the cost-ordered dispatch as one extra workgroup:
// no launch of gl_order_kernel (one launch boundary less on every step)
bool wave_front_end(const gl_model* m) { return m->has_epl && (int)m->comps.size() <= 64 && m->wave_prep; }
bool order_in_front_end(const gl_model* m, int B) {
  return wave_front_end(m) && m->use_order && m->order_fused && m->epl_comp >= 0 && B >= 2;
}

// Tapered end of the cost-ordered dispatch (pair kernels, fused likelihood).  A launch is whole resident rounds of the chip
// (256 CUs x the workgroups a CU holds) plus a remainder; the samples of the remainder -- the cheapest ones, dispatched last --
// run as twice as many workgroups of half the pixels, so the last round is made of shorter workgroups (C2 at 1024 samples: two
// rounds of 768 + 512 workgroups -> two rounds + 1024 half-size ones: -0.9 us of 87).  Splitting samples that are NOT the
// remainder puts the boundary inside a round and costs 2-3 %, hence the exact count.  Returns the workgroups per tail sample
// (0 = does not apply), the first tail rank and the partial rows per sample.
int tail_plan(const gl_model* m, int B, int n_chunks, int* tail_from, int* n_rows) {
  *tail_from = B;
  *n_rows = n_chunks;
  const bool pair_epl = m->pair && (m->static_id == ST_EPLSHEAR_SERSIC || m->static_id == ST_EPLSHEAR_SERSIC_SERSIC);
  if (m->tail_rows == 0 || !pair_epl || m->has_post || !order_in_front_end(m, B) || B > 1024) return 0;
  const int tiles = (m->N + 2 * WG - 1) / (2 * WG);
  const int slots = 256 * (m->static_id == ST_EPLSHEAR_SERSIC ? 3 : 2);  // launch_static: waves per SIMD the kernel is budgeted for
  int n_tail = m->tail_n, rows = m->tail_rows;
  if (n_tail < 0) {  // the remainder beyond whole rounds, when it is a substantial part of a round
    const long long wgs = (long long)B * n_chunks, rem = wgs % slots;
    if (wgs < slots || rem * 4 < slots) return 0;
    n_tail = (int)(rem / n_chunks);
  }
  if (rows < 0) rows = 2 * n_chunks;
  if (n_tail <= 0 || n_tail > B || rows > tiles || rows == n_chunks) return 0;
  *tail_from = B - n_tail;
  *n_rows = std::max(n_chunks, rows);
  return rows;
}

// The launch shape of one call on B samples.  Computed once per entry point and passed down: the workspace layout (carve), the
// rank the front end's sort splits at (run_prep) and the main kernel's grid (run_likelihood) all read the same plan.
struct LaunchPlan {
  int chunk, n_chunks;  // pixels per workgroup, workgroups per sample (chunking)
  int tail_rows;        // workgroups per sample of the tapered end, 0 = the shape has none (tail_plan)
  int tail_from;        // first rank of the tapered end (B without one)
  int n_rows;           // partial rows a sample owns in the workspace: max(n_chunks, tail_rows)
};
LaunchPlan launch_plan(const gl_model* m, int B) {
  LaunchPlan p{};
  chunking(m, B, &p.chunk, &p.n_chunks);
  p.tail_rows = tail_plan(m, B, p.n_chunks, &p.tail_from, &p.n_rows);
  return p;
}

struct Workspace {
  float* derived;
  float* partial;
  float* params;  // [B,P] constrained rows produced from z (gl_logprob_fwd_bwd)
  int* order;     // [B] cost-ordered dispatch
  int* cost;      // [B] per-sample dispatch cost written by prep (single-EPL models)
  float* gal_dyn;  // [B][G][DP_ND] catalogue members' per-sample constants
  float *pos_w, *pos_adj, *pos_g, *pos_fam, *pos_ll, *pos_chi2, *pos_grad;  // image-position likelihood
  float* img_ss;   // supersampled / pre-PSF image or its cotangent (PSF path only)
  float* img_tmp;  // final-resolution image / its cotangent (PSF path only)
  float* stats;    // [B][2] chi2, normalisation of the materialised image (PSF path only)
  size_t bytes;
};

// (the partial rows are sized for the tapered end whenever the shape has one, whether or not the call at hand uses it)
Workspace carve(const gl_model* m, int B, void* base, const LaunchPlan& plan) {
  Workspace w{};
  size_t off = 0;
  char* p = (char*)base;
  w.derived = (float*)(p + off);
  off += align_up((size_t)B * m->D * sizeof(float), 256);
  w.partial = (float*)(p + off);
  off += align_up((size_t)B * plan.n_rows * m->A * sizeof(float), 256);
  w.params = (float*)(p + off);
  off += align_up((size_t)B * std::max(m->P, 1) * sizeof(float), 256);
  w.order = (int*)(p + off);
  off += align_up((size_t)B * sizeof(int), 256);
  w.cost = (int*)(p + off);
  off += align_up((size_t)B * sizeof(int), 256);
  if (m->G) {
    w.gal_dyn = (float*)(p + off);
    off += align_up((size_t)B * m->G * GM_ND * sizeof(float), 256);
  }
  if (m->pos_J) {
    auto take = [&](size_t n) { float* q = (float*)(p + off); off += align_up(n * sizeof(float), 256); return q; };
    w.pos_w = take((size_t)B * m->pos_J * 6);
    w.pos_adj = take((size_t)B * m->pos_J * 3);
    w.pos_g = take((size_t)B * m->pos_J * std::max(m->P, 1));
    w.pos_fam = take((size_t)B * m->pos_F * 2);
    w.pos_ll = take(B);
    w.pos_chi2 = take(B);
    w.pos_grad = take((size_t)B * std::max(m->P, 1));
  }
  if (m->has_post) {
    w.img_ss = (float*)(p + off);
    off += align_up((size_t)B * m->height * m->width * sizeof(float), 256);
    w.img_tmp = (float*)(p + off);  // final-resolution image / its cotangent
    off += align_up((size_t)B * (m->height / m->supersample) * (m->width / m->supersample) * sizeof(float), 256);
    w.stats = (float*)(p + off);
    off += align_up((size_t)B * 2 * sizeof(float), 256);
  } else if (m->mp_K >= 2) {  // lens planes (gl_multiplane_loglike): the image is materialised for the pixel statistics
    w.img_tmp = (float*)(p + off);
    off += align_up((size_t)B * m->height * m->width * sizeof(float), 256);
    w.stats = (float*)(p + off);
    off += align_up((size_t)B * 2 * sizeof(float), 256);
  }
  w.bytes = off;
  return w;
}


MainArgs base_args(const gl_model* m, const Workspace& w, int chunk) {
  MainArgs a{};
  a.comps = m->d_comps;
  a.n_lens = m->n_lens;
  a.n_ll = m->n_ll;
  a.n_src = m->n_src;
  a.derived = w.derived;
  a.D = m->D;
  a.A = m->A;
  a.Apad = m->Apad;
  a.ncols = m->ncols;
  a.gx = m->d_gx;
  a.gy = m->d_gy;
  a.pix = m->d_pix;
  a.N = m->N;
  a.chunk = chunk;
  a.img_stride = (long long)m->height * m->width;
  a.out_scale = m->conversion_factor;
  a.partial = w.partial;
  a.shp_tab = m->d_shp_tab;
  a.nfw_tab = m->d_nfw_tab;
  a.neutral = m->d_nfw_tab ? m->d_nfw_tab + 2 * glh::kNfwNodes : nullptr;
  a.grid_rmax = m->shp_cull ? m->grid_rmax : -1.f;  // (negative: the culling test of the table-mode shapelet kernels is off)
  a.dbg = m->dbg_flags;
  a.shp_stride = m->shp_stride;
  a.parts = 7u;
  a.cats = m->d_cats;
  a.gal_static = m->d_gal_static;
  a.gal_dyn = w.gal_dyn;
  a.G = m->G;
  a.scaled_first = m->cats.empty() ? -1 : m->cats[0].dev.comp;
  a.series = m->d_series;
  a.interp = m->d_interp;
  a.src_scale = m->src_scaled ? m->d_src_scale.get() : nullptr;
  return a;
}

// "The model is ready": every GL_SCALED lens has its catalogue, every GL_INTERPOL light its image and (with_series) every GL_SERIES
// lens its coefficient field.  The
// pixel-grid entry points report how many are missing and the call that attaches them (counted = true), the others name the kind.
int check_ready(const gl_model* m, bool with_series, bool counted) {
  const int no_cat = m->n_scaled - (int)m->cats.size(), no_field = m->n_series - m->n_series_set;
  if (no_cat)
    return counted ? fail(GL_EINVAL, "%d GL_SCALED component(s) without a catalogue (gl_model_set_catalogue)", no_cat)
                   : fail(GL_EINVAL, "GL_SCALED component without a catalogue");
  if (m->n_interp != m->n_interp_set)
    return fail(GL_EINVAL, "%d GL_INTERPOL component(s) without an image (gl_model_set_light_image)", m->n_interp - m->n_interp_set);
  if (with_series && no_field)
    return counted ? fail(GL_EINVAL, "%d GL_SERIES component(s) without a coefficient field (gl_model_set_series)", no_field)
                   : fail(GL_EINVAL, "GL_SERIES component without a coefficient field");
  return GL_OK;
}

// A model with lens planes (gl_model_set_lens_planes) is served by the gl_multiplane_* entries alone: every single-plane entry
// refuses it instead of tracing its lenses as if they shared a plane.
int refuse_planes(const gl_model* m, const char* what) {
  if (m && m->mp_K >= 2)
    return fail(GL_EUNSUPPORTED, "%s does not serve a model with %d lens planes (gl_model_set_lens_planes): lens maps, renders, "
                                 "pixel statistics and their gradients through the gl_multiplane_* entries alone", what, m->mp_K);
  return GL_OK;
}

// the arguments every pixel-grid call shares; on success the call's launch plan and its workspace, carved
int check_call(const gl_model* m, const void* params, int B, void* ws, size_t ws_bytes, LaunchPlan* plan, Workspace* w) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (!params) return fail(GL_EINVAL, "params is null");
  if (B <= 0 || B > 65535) return fail(GL_EINVAL, "batch size %d outside [1, 65535]", B);
  if (int rc = check_ready(m, true, true)) return rc;
  if (!ws) return fail(GL_EINVAL, "workspace is null");
  *plan = launch_plan(m, B);
  *w = carve(m, B, ws, *plan);
  if (ws_bytes < w->bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", ws_bytes, w->bytes);
  return GL_OK;
}

// per (sample, galaxy) constants of the catalogue members, from the constrained parameter rows
int run_galprep(const gl_model* m, const float* params, int B, const Workspace& w, hipStream_t stream) {
  if (!m->G) return GL_OK;
  long long total = (long long)B * m->G;
  hipLaunchKernelGGL(gl_galprep_kernel, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, stream, m->d_comps,
                     m->d_cats, (int)m->cats.size(), params, m->P, B, m->d_gal_table, m->d_gal_static, w.gal_dyn, m->G);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// LDS of the wavefront front end: one parameter row per wavefront of the workgroup (0: rows too long, read back from global memory)
size_t prep_row_bytes(const gl_model* m) {
  const size_t bytes = (size_t)4 * m->P * sizeof(float);
  return (m->prep_lds && bytes <= 48 * 1024) ? bytes : 0;
}

// The front end of a call: derived constants, dispatch cost and (wavefront form) the cost order of every sample, then the catalogue
// members' constants.  The rows come packed (`params` [B,P], z null) or unconstrained (`z` [B,d_z], params null: the constrained
// rows are written to w.params through the model's bijectors).
int run_prep(const gl_model* m, const float* params, const float* z, int B, const LaunchPlan& plan, const Workspace& w,
             hipStream_t stream) {
  const int n_comp = (int)m->comps.size(), d_z = z ? m->d_z : 0;
  const ZCol* zcols = z ? m->d_zcols.get() : nullptr;
  const int* src = z ? m->d_src.get() : nullptr;
  const float* const_row = z ? m->d_const.get() : nullptr;
  float* rows_out = z ? w.params : nullptr;
  int* cost = m->epl_comp >= 0 ? w.cost : nullptr;
  if (wave_front_end(m)) {  // one wavefront per sample: the EPL coefficient tables are built by a scan over its lanes
    const bool ord = order_in_front_end(m, B);
    const size_t rows = prep_row_bytes(m);
    // the rank the sort must split deterministically: which samples run the tapered end may not depend on the order the atomics
    // of the counting sort leave inside a cost bin
    const int split_rank = plan.tail_rows ? plan.tail_from : -1;
    hipLaunchKernelGGL(gl_prep_wave_kernel, dim3((B + 3) / 4 + (ord ? 1 : 0)), dim3(256), rows, stream, m->d_comps.get(), n_comp,
                       params, z, d_z, zcols, src, const_row, m->P, B, rows_out, w.derived, m->D, cost, m->epl_comp,
                       ord ? w.order : nullptr, rows ? 1 : 0, split_rank, m->d_interp.get());
  } else if (z) {  // thread per component
    hipLaunchKernelGGL(gl_zprep_kernel, dim3((B * n_comp + 127) / 128), dim3(128), 0, stream, m->d_comps.get(), n_comp, z, d_z,
                       zcols, src, const_row, m->P, B, rows_out, w.derived, m->D, cost, m->epl_comp, m->d_interp.get());
  } else {
    hipLaunchKernelGGL(gl_prep_kernel, dim3((B * n_comp + 127) / 128), dim3(128), 0, stream, m->d_comps.get(), n_comp, params,
                       m->P, B, w.derived, m->D, cost, m->epl_comp, m->d_interp.get());
  }
  GL_HIP(hipGetLastError());
  return run_galprep(m, z ? w.params : params, B, w, stream);
}

FinArgs fin_args(const gl_model* m, const float* params, const Workspace& w, float* loglike, float* chi2, float* grad,
                 const float* z, float* logprob, float* grad_z, float chi2_scale, const float* extra_stats,
                 int use_partial, bool with_positions, float pos_chi2_scale) {
  FinArgs f{};
  f.n_comp = (int)m->comps.size();
  f.P = m->P;
  f.A = m->A;
  f.d_z = m->d_z;
  f.params = params;
  f.loglike = loglike;
  f.chi2 = chi2;
  f.grad = grad;
  f.z = z;
  f.zcols = z ? (const ZCol*)m->d_zcols : nullptr;
  f.logprob = logprob;
  f.grad_z = grad_z;
  f.chi2_scale = chi2_scale;
  f.extra_stats = extra_stats;
  f.use_partial = use_partial;
  f.pos_ll = with_positions ? w.pos_ll : nullptr;
  f.pos_chi2 = with_positions ? w.pos_chi2 : nullptr;
  f.pos_grad = with_positions && (grad || grad_z) ? w.pos_grad : nullptr;
  f.pos_chi2_scale = pos_chi2_scale;
  f.cats = m->d_cats;
  return f;
}

int run_finalize(const gl_model* m, const float* params, int B, int n_chunks, const Workspace& w, float* loglike,
                 float* chi2, float* grad, hipStream_t stream, const float* z = nullptr, float* logprob = nullptr,
                 float* grad_z = nullptr, float chi2_scale = 1.f, const float* extra_stats = nullptr,
                 int use_partial = 1, bool with_positions = false, float pos_chi2_scale = 0.f) {
  size_t shmem = (size_t)(((m->A + 3) & ~3) + ((m->P + 3) & ~3) + ((m->d_z + 3) & ~3) + 4 * m->d_z + 4 + m->P) * sizeof(float);
  FinArgs f = fin_args(m, params, w, loglike, chi2, grad, z, logprob, grad_z, chi2_scale, extra_stats, use_partial,
                       with_positions, pos_chi2_scale);
  bool basic = true;
  for (const CompDesc& c : m->comps)
    basic = basic && (c.kind == K_EPL || c.kind == K_SIE || c.kind == K_SHEAR || c.kind == K_SIS || c.kind == K_SERSIC || c.kind == K_SERSIC_ELLIPSE);
  const int nc = GL_DBG(m->dbg_flags, 8) ? -1 : n_chunks;
  if (basic) hipLaunchKernelGGL(gl_finalize_kernel<true>, dim3(B), dim3(128), shmem, stream, m->d_comps, f, w.partial, nc);
  else hipLaunchKernelGGL(gl_finalize_kernel<false>, dim3(B), dim3(128), shmem, stream, m->d_comps, f, w.partial, nc);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// heaviest samples first (only EPL has a data-dependent cost)
int run_order(const gl_model* m, int B, const Workspace& w, MainArgs* a, hipStream_t stream) {
  a->order = nullptr;
  if (!m->has_epl || !m->use_order || B < 2) return GL_OK;
  if (order_in_front_end(m, B)) {  // the front end's extra workgroup has written it
    a->order = w.order;
    return GL_OK;
  }
  hipLaunchKernelGGL(gl_order_kernel, dim3(1), dim3(ORDER_WG), 0, stream, m->d_comps, m->n_lens, w.derived, m->D, B,
                     w.order, m->epl_comp >= 0 ? w.cost : nullptr);
  GL_HIP(hipGetLastError());
  a->order = w.order;
  return GL_OK;
}


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
  return a;
}

// image-position likelihood on the packed parameter rows `params` [B,P] (already on the device)
int run_positions(const gl_model* m, const float* params, int B, const Workspace& w, bool want_grad, hipStream_t stream) {
  if (m->n_series) return fail(GL_EUNSUPPORTED, "a series-expansion lens lives on the pixel grid only (series_profile.py:76-81): no image-position likelihood");
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
  a.fam_scale = m->pos_scaled ? m->d_pos_scale.get() : nullptr;
  a.w_pos = w.pos_w;
  a.w_adj = w.pos_adj;
  a.w_g = w.pos_g;
  a.w_fam = w.pos_fam;
  a.ll = w.pos_ll;
  a.chi2 = w.pos_chi2;
  a.grad = want_grad ? w.pos_grad : nullptr;
  auto blocks = [](long long n) { return dim3((unsigned)((n + 63) / 64)); };
  if (m->has_user) {
    int lens_params = m->lens_params;
    void* args1[] = {&a};
    void* args2[] = {&a, &lens_params};
    auto go = [&](int k, long long n, void** args) {
      return hipModuleLaunchKernel(m->user_point_fn[k], blocks(n).x, 1, 1, 64, 1, 1, 0, stream, args, nullptr);
    };
    GL_HIP(go(0, (long long)B * a.J, args1));
    GL_HIP(go(1, (long long)B * a.F, args1));
    if (want_grad && m->lens_params) GL_HIP(go(2, (long long)B * a.J * m->lens_params, args2));
    GL_HIP(go(3, (long long)B * (a.P + 1), args2));
    return GL_OK;
  }
  hipLaunchKernelGGL(gl_pos_p1_kernel, blocks((long long)B * a.J), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(gl_pos_p2_kernel, blocks((long long)B * a.F), dim3(64), 0, stream, a);
  if (want_grad && m->lens_params)
    hipLaunchKernelGGL(gl_pos_p3_kernel, blocks((long long)B * a.J * m->lens_params), dim3(64), 0, stream, a,
                       m->lens_params);
  hipLaunchKernelGGL(gl_pos_p4_kernel, blocks((long long)B * (a.P + 1)), dim3(64), 0, stream, a, m->lens_params);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- PSF / supersampling path (gl_post.hip.h) -------------------------------------------------------------
PostArgs post_args(const gl_model* m, float scale) {
  PostArgs p{};
  p.keff = m->d_psf;
  p.KH = m->KH; p.KW = m->KW; p.pt = m->pad_t; p.pl = m->pad_l;
  p.Hs = m->height; p.Ws = m->width; p.ss = m->supersample;
  p.H = m->height / m->supersample; p.W = m->width / m->supersample;
  p.scale = scale;
  return p;
}
// supersampled pre-PSF image S [B,Hs,Ws] -> final image [B,H,W] (x conversion factor)
// the register-blocked pair kernel on one plan (gl_post.hip.h); false: no instantiation for this kernel width / stride
// the instantiations launch_corr can reach: the wide stride-2 family (16 outputs per thread) requires KWP <= 28, and the
// supersample-2 transpose plan (two column classes per thread) has KWP = pad4(width) with width <= ceil(32 / 2) + 1 = 17
constexpr bool corr_reachable(int kwp, int ncj, int ox) { return !(ox == 16 && kwp > 28) && !(ncj == 2 && kwp > 20); }
template <int KWP, int ST, int KS, int NCJ, int OX>
bool corr_launch(dim3 grid, size_t sh, hipStream_t stream, const float* in, float* out, const CorrArgs& a, std::atomic<const void*>* last) {
  if constexpr (corr_reachable(KWP, NCJ, OX)) {
    auto* fn = gl_corr_pair_kernel<KWP, ST, KS, NCJ, OX>;
    if (sh > 64 * 1024) {
      static const hipError_t big = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      if (big != hipSuccess) return false;
    }
    hipLaunchKernelGGL(fn, grid, dim3(CORR_GT * KS), sh, stream, in, out, a);
    if (last) last->store(reinterpret_cast<const void*>(fn), std::memory_order_relaxed);
    return true;
  } else {
    return false;
  }
}
// `last`: where the host function of the launched kernel is recorded (gl_model_last_post_kernel)
bool launch_corr(const gl_model::CorrPlan& pl, int B, const float* in, float* out, float scale, hipStream_t stream, int dbg = 0,
                 int max_pairs_env = 0, int corr_wide = 1, std::atomic<const void*>* last = nullptr) {
  if (!pl.ok) return false;
  CorrArgs a = pl.args;
  a.B = B;
  a.scale = scale;
  a.dbg = dbg;
  a.vec = (a.Wi % 4 == 0 && a.Wout % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) ? 1 : 0;
  // forward at supersample 2 with kernels up to 28 taps wide: 16 outputs per thread and 8 wavefronts per tile (two 75 KB tiles per
  // CU); everything else 8 outputs per thread
  const bool wide = pl.ST == 2 && a.ncj == 1 && pl.KWP <= 28 && pl.max_KH <= 28 && corr_wide;
  // (16 outputs per thread in the transpose at supersample 2 as well: 62.7 us against 47.6 -- half the workgroups, 1.56 rounds)
  const int ox = wide ? 16 : CORR_OX, ks = wide ? 8 : pl.ST == 2 ? 4 : 2;
  const int TR = (CORR_TR - 1) * pl.ST + pl.max_KH, TC = corr_tile_width((CORR_TCG * ox - 1) * pl.ST + pl.KWP) | 1;
  const size_t sh = std::max((size_t)TR * TC * sizeof(float2), (size_t)(ks - 1) * a.ncj * ox * CORR_GT * sizeof(float2) +
                                                                   (size_t)2 * CORR_TR * CORR_TCG * ox * a.ncj * sizeof(float));
  if (sh > (wide ? 80 : 64) * 1024) return false;
  // grid.z carries (row class, sample pair): at most 65535 per launch -- larger batches (the basis stack of lstsq_simulate is
  // B x D images) go out in slices
  const int max_pairs = max_pairs_env > 0 ? max_pairs_env : 65535 / a.n_class;
  if ((B + 1) / 2 > max_pairs) {
    for (int b_lo = 0; b_lo < B; b_lo += 2 * max_pairs) {
      const int nb = std::min(B - b_lo, 2 * max_pairs);
      if (!launch_corr(pl, nb, in + (size_t)b_lo * a.Hi * a.Wi, out + (size_t)b_lo * a.Hout * a.Wout, scale, stream, dbg, max_pairs_env, corr_wide, last)) return false;
    }
    return true;
  }
  const dim3 grid((pl.max_Wo + CORR_TCG * ox - 1) / (CORR_TCG * ox), (pl.max_Ho + CORR_TR - 1) / CORR_TR,
                  (unsigned)(a.n_class * ((B + 1) / 2)));
#define GL_CORR(KWP_, ST_, KS_, NCJ_, OX_) return corr_launch<KWP_, ST_, KS_, NCJ_, OX_>(grid, sh, stream, in, out, a, last);
#define GL_CORR_W(ST_, KS_, NCJ_, OX_)                                                                                          \
  switch (pl.KWP) {                                                                                                             \
    case 4: GL_CORR(4, ST_, KS_, NCJ_, OX_) case 8: GL_CORR(8, ST_, KS_, NCJ_, OX_) case 12: GL_CORR(12, ST_, KS_, NCJ_, OX_)     \
    case 16: GL_CORR(16, ST_, KS_, NCJ_, OX_) case 20: GL_CORR(20, ST_, KS_, NCJ_, OX_) case 24: GL_CORR(24, ST_, KS_, NCJ_, OX_) \
    case 28: GL_CORR(28, ST_, KS_, NCJ_, OX_) case 32: GL_CORR(32, ST_, KS_, NCJ_, OX_)                                          \
    default: return false;                                                                                                      \
  }
  if (wide) { GL_CORR_W(2, 8, 1, 16) }
  if (pl.ST == 2 && a.ncj == 1) { GL_CORR_W(2, 4, 1, CORR_OX) }  // forward at supersample 2
  if (pl.ST == 1 && a.ncj == 1) { GL_CORR_W(1, 2, 1, CORR_OX) }  // forward / transpose at supersample 1
  if (pl.ST == 1 && a.ncj == 2) { GL_CORR_W(1, 2, 2, CORR_OX) }  // transpose at supersample 2
#undef GL_CORR_W
#undef GL_CORR
  return false;
}

int post_fwd(const gl_model* m, int B, const float* S, float* out, hipStream_t stream, float scale) {
  if (launch_corr(m->corr_fwd, B, S, out, scale, stream, m->dbg_flags, m->corr_max_pairs, m->corr_wide, &m->last_post_fn[0])) {
    GL_HIP(hipGetLastError());
    return GL_OK;
  }
  PostArgs p = post_args(m, scale);
  const int TR = (PT - 1) * p.ss + p.KH, TC = ((PT - 1) * p.ss + p.KW) | 1;
  size_t shmem = (size_t)TR * TC * sizeof(float);
  if (shmem > 64 * 1024) return fail(GL_EUNSUPPORTED, "PSF too large for the LDS-tiled convolution (%zu B)", shmem);
  dim3 grid((p.W + PT - 1) / PT, (p.H + PT - 1) / PT, B);
  hipLaunchKernelGGL(gl_psf_pool_fwd_kernel, grid, dim3(256), shmem, stream, S, out, p);
  m->last_post_fn[0].store(reinterpret_cast<const void*>(gl_psf_pool_fwd_kernel), std::memory_order_relaxed);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
// cotangent of the final image [B,H,W] -> cotangent of S [B,Hs,Ws]
int post_bwd(const gl_model* m, int B, const float* gP, float* gS, hipStream_t stream, float scale) {
  if (launch_corr(m->corr_bwd, B, gP, gS, scale, stream, m->dbg_flags, m->corr_max_pairs, m->corr_wide, &m->last_post_fn[1])) {
    GL_HIP(hipGetLastError());
    return GL_OK;
  }
  PostArgs p = post_args(m, scale);
  const int TR = (PT - 1 + p.KH) / p.ss + 3, TC = ((PT - 1 + p.KW) / p.ss + 3) | 1;
  size_t shmem = (size_t)TR * TC * sizeof(float);
  dim3 grid((p.Ws + PT - 1) / PT, (p.Hs + PT - 1) / PT, B);
  hipLaunchKernelGGL(gl_psf_pool_bwd_kernel, grid, dim3(256), shmem, stream, gP, gS, p);
  m->last_post_fn[1].store(reinterpret_cast<const void*>(gl_psf_pool_bwd_kernel), std::memory_order_relaxed);
  GL_HIP(hipGetLastError());
  return GL_OK;
}
int render_ss(const gl_model* m, MainArgs a, int B, int n_chunks, const Workspace& w, hipStream_t stream) {
  if (m->d_pix) GL_HIP(hipMemsetAsync(w.img_ss, 0, sizeof(float) * (size_t)B * m->height * m->width, stream));
  a.img = w.img_ss;
  a.out_scale = 1.f;  // NaN -> 0 happens in the kernel; the det(T) scale is applied after pooling (tf/simulator.py:156)
  return launch_main<IMG_FWD>(m, a, B, n_chunks, stream);
}

// likelihood after prep: fused kernel when the image never has to exist, else render -> PSF/pool -> pixel
// statistics (-> transposes -> VJP).  Tells finalize where chi2 / normalisation come from.
// `fin_rows`: the partial rows per sample finalize must reduce (the plan's chunks, or its rows when the tapered end ran).
int run_likelihood(const gl_model* m, int B, const LaunchPlan& plan, const Workspace& w, const float* obs,
                   const float* err, const float* mask, float bg_rms, float exp_time, bool want_grad,
                   hipStream_t stream, const float** extra_stats, int* use_partial, int* fin_rows) {
  int rc;
  const int n_chunks = plan.n_chunks;
  MainArgs a = base_args(m, w, plan.chunk);
  a.obs = obs;
  a.err = err;
  a.mask = mask;
  a.bg2 = bg_rms * bg_rms;
  a.inv_t = 1.0f / exp_time;
  if ((rc = run_order(m, B, w, &a, stream))) return rc;
  *extra_stats = nullptr;
  *use_partial = 1;
  *fin_rows = n_chunks;
  if (!m->has_post && a.order && want_grad) {  // (the rounds are counted for the gradient kernels' occupancy; forward-only calls keep the plain grid)
    a.tail_rows = plan.tail_rows;
    a.tail_from = plan.tail_from;
    a.n_rows = plan.n_rows;
    a.n_samples = B;
    *fin_rows = plan.n_rows;
  }
  if (!m->has_post) return want_grad ? launch_main<LL_GRAD>(m, a, B, n_chunks, stream) : launch_main<LL_FWD>(m, a, B, n_chunks, stream);
  if ((rc = render_ss(m, a, B, n_chunks, w, stream))) return rc;
  if ((rc = post_fwd(m, B, w.img_ss, w.img_tmp, stream, m->conversion_factor))) return rc;
  const int HW = (m->height / m->supersample) * (m->width / m->supersample);
  hipLaunchKernelGGL(gl_imgstats_kernel, dim3(B), dim3(256), 0, stream, w.img_tmp, obs, err, mask, a.bg2, a.inv_t, HW,
                     w.stats, want_grad ? w.img_tmp : nullptr);
  GL_HIP(hipGetLastError());
  *extra_stats = w.stats;
  *use_partial = want_grad ? 1 : 0;
  if (!want_grad) return GL_OK;
  if ((rc = post_bwd(m, B, w.img_tmp, w.img_ss, stream, m->conversion_factor))) return rc;
  a.gimg = w.img_ss;
  a.out_scale = 1.f;
  return launch_main<IMG_BWD>(m, a, B, n_chunks, stream);
}

}  // namespace

namespace {
struct LstsqWs {
  float *stack_ss, *stack, *partial, *coeffs;
  float* mats;  // [B][2][D][D | 1]: A and V of the eigen solve for systems above LS_LDS_MAXN unknowns (else null)
  int* todo;    // [B]: 1 = the Cholesky attempt left this system to the eigenvalue solve
  int chunk, n_chunks, Dp;
  int n_chunks_f;  // workgroups per sample of the stack-free kernel (gl_shp_normal_kernel: 512-pixel tiles dealt round-robin)
  size_t bytes;
};
// a kernel that asks for more than 64 KB of dynamic LDS (up to the CU's 160) has to be told once per process
int raise_lds_limit(const void* kernel, bool* raised) {
  if (!*raised) {
    GL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    *raised = true;
  }
  return GL_OK;
}

// pixel chunks per sample of the normal-matrix kernels: ~`wgs` (2048) workgroups in flight, whole 64-pixel groups per chunk
void lstsq_chunks(long long HW, int B, int wgs, int* chunk, int* n_chunks) {
  long long want = std::max<long long>(1, ((long long)wgs + B - 1) / B);
  long long per = (HW + want - 1) / want;
  per = std::max<long long>(2 * LS_TPP, (per + 2 * LS_TPP - 1) / (2 * LS_TPP) * (2 * LS_TPP));
  *chunk = (int)per;
  *n_chunks = (int)((HW + per - 1) / per);
}

// (behind the call workspace `cw` of the same base)
LstsqWs carve_lstsq(const gl_model* m, int B, void* base, const Workspace& cw) {
  LstsqWs w{};
  size_t off = align_up(cw.bytes, 256);
  const int D = (int)m->lin_cols.size();
  const size_t HWs = (size_t)m->height * m->width, HW = HWs / ((size_t)m->supersample * m->supersample);
  char* p = (char*)base;
  auto take = [&](size_t n) { float* q = (float*)(p + off); off += align_up(n * sizeof(float), 256); return q; };
  w.Dp = (D + 1 + 3) & ~3;
  lstsq_chunks((long long)HW, B, m->lstsq_wgs, &w.chunk, &w.n_chunks);
  w.stack_ss = m->has_post ? take((size_t)B * D * HWs) : nullptr;
  w.stack = take((size_t)B * D * HW);
  // three workgroups per CU there: 1.5 x the workgroup target = four full rounds of the chip at the default (measured: 2048 ->
  // 0.708, 3072 -> 0.694, 4096 -> 0.697, 6144 -> 0.715 ms per C3L solve)
  w.n_chunks_f = (int)std::min<long long>(((long long)HW + 511) / 512, std::max<long long>(1, (3LL * m->lstsq_wgs / 2 + B - 1) / B));
  w.partial = take((size_t)B * std::max(w.n_chunks, w.n_chunks_f) * w.Dp * w.Dp);
  w.coeffs = take((size_t)B * D);
  w.mats = D > LS_LDS_MAXN ? take((size_t)B * 2 * D * (D | 1)) : nullptr;
  w.todo = (int*)take((size_t)B);
  w.bytes = off;
  return w;
}
}  // namespace

// ---- gl_model_create_user, step by step ----------------------------------------------------------------------------------
namespace {
struct ModelDeleter {
  void operator()(gl_model* m) const { gl_model_destroy(m); }
};

int check_create_args(const gl_component* comps, int n_lens, int n_lens_light, int n_src, const gl_grid* grid) {
  if (!grid) return fail(GL_EINVAL, "grid is null");
  if (n_lens < 0 || n_lens_light < 0 || n_src < 0) return fail(GL_EINVAL, "negative component count");
  if (n_lens + n_lens_light + n_src > 0 && !comps) return fail(GL_EINVAL, "comps is null");
  if (grid->height <= 0 || grid->width <= 0 || grid->n_region <= 0) return fail(GL_EINVAL, "empty grid");
  if (!grid->grid_x || !grid->grid_y) return fail(GL_EINVAL, "grid_x / grid_y is null");
  if (grid->supersample < 1) return fail(GL_EINVAL, "supersample must be >= 1");
  if (grid->height % grid->supersample || grid->width % grid->supersample)
    return fail(GL_EINVAL, "grid size not a multiple of supersample");
  if ((long long)grid->n_region > (long long)grid->height * grid->width)
    return fail(GL_EINVAL, "n_region exceeds height*width");
  if (!grid->pix_index && (long long)grid->n_region != (long long)grid->height * grid->width)
    return fail(GL_EINVAL, "pix_index is required when n_region != height*width");
  if (grid->psf && (grid->psf_h <= 0 || grid->psf_w <= 0)) return fail(GL_EINVAL, "bad PSF shape");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GL_ENODEVICE, "no HIP device available");
  return GL_OK;
}

// the component table (offsets into the parameter, derived and accumulator rows), the linear columns and what the kinds imply
int build_components(gl_model* m, const gl_component* comps, int n_comp, const char* const* bodies, int n_bodies) {
  const int n_lens = m->n_lens;
  int p_off = 0, d_off = 0, a_off = NSTAT;
  for (int i = 0; i < n_comp; ++i) {
    const gl_component& c = comps[i];
    const bool mass = i < n_lens;
    const bool is_mass_kind = (c.kind >= GL_EPL && c.kind <= GL_TNFW) || c.kind == GL_USER_MASS;
    const bool is_light_kind = (c.kind >= GL_SERSIC && c.kind <= GL_CORE_SERSIC) || c.kind == GL_USER_LIGHT || c.kind == GL_INTERPOL;
    if ((mass && !is_mass_kind) || (!mass && !is_light_kind))
      return fail(GL_EINVAL, "component %d: kind %d is not a %s profile", i, c.kind, mass ? "mass" : "light");
    int iparam = c.iparam;
    if (c.kind == GL_USER_MASS || c.kind == GL_USER_LIGHT) {
      if (iparam < 0 || iparam > USER_MAXP || (int)c.flags >= n_bodies || !bodies[c.flags])
        return fail(GL_EINVAL, "component %d: a user-written profile takes 0..%d parameters and the index of its body (got %d parameters, "
                               "body %u of %d)", i, USER_MAXP, iparam, c.flags, n_bodies);
      m->has_user = true;
    }
    if (c.kind == GL_EPL) {
      if (iparam <= 0) iparam = 50;  // epl.py:15
      if (iparam > 1000) return fail(GL_EINVAL, "EPL niter %d too large", iparam);
    }
    if (c.kind == GL_EPL) { m->epl_comp = m->has_epl ? -2 : i; m->has_epl = true; }
    if (c.kind >= GL_DPIS && c.kind <= GL_SERIES) m->fam = std::max(m->fam, 1);
    if (c.kind == GL_NFW_ELLIPSE || c.kind == GL_TNFW || c.kind == GL_CORE_SERSIC || c.kind == GL_INTERPOL) m->fam = 2;
    if (c.kind == GL_SERIES && (iparam < 0 || iparam > SERIES_MAX_ORDER))
      return fail(GL_EINVAL, "component %d: series order %d outside [0, %d]", i, iparam, SERIES_MAX_ORDER);
    if (c.kind == GL_SCALED) {
      if (iparam < 1 || iparam > 3) return fail(GL_EINVAL, "component %d: GL_SCALED takes 1..3 scales, got %d", i, iparam);
      ++m->n_scaled;
    }
    if (c.kind == GL_SHAPELETS) {
      if (iparam < 0 || iparam > GL_SHAPELETS_NMAX_CAP)
        return fail(GL_EUNSUPPORTED, "shapelets n_max=%d outside [0,%d]", iparam, GL_SHAPELETS_NMAX_CAP);
      m->has_shapelets = true;
      if (iparam > SH_CAP) m->shp_big = true;
      if (c.flags & GL_FLAG_SHAPELETS_INTERPOLATE) m->has_table = true;
    }
    CompDesc cd{};
    cd.kind = c.kind;
    cd.iparam = iparam;
    cd.flags = c.flags;
    cd.p_off = p_off;
    cd.d_off = d_off;
    cd.a_off = a_off;
    cd.n_par = kind_num_params(c.kind, iparam);
    cd.n_acc = kind_num_acc(c.kind, iparam);
    if (c.kind == GL_SCALED) cd.iparam = -1;  // catalogue slot, set by gl_model_set_catalogue
    if (c.kind == GL_SERIES) {
      cd.flags = (unsigned)m->n_series++;
      m->series.push_back(SeriesDev{nullptr, nullptr, 0.f, iparam});
      m->series_buf.emplace_back();
      m->series_comp.push_back(i);
    }
    if (c.kind == GL_INTERPOL) {  // table slot; the table itself arrives with gl_model_set_light_image
      cd.iparam = m->n_interp++;
      cd.flags = c.flags & GL_FLAG_INTERPOL_LINEAR;
      m->interp.push_back(InterpDev{nullptr, 0, 0});
      m->interp_buf.emplace_back();
    }
    cd.lin_off = (int)m->lin_cols.size();
    for (int k = 0; k < kind_num_linear(c.kind, iparam); ++k) m->lin_cols.push_back(p_off + kind_linear_col(c.kind, iparam) + k);
    // a user-written light whose last parameter is declared the linear amplitude (gl_component::reserved): one basis image
    if (c.kind == GL_USER_LIGHT && c.reserved == 1 && iparam >= 1) m->lin_cols.push_back(p_off + iparam - 1);
    p_off += cd.n_par;
    d_off += (kind_num_derived(c.kind, iparam) + 3) & ~3;
    a_off += cd.n_acc;
    m->comps.push_back(cd);
  }
  if (m->has_user && m->n_interp)
    return fail(GL_EUNSUPPORTED, "a model that mixes user-written profiles with GL_INTERPOL lights is not served: the run-time "
                                 "compiled kernels carry no image tables");
  m->P = p_off;
  for (int i = 0; i < n_lens; ++i) m->lens_params += m->comps[i].n_par;
  m->D = std::max(d_off, 4);
  m->A = a_off;
  m->Apad = a_off | 1;  // odd: the 16 leader lanes of a wave land on 16 different LDS banks
  for (int i = 0; i < n_lens; ++i) m->has_nfw = m->has_nfw || m->comps[i].kind == K_NFW;
  m->nfw_lds = m->has_nfw ? sizeof(float) * 2 * glh::kNfwNodes : 0;  // the h(X) table rides in every main kernel's LDS
  m->ncols = ((size_t)(((m->D + 3) & ~3) + 64 * m->Apad) * sizeof(float) + m->nfw_lds <= 60 * 1024) ? 64 : 16;
  return GL_OK;
}

// Every GIGALENS_HIP_* variable, read once at model creation, one line each: what the calls look at later goes into the model,
// what only the steps of the creation look at into Knobs.
struct Knobs {
  int tile, tile_grad, use_static, pair, shp, cluster, corr_pair;
};
Knobs read_env_knobs(gl_model* m) {
  Knobs k{};
  k.tile = env_int("GIGALENS_HIP_TILE", 0);                 // pixels per thread per tile: 1, 2 or 4 (0: the kernel's own choice)
  k.tile_grad = env_int("GIGALENS_HIP_TILE_GRAD", k.tile);  // ... of the gradient launches (default: GIGALENS_HIP_TILE)
  k.use_static = env_int("GIGALENS_HIP_STATIC", 1);         // 0: the interpreter kernel for every composition
  m->static_variant = env_int("GIGALENS_HIP_STATIC_VARIANT", 0);
  k.pair = env_int("GIGALENS_HIP_PAIR", 1);                 // 0: no pixel-pair form of the specialised kernels
  k.shp = env_int("GIGALENS_HIP_SHP", 1);                   // 0: the round-2 kernels for one-shapelet-source models
  k.cluster = env_int("GIGALENS_HIP_CLUSTER", -1);          // 0: no cluster kernel; 1 / 2: its pixel-split / component-per-wave form for every cluster model
  m->target_wgs = std::max(1, env_int("GIGALENS_HIP_TARGET_WGS", 2048));
  m->target_wgs_set = getenv("GIGALENS_HIP_TARGET_WGS") != nullptr;
  m->use_order = env_int("GIGALENS_HIP_ORDER", 1) != 0;
  m->order_fused = env_int("GIGALENS_HIP_ORDER_FUSED", 1) != 0;  // tests: 0 = the sort as a launch of its own (gl_order_kernel)
  m->prep_lds = env_int("GIGALENS_HIP_PREP_LDS", 1) != 0;  // tests: 0 = the front end reads the parameter row back from global memory
  m->tail_rows = env_int("GIGALENS_HIP_TAIL_ROWS", -1);  // -1: twice the chunks; 0: no tapered end; n: n workgroups per tail sample
  m->tail_n = env_int("GIGALENS_HIP_TAIL_N", -1);        // -1: the remainder beyond whole rounds; n: the last n samples
#ifdef GL_EXPERIMENTS
  // dissection builds only (hipcc -DGL_EXPERIMENTS; never __graft_entry__.build()): work-skipping flags and a raw chunk size
  m->chunk_px_override = env_int("GIGALENS_HIP_CHUNK_PX", 0);
  m->dbg_flags = env_int("GIGALENS_HIP_DBGFLAGS", 0);
#endif
  m->shp_cull = env_int("GIGALENS_HIP_SHP_CULL", 1);
  m->shp_blocked = env_int("GIGALENS_HIP_SHP_BLOCKED", 1);
  m->corr_max_pairs = env_int("GIGALENS_HIP_CORR_MAXPAIRS", 0);  // tests: force the slicing of the PSF launches (read once)
  m->corr_wide = env_int("GIGALENS_HIP_CORR_WIDE", 1);           // 0: 8 outputs per thread in the stride-2 forward correlation as well
  k.corr_pair = env_int("GIGALENS_HIP_CORR_PAIR", 1);            // 0: the tap kernels for every PSF (no register-blocked pair kernel)
  m->wave_prep = env_int("GIGALENS_HIP_WAVE_PREP", 1) != 0;
  m->lstsq_wgs = std::max(1, env_int("GIGALENS_HIP_LSTSQ_WGS", 2048));
  m->lstsq_chol = env_int("GIGALENS_HIP_LSTSQ_CHOL", 1) != 0;    // tests: 0 = every system through the eigenvalue solve
  m->lstsq_fused = env_int("GIGALENS_HIP_LSTSQ_FUSED", 1) != 0;  // tests: 0 = the linear solve through the basis stack (read once)
  return k;
}

// the dissection knobs: checked in an experiment build, refused in the shipped one
int check_experiment_knobs(const gl_model* m) {
#ifdef GL_EXPERIMENTS
  if (m->chunk_px_override < 0 || m->chunk_px_override % (WG * 4) != 0)
    return fail(GL_EINVAL, "GIGALENS_HIP_CHUNK_PX=%d is not a positive multiple of the tile (%d pixels)", m->chunk_px_override, WG * 4);
  if (m->dbg_flags || m->chunk_px_override)
    fprintf(stderr, "libgigalens_hip: EXPERIMENT BUILD with GIGALENS_HIP_DBGFLAGS=%d GIGALENS_HIP_CHUNK_PX=%d -- results are not valid\n",
            m->dbg_flags, m->chunk_px_override);
#else
  // the shipped library has no work-skipping paths: a stray dissection variable is an error, not a silently ignored hint
  (void)m;
  for (const char* name : {"GIGALENS_HIP_DBGFLAGS", "GIGALENS_HIP_CHUNK_PX"}) {
    const char* v = getenv(name);
    if (v && *v && atoi(v) != 0)
      return fail(GL_EINVAL, "%s is set but this library was built without -DGL_EXPERIMENTS (the dissection knobs do not exist in it)", name);
  }
#endif
  return GL_OK;
}

// which main kernel serves the model: a specialised composition (and its pair / shapelet forms), the cluster kernels or the
// interpreter, and the tile each launches with
int select_kernels(gl_model* m, const Knobs& k) {
  const int n_comp = (int)m->comps.size(), n_lens = m->n_lens, n_lens_light = m->n_ll, n_src = m->n_src;
  m->tile = (k.tile == 4 || k.tile == 1) ? k.tile : 2;
  m->tile_grad = (k.tile_grad == 4 || k.tile_grad == 1 || k.tile_grad == 2) ? k.tile_grad : 0;
  m->static_id = k.use_static ? match_static(m) : 0;
  if (m->has_user) {  // the run-time compiled interpreter serves the whole model
    m->static_id = 0;
    if (m->shp_big) return fail(GL_EUNSUPPORTED, "user-written profiles beside shapelets with n_max > %d", SH_CAP);
  }
  if (m->shp_big) {  // orders above SH_CAP: the runtime-order interpreter variant only (compiled for the basic profile families)
    m->static_id = 0;
    if (m->fam)
      return fail(GL_EUNSUPPORTED, "shapelets with n_max > %d are served together with EPL / SIE / NFW / Shear / SIS lenses and Sersic "
                                   "lights only (this model also holds dPIE-family, catalogue, series or extended profiles)", SH_CAP);
  }
  m->pair = k.pair;
  // the pair kernels' epilogue addresses the accumulator row in closed form: [NSTAT | components in order, static_nacc each];
  // gl_shp.hip.h addresses it as [NSTAT | lenses | lens lights | shapelet] and needs a table-mode model's pair table
  int off = NSTAT;
  bool ok_row = true;
  for (int i = 0; i < n_comp; ++i) {
    ok_row = ok_row && m->comps[i].a_off == off;
    off += static_nacc(m->comps[i].kind);
  }
  if (m->pair && m->static_id && (!ok_row || off != m->A)) m->pair = 0;
  m->shp_kernel = k.shp && k.pair && m->static_id && ok_row && n_src == 1 && m->comps.back().kind == K_SHAPELETS;
  m->light_spherical = n_comp > n_lens;
  for (int i = n_lens; i < n_comp; ++i) m->light_spherical = m->light_spherical && m->comps[i].kind == K_SERSIC;
  m->static_matched = m->static_id;
  if (!m->tile_grad) m->tile_grad = m->static_id ? 1 : 2;  // measured: T=1 wins once the VJP state lives in registers
  if (!m->static_id) {  // the interpreter kernel is built for T = 2 and 4
    if (!k.tile && !m->has_epl && !m->has_shapelets && !m->fam) m->tile = 4;  // cheap profiles, forward modes: amortise the per-tile work
    if (m->tile == 1) m->tile = 2;
    if (m->tile_grad == 1) m->tile_grad = 2;
  }
  if (k.cluster && !m->static_id && !m->has_user && n_lens_light == 0 && n_lens >= 1 && n_lens <= 8 && n_src >= 1 &&
      n_src <= 20 && (size_t)64 * m->Apad * sizeof(float) <= 64 * 1024) {
    bool ok_c = true, ell = false;
    for (int i = 0; i < n_lens; ++i) ok_c = ok_c && m->comps[i].kind == K_NFW;
    for (int i = n_lens; i < n_comp; ++i) {
      ok_c = ok_c && (m->comps[i].kind == K_SERSIC || m->comps[i].kind == K_SERSIC_ELLIPSE);
      ell = ell || m->comps[i].kind == K_SERSIC_ELLIPSE;
    }
    // the kernel addresses the derived / accumulator blocks in closed form: component-major, fixed block sizes
    constexpr int NFWP = (NFW_ND + 3) & ~3, SERP = (SER_NDX + 3) & ~3;  // the strides gl_cluster_kernel walks the derived row with
    for (int i = 0; i < n_lens && ok_c; ++i) ok_c = m->comps[i].d_off == NFWP * i && m->comps[i].a_off == NSTAT + NFW_NACC * i;
    for (int i = 0; i < n_src && ok_c; ++i)
      ok_c = m->comps[n_lens + i].d_off == NFWP * n_lens + SERP * i && m->comps[n_lens + i].a_off == NSTAT + NFW_NACC * n_lens + SER_NACC * i;
    ok_c = ok_c && (size_t)64 * m->Apad * sizeof(float) + sizeof(float) * 2 * glh::kNfwNodes <= 64 * 1024;
    if (ok_c) m->cluster = ell ? 2 : 1;
    // ... in its component-per-wave form (gl_clusterw.hip.h) when the model fills at least 60 % of the component slots of the
    // instantiation that holds it (4 waves x (1 + 2), (2 + 3) or (2 + 5) halos + sources): an unused slot is evaluated all the same.
    // GIGALENS_HIP_CLUSTER: 1 = the pixel-split kernel for every cluster model, 2 = the component-per-wave kernel for every one
    if (m->cluster) {
      const int cap = (n_lens <= 4 && n_src <= 8) ? 12 : (n_src <= 12 ? 20 : 28);
      m->cluster_w = k.cluster == 2 || (k.cluster != 1 && 10 * (n_lens + n_src) >= 6 * cap);
    }
  }
  return GL_OK;
}

// the uploads of the creation: every failure of one reports the same way
int create_failed() { return fail(GL_ENOMEM, "device allocation / upload failed in gl_model_create"); }
template <class T>
int put(DevBuf<T>& buf, const T* src, size_t n) {
  return buf.upload(src, n) == hipSuccess ? GL_OK : create_failed();
}

// component table, pixel grid, linear columns and pixel list on the device
int upload_grid(gl_model* m, const gl_grid* grid) {
  int rc;
  if (m->comps.empty()) {  // (a model without components still hands the kernels a table)
    if (m->d_comps.alloc(1) != hipSuccess) return create_failed();
  } else if ((rc = put(m->d_comps, m->comps.data(), m->comps.size()))) {
    return rc;
  }
  if ((rc = put(m->d_gx, grid->grid_x, m->N))) return rc;
  for (int i = 0; i < m->N; ++i) m->grid_rmax = std::max(m->grid_rmax, std::hypot(grid->grid_x[i], grid->grid_y[i]));
  if ((rc = put(m->d_gy, grid->grid_y, m->N))) return rc;
  if (!m->lin_cols.empty() && (rc = put(m->d_lin_cols, m->lin_cols.data(), m->lin_cols.size()))) return rc;
  if (grid->pix_index) {
    for (int i = 0; i < m->N; ++i)
      if (grid->pix_index[i] < 0 || grid->pix_index[i] >= m->height * m->width)
        return fail(GL_EINVAL, "pix_index[%d]=%d out of range", i, grid->pix_index[i]);
    if ((rc = put(m->d_pix, grid->pix_index, m->N))) return rc;
  }
  return GL_OK;
}

// the NFW h(X) tables and the shapelet node table of the models that interpolate
int upload_tables(gl_model* m) {
  int rc;
  if (m->has_nfw) {
    // [h(X) node table | neutral blocks | H(s) cubics]: the layout gl_clusterw_kernel addresses (CW_NEUTRAL_OFF, CW_TABS_OFF)
    std::vector<float> tab;
    glh::build_nfw_table([](double X, double& g, double& gp) { glp::nfw_gw<double>(X, g, gp); }, tab);
    // behind the table: the constant blocks of an unused component slot of gl_clusterw_kernel (zero amplitude, all else finite)
    const float neutral_nfw[4] = {0.f, 0.f, 1.f, 0.f};  // NFW_CX, NFW_CY, NFW_INVRS, NFW_K0
    float neutral_ser[16] = {0.f};
    neutral_ser[glp::SER_C] = neutral_ser[glp::SER_SQ] = neutral_ser[glp::SER_ISQ] = neutral_ser[glp::SER_INVRS] = 1.f;
    neutral_ser[glp::SER_INVN] = neutral_ser[glp::SER_IRS2] = 1.f;
    neutral_ser[glp::SER_BN] = 1.6721f;  // n = 1; SER_IE = SER_CG = 0
    tab.insert(tab.end(), neutral_nfw, neutral_nfw + 4);
    tab.insert(tab.end(), neutral_ser, neutral_ser + 16);
    // ... and the table of the same function in s = X^2 (gl_host_tables.h::build_nfw_table_s), [4][kNfwSIntervals]
    std::vector<float> tab_s;
    glh::build_nfw_table_s([](double X, double& g, double& gp) { glp::nfw_gw<double>(X, g, gp); }, tab_s);
    tab.insert(tab.end(), tab_s.begin(), tab_s.end());
    if ((rc = put(m->d_nfw_tab, tab.data(), tab.size()))) return rc;
  }
  if (m->has_table) {
    // the full n_max = 10 table (stride 12, two rows of a node pair = six aligned float4), or -- for a model with orders above
    // 10, whose shapelet components all run the runtime-order path -- the n_max = 20 one (stride 24)
    std::vector<float> tab;
    glh::build_shapelet_table(m->shp_big ? SH_CAPB : SH_CAP, tab, &m->shp_stride);
    if ((rc = put(m->d_shp_tab, tab.data(), tab.size()))) return rc;
  }
  return GL_OK;
}

// Plans of the register-blocked pair kernel (gl_post.hip.h gl_corr_pair_kernel): forward = one class (stride ss, Keff), transpose =
// ss^2 residue classes (stride 1, the class's decimated and flipped sub-kernel); rows padded to a multiple of four taps.  Each
// appends its padded kernels to kbuf.
int pad4(int n) { return std::max(4, (n + 3) & ~3); }
void plan_corr_fwd(gl_model* m, const std::vector<double>& keff, std::vector<float>& kbuf) {
  const int ss = m->supersample, Hs = m->height, Ws = m->width, H = Hs / ss, W = Ws / ss;
  gl_model::CorrPlan& f = m->corr_fwd;
  f.KWP = pad4(m->KW);
  f.ST = ss;
  CorrClass c{};
  c.koff = 0; c.KH = m->KH; c.pt = m->pad_t; c.pl = m->pad_l; c.Ho = H; c.Wo[0] = W; c.oo_r = 0; c.oo_c[0] = 0;
  kbuf.assign((size_t)m->KH * f.KWP, 0.f);
  for (int u = 0; u < m->KH; ++u)
    for (int v = 0; v < m->KW; ++v) kbuf[(size_t)u * f.KWP + v] = (float)keff[(size_t)u * m->KW + v];
  f.args.n_class = 1; f.args.ncj = 1; f.args.Hi = Hs; f.args.Wi = Ws; f.args.Hout = H; f.args.Wout = W; f.args.os = 1;
  f.args.cls[0] = c;
  f.max_Ho = H; f.max_Wo = W; f.max_KH = m->KH; f.ok = true;
}
void plan_corr_bwd(gl_model* m, const std::vector<double>& keff, std::vector<float>& kbuf) {
  // transpose: row class pi = (i + pt) mod ss -> one workgroup family; its ss column classes pj share a thread.  Class
  // (pi, pj): outputs i = ss n + ri, j = ss q + rj;  gS = sum_{t, s} gP[n + t - padT][q + s - padL] Kf[t][s] with the
  // flipped decimated kernel Kf[t][s] = Keff[pi + ss (A - 1 - t)][pj + ss (C - 1 - s)].  The column classes' left
  // paddings differ by at most one: they are levelled to the largest by shifting the kernel right.
  const int ss = m->supersample, Hs = m->height, Ws = m->width, H = Hs / ss, W = Ws / ss;
  gl_model::CorrPlan& g = m->corr_bwd;
  g.ST = 1;
  g.args.n_class = ss; g.args.ncj = ss; g.args.Hi = H; g.args.Wi = W; g.args.Hout = Hs; g.args.Wout = Ws; g.args.os = ss;
  int Cn[4], rjn[4], pln[4], max_pl = -(1 << 30), width = 1;
  for (int pj = 0; pj < ss; ++pj) {
    Cn[pj] = m->KW > pj ? (m->KW - pj + ss - 1) / ss : 0;
    rjn[pj] = ((pj - m->pad_l) % ss + ss) % ss;
    pln[pj] = (Cn[pj] - 1) - (rjn[pj] + m->pad_l - pj) / ss;
    max_pl = std::max(max_pl, pln[pj]);
  }
  for (int pj = 0; pj < ss; ++pj) width = std::max(width, Cn[pj] + (max_pl - pln[pj]));
  g.KWP = pad4(width);
  // column classes ordered by their output offset, so Wo[0] is the largest
  int order[4];
  for (int pj = 0; pj < ss; ++pj) order[rjn[pj]] = pj;
  for (int pi = 0; pi < ss; ++pi) {
    const int A = m->KH > pi ? (m->KH - pi + ss - 1) / ss : 0;
    const int ri = ((pi - m->pad_t) % ss + ss) % ss;
    CorrClass c{};
    c.koff = (int)kbuf.size();
    c.KH = A;
    c.pt = (A - 1) - (ri + m->pad_t - pi) / ss;
    c.pl = max_pl;
    c.Ho = ri < Hs ? (Hs - ri + ss - 1) / ss : 0;
    c.oo_r = ri;
    kbuf.resize(kbuf.size() + (size_t)A * ss * g.KWP, 0.f);
    for (int jj = 0; jj < ss; ++jj) {
      const int pj = order[jj], C = Cn[pj], sh = max_pl - pln[pj];
      c.Wo[jj] = rjn[pj] < Ws ? (Ws - rjn[pj] + ss - 1) / ss : 0;
      c.oo_c[jj] = rjn[pj];
      for (int t = 0; t < A; ++t)
        for (int q = 0; q < C; ++q)
          kbuf[(size_t)c.koff + ((size_t)t * ss + jj) * g.KWP + sh + q] =
              (float)keff[(size_t)(pi + ss * (A - 1 - t)) * m->KW + (pj + ss * (C - 1 - q))];
    }
    g.args.cls[pi] = c;
    g.max_Ho = std::max(g.max_Ho, c.Ho); g.max_Wo = std::max(g.max_Wo, c.Wo[0]); g.max_KH = std::max(g.max_KH, c.KH);
  }
  g.ok = true;
}

// PSF and pooling: the effective kernel flip(psf) (*) box(ss)/ss^2 of the tap kernels and, where it serves, the pair kernel's plans
int build_post(gl_model* m, const gl_grid* grid, const Knobs& k) {
  m->has_post = grid->psf != nullptr || grid->supersample != 1;
  if (!m->has_post) return GL_OK;
  // flat = flip(psf) cross-correlated with SAME padding (tf/simulator.py:62-70,145-147), then box(ss)/ss^2 pooling
  const int kh = grid->psf ? grid->psf_h : 1, kw = grid->psf ? grid->psf_w : 1, ss = grid->supersample;
  m->psf_h = kh;
  m->psf_w = kw;
  m->KH = kh + ss - 1;
  m->KW = kw + ss - 1;
  m->pad_t = (kh - 1) / 2;
  m->pad_l = (kw - 1) / 2;
  std::vector<double> keff((size_t)m->KH * m->KW, 0.0);
  for (int u = 0; u < kh; ++u)
    for (int v = 0; v < kw; ++v) {
      double f = grid->psf ? (double)grid->psf[(size_t)(kh - 1 - u) * kw + (kw - 1 - v)] : 1.0;
      for (int a2 = 0; a2 < ss; ++a2)
        for (int c2 = 0; c2 < ss; ++c2) keff[(size_t)(u + a2) * m->KW + (v + c2)] += f / (double)(ss * ss);
    }
  std::vector<float> kf(keff.begin(), keff.end());
  if (int rc = put(m->d_psf, kf.data(), kf.size())) return rc;
  if (k.corr_pair && ss <= 2 && m->KW <= 32 && m->KH <= 64) {
    std::vector<float> kbuf;
    plan_corr_fwd(m, keff, kbuf);
    plan_corr_bwd(m, keff, kbuf);
    if (int rc = put(m->d_corr_k, kbuf.data(), kbuf.size())) return rc;
    m->corr_fwd.args.k = m->corr_bwd.args.k = m->d_corr_k;
  }
  return GL_OK;
}
}  // namespace

extern "C" {

const char* gl_last_error(void) { return g_err; }
const char* gl_version(void) { return "gigalens_hip 0.1 (gfx950)"; }

int gl_kind_num_params(const gl_component* comp) {
  if (!comp) return fail(GL_EINVAL, "component is null");
  int n = kind_num_params(comp->kind, comp->iparam);
  if (n < 0) return fail(GL_EINVAL, "unknown profile kind %d (iparam %d)", comp->kind, comp->iparam);
  return n;
}

int gl_model_create(const gl_component* comps, int n_lens, int n_lens_light, int n_src, const gl_grid* grid,
                    gl_model** out) {
  return gl_model_create_user(comps, n_lens, n_lens_light, n_src, grid, nullptr, 0, out);
}

int gl_model_create_user(const gl_component* comps, int n_lens, int n_lens_light, int n_src, const gl_grid* grid,
                         const char* const* bodies, int n_bodies, gl_model** out) {
  if (!out) return fail(GL_EINVAL, "out is null");
  if (n_bodies < 0 || (n_bodies > 0 && !bodies)) return fail(GL_EINVAL, "bad user bodies");
  *out = nullptr;
  int rc;
  if ((rc = check_create_args(comps, n_lens, n_lens_light, n_src, grid))) return rc;
  // (the deleter is gl_model_destroy: every early return below leaves nothing behind)
  std::unique_ptr<gl_model, ModelDeleter> m(new (std::nothrow) gl_model());
  if (!m) return fail(GL_ENOMEM, "host allocation failed");
  m->n_lens = n_lens;
  m->n_ll = n_lens_light;
  m->n_src = n_src;
  if ((rc = build_components(m.get(), comps, n_lens + n_lens_light + n_src, bodies, n_bodies))) return rc;
  m->height = grid->height;
  m->width = grid->width;
  m->supersample = grid->supersample;
  m->N = grid->n_region;
  m->conversion_factor = grid->conversion_factor;
  const Knobs knobs = read_env_knobs(m.get());
  if ((rc = select_kernels(m.get(), knobs))) return rc;
  if ((rc = check_experiment_knobs(m.get()))) return rc;
  size_t shmem = (size_t)(((m->D + 3) & ~3) + m->ncols * m->Apad) * sizeof(float) + m->nfw_lds;
  if (shmem > 64 * 1024) return fail(GL_EUNSUPPORTED, "model needs %zu B of LDS per workgroup (> 64 KiB)", shmem);
  if ((rc = upload_grid(m.get(), grid))) return rc;
  if ((rc = upload_tables(m.get()))) return rc;
  if ((rc = build_post(m.get(), grid, knobs))) return rc;
  if (m->has_user) {  // the interpreter kernel with the user's bodies inside, compiled now (a few seconds, once per model)
    m->tile = 2;
    m->tile_grad = 2;
    if ((rc = compile_user_model(m.get(), bodies, n_bodies))) return rc;
  }
  *out = m.release();
  return GL_OK;
}

int gl_model_set_timing(gl_model* m, int slots) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (slots < 0 || slots > 65536) return fail(GL_EINVAL, "timing slots %d outside [0, 65536]", slots);
  for (hipEvent_t e : m->evs) (void)hipEventDestroy(e);
  m->evs.clear();
  m->timing_slots = 0;
  m->timing_count = 0;
  m->timing_calls = 0;
  m->evs.reserve((size_t)2 * slots);
  for (int i = 0; i < 2 * slots; ++i) {
    hipEvent_t e;
    GL_HIP(hipEventCreate(&e));
    m->evs.push_back(e);
  }
  m->timing_slots = slots;
  return GL_OK;
}

int gl_model_set_timing_stride(gl_model* m, int stride) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (stride < 1) return fail(GL_EINVAL, "stride must be >= 1");
  m->timing_stride = stride;
  m->timing_calls = 0;
  return GL_OK;
}

int gl_model_last_main_ms(gl_model* m, float* ms) {
  if (!m || !ms) return fail(GL_EINVAL, "null argument");
  if (!m->timing_slots || !m->timing_count) return fail(GL_EINVAL, "no timed main launch on this model");
  const int slot = (int)((m->timing_count.load() - 1) % m->timing_slots);
  GL_HIP(hipEventSynchronize(m->evs[2 * slot + 1]));
  GL_HIP(hipEventElapsedTime(ms, m->evs[2 * slot], m->evs[2 * slot + 1]));
  return GL_OK;
}

int gl_model_timing_drain(gl_model* m, float* ms, int cap, int* n_out) {
  if (!m || !ms || !n_out || cap < 0) return fail(GL_EINVAL, "bad argument");
  *n_out = 0;
  if (!m->timing_slots) return fail(GL_EINVAL, "timing is not enabled on this model");
  const long long count = m->timing_count.load();
  const long long have = std::min<long long>(count, m->timing_slots);
  const long long first = count - have;  // oldest launch still in the ring
  int n = 0;
  for (long long k = first; k < count && n < cap; ++k, ++n) {
    const int slot = (int)(k % m->timing_slots);
    GL_HIP(hipEventSynchronize(m->evs[2 * slot + 1]));
    GL_HIP(hipEventElapsedTime(&ms[n], m->evs[2 * slot], m->evs[2 * slot + 1]));
  }
  *n_out = n;
  m->timing_count = 0;
  m->timing_calls = 0;
  return GL_OK;
}

int gl_model_last_main_kernel(const gl_model* m, char* buf, size_t cap) {
  if (!m || !buf || cap == 0) return fail(GL_EINVAL, "bad argument");
  if (m->last_main_user >= 0) {  // a model with user-written profiles: a run-time compiled kernel (gl_user.hip)
    const int u = m->last_main_user.load();
    if (u >= 16)
      snprintf(buf, cap, "gl_pair_kernel<%d, v2f, 2, KindList<the model's own component list>...> [run-time compiled with the model's user-written profile bodies]", u - 16);
    else
      snprintf(buf, cap, "gl_main_kernel<%d, 2, %s, %d> [run-time compiled with the model's user-written profile bodies]", u,
               m->has_shapelets ? "true" : "false", m->fam);
    return GL_OK;
  }
  if (!m->last_main_fn) return fail(GL_EINVAL, "no main kernel has been launched on this model yet");
  const char* name = hipKernelNameRefByPtr(m->last_main_fn.load(), nullptr);
  if (!name) return fail(GL_ELAUNCH, "hipKernelNameRefByPtr returned no name");
  snprintf(buf, cap, "%s", name);
  return GL_OK;
}

int gl_model_last_post_kernel(const gl_model* m, int transpose, char* buf, size_t cap) {
  if (!m || !buf || cap == 0 || (transpose != 0 && transpose != 1)) return fail(GL_EINVAL, "bad argument");
  const void* fn = m->last_post_fn[transpose].load();
  if (!fn) return fail(GL_EINVAL, "no %s post-processing kernel has been launched on this model yet", transpose ? "transposed" : "forward");
  const char* name = hipKernelNameRefByPtr(fn, nullptr);
  if (!name) return fail(GL_ELAUNCH, "hipKernelNameRefByPtr returned no name");
  snprintf(buf, cap, "%s", name);
  return GL_OK;
}

int gl_post_apply(const gl_model* m, int B, const float* in, float* out, int transpose, float scale, void* hip_stream) {
  if (!m || !in || !out) return fail(GL_EINVAL, "null argument");
  if (B <= 0) return fail(GL_EINVAL, "B must be positive");
  if (transpose != 0 && transpose != 1) return fail(GL_EINVAL, "transpose must be 0 or 1");
  if (!m->has_post) return fail(GL_EINVAL, "the model has no PSF and no supersampling: there is no post-processing to apply");
  hipStream_t stream = (hipStream_t)hip_stream;
  return transpose ? post_bwd(m, B, in, out, stream, scale) : post_fwd(m, B, in, out, stream, scale);
}

int gl_model_launch_shape(const gl_model* m, int B, int* chunk_px, int* n_chunks, int* row_floats, size_t* partial_offset_bytes) {
  if (!m || B < 1) return fail(GL_EINVAL, "bad argument");
  const LaunchPlan plan = launch_plan(m, B);
  const Workspace w = carve(m, B, nullptr, plan);
  if (chunk_px) *chunk_px = plan.chunk;
  if (n_chunks) *n_chunks = plan.n_rows;  // partial rows a sample owns (the chunks, or the workgroups of a tail sample if more: tail_plan)
  if (row_floats) *row_floats = m->A;
  if (partial_offset_bytes) *partial_offset_bytes = (size_t)((const char*)w.partial - (const char*)nullptr);
  return GL_OK;
}

void gl_model_destroy(gl_model* m) {  // (the device buffers go with their owners: glk::DevBuf)
  if (!m) return;
  if (m->user_module) (void)hipModuleUnload(m->user_module);
  if (m->user_point_module) (void)hipModuleUnload(m->user_point_module);
  for (hipEvent_t e : m->evs) (void)hipEventDestroy(e);
  delete m;
}

int gl_model_num_params(const gl_model* m) { return m ? m->P : fail(GL_EINVAL, "model is null"); }
int gl_model_param_offset(const gl_model* m, int component) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (component < 0 || component >= (int)m->comps.size()) return fail(GL_EINVAL, "component index out of range");
  return m->comps[component].p_off;
}
int64_t gl_model_num_pixels(const gl_model* m) { return m ? m->N : fail(GL_EINVAL, "model is null"); }

size_t gl_workspace_bytes(const gl_model* m, int B) {
  if (!m || B <= 0) return 0;
  return carve(m, B, nullptr, launch_plan(m, B)).bytes;
}

int gl_simulate_fwd(const gl_model* m, const float* params, int B, float* img, void* workspace,
                    size_t workspace_bytes, void* hip_stream) {
  return gl_simulate_parts_fwd(m, params, B, 7u, img, workspace, workspace_bytes, hip_stream);  // every part
}

int gl_simulate_parts_fwd(const gl_model* m, const float* params, int B, unsigned parts, float* img, void* workspace,
                          size_t workspace_bytes, void* hip_stream) {
  if (int rp = refuse_planes(m, "gl_simulate_parts_fwd")) return rp;
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w);
  if (rc) return rc;
  if (!img) return fail(GL_EINVAL, "img is null");
  if (parts == 0 || parts > 7u) return fail(GL_EINVAL, "parts must be a non-empty subset of {1,2,4}");
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = run_prep(m, params, nullptr, B, plan, w, stream))) return rc;
  MainArgs a = base_args(m, w, plan.chunk);
  a.parts = parts;
  if ((rc = run_order(m, B, w, &a, stream))) return rc;
  if (m->has_post) {
    if ((rc = render_ss(m, a, B, plan.n_chunks, w, stream))) return rc;
    return post_fwd(m, B, w.img_ss, img, stream, m->conversion_factor);
  }
  if (m->d_pix) GL_HIP(hipMemsetAsync(img, 0, sizeof(float) * (size_t)B * m->height * m->width, stream));
  a.img = img;
  return launch_main<IMG_FWD>(m, a, B, plan.n_chunks, stream);
}

int gl_simulate_bwd(const gl_model* m, const float* params, const float* grad_img, int B, float* grad_params,
                    void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rp = refuse_planes(m, "gl_simulate_bwd")) return rp;
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w);
  if (rc) return rc;
  if (!grad_img || !grad_params) return fail(GL_EINVAL, "grad_img / grad_params is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = run_prep(m, params, nullptr, B, plan, w, stream))) return rc;
  MainArgs a = base_args(m, w, plan.chunk);
  a.gimg = grad_img;
  if (m->has_post) {
    if ((rc = post_bwd(m, B, grad_img, w.img_ss, stream, m->conversion_factor))) return rc;
    a.gimg = w.img_ss;
    a.out_scale = 1.f;
  }
  if ((rc = run_order(m, B, w, &a, stream))) return rc;
  if ((rc = launch_main<IMG_BWD>(m, a, B, plan.n_chunks, stream))) return rc;
  return run_finalize(m, params, B, plan.n_chunks, w, nullptr, nullptr, grad_params, stream);
}

int gl_loglike_fwd_bwd(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                       const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                       float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rp = refuse_planes(m, "gl_loglike_fwd_bwd")) return rp;
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w);
  if (rc) return rc;
  if (!obs || !loglike || !chi2) return fail(GL_EINVAL, "obs / loglike / chi2 is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = run_prep(m, params, nullptr, B, plan, w, stream))) return rc;
  const float* extra = nullptr;
  int use_partial = 1, fin_rows = plan.n_chunks;
  if ((rc = run_likelihood(m, B, plan, w, obs, err_or_null, mask_or_null, bg_rms, exp_time,
                           grad_params_or_null != nullptr, stream, &extra, &use_partial, &fin_rows)))
    return rc;
  return run_finalize(m, params, B, fin_rows, w, loglike, chi2, grad_params_or_null, stream, nullptr, nullptr, nullptr,
                      1.f, extra, use_partial);
}

int gl_model_num_linear(const gl_model* m) { return m ? (int)m->lin_cols.size() : fail(GL_EINVAL, "model is null"); }
int gl_model_linear_column(const gl_model* m, int k) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (k < 0 || k >= (int)m->lin_cols.size()) return fail(GL_EINVAL, "linear coefficient index out of range");
  return m->lin_cols[k];
}

namespace {
// what the solve half of the linear-amplitude step needs of a workspace
struct SolveWs {
  float* partial;  // [B][n_chunks][Dp*Dp]
  float* mats;     // [B][2][D][D | 1] above LS_LDS_MAXN unknowns, else null
  int* todo;       // [B]
  int Dp, chunk, n_chunks;
};
// host function pointers of the most recent solve's normal-matrix, Cholesky and eigen kernel (null: the stage did not run)
std::atomic<const void*> g_lstsq_last_fn[3];
#define GL_LS_LAUNCH(slot_, kernel_, ...)                      \
  do {                                                         \
    g_lstsq_last_fn[slot_] = (const void*)&kernel_;            \
    hipLaunchKernelGGL((kernel_), __VA_ARGS__);                \
  } while (0)

// The solve of gl_lstsq_fwd and gl_lstsq_solve_stack: normal matrices of [stack / err | obs / err] per (sample, pixel chunk) --
// unless the stack-free kernel already left them (`have_partials`) --, their sum, the Cholesky attempt, the eigenvalue solve.
int lstsq_solve(const float* stack, const float* obs, const float* err, int B, int D, int HW, const SolveWs& sw,
                bool have_partials, bool chol, float* coeffs, hipStream_t stream) {
  int rc;
  NormalArgs na{};
  na.stack = stack;
  na.obs = obs;
  na.err = err;
  na.D = D;
  na.Dp = sw.Dp;
  na.HW = HW;
  na.chunk = sw.chunk;
  na.n_chunks = sw.n_chunks;
  na.partial = sw.partial;
  if (have_partials) {
    // the partials are already there
  } else if (D + 1 <= LS_SMALL)
    GL_LS_LAUNCH(0, gl_normal_small_kernel<LS_SMALL>, dim3(sw.n_chunks, B), dim3(256), 0, stream, na);
  else if (D + 1 > LS_MAXD) {  // more than five tile rows: super-block pairs (gl_normal_pair_kernel)
    const int vec_ok = (HW % 4 == 0) && ((uintptr_t)obs % 16 == 0) && ((uintptr_t)err % 16 == 0) && ((uintptr_t)stack % 16 == 0);
    const int n_sb = (D + 1 + 16 * LS_SB - 1) / (16 * LS_SB);
    const dim3 grid(sw.n_chunks, B, n_sb * (n_sb + 1) / 2), block(256);
    if (vec_ok) GL_LS_LAUNCH(0, gl_normal_pair_kernel<true>, grid, block, 0, stream, na);
    else GL_LS_LAUNCH(0, gl_normal_pair_kernel<false>, grid, block, 0, stream, na);
  } else {
    // 16-byte loads need every channel row, obs and err on a 16-byte pitch
    const int vec_ok = (HW % 4 == 0) && ((uintptr_t)obs % 16 == 0) && ((uintptr_t)err % 16 == 0) && ((uintptr_t)stack % 16 == 0);
    const dim3 grid(sw.n_chunks, B), block(256);
#define GL_NORMAL_MFMA(NT_)                                                                                  \
  if (vec_ok) GL_LS_LAUNCH(0, (gl_normal_mfma_kernel<NT_, true>), grid, block, 0, stream, na);               \
  else GL_LS_LAUNCH(0, (gl_normal_mfma_kernel<NT_, false>), grid, block, 0, stream, na)
    switch ((D + 1 + 15) / 16) {
      case 1: GL_NORMAL_MFMA(1); break;
      case 2: GL_NORMAL_MFMA(2); break;
      case 3: GL_NORMAL_MFMA(3); break;
      case 4: GL_NORMAL_MFMA(4); break;
      default: GL_NORMAL_MFMA(5); break;
    }
#undef GL_NORMAL_MFMA
  }
  GL_HIP(hipGetLastError());
  int n_sum = sw.n_chunks;
  if (n_sum > 8) {  // many chunks (small batches): reduce them with the whole chip first
    hipLaunchKernelGGL(gl_partial_sum_kernel, dim3((sw.Dp * sw.Dp + 255) / 256, B), dim3(256), 0, stream, sw.partial,
                       sw.n_chunks, sw.Dp * sw.Dp);
    GL_HIP(hipGetLastError());
    n_sum = 1;
  }
  const int* todo = nullptr;
  g_lstsq_last_fn[1] = nullptr;
  if (D <= LS_LDS_MAXN && chol) {  // the inverse when the pseudo-inverse's cut is provably idle (gl_chol_solve_kernel)
    const int nb = D + 1 <= 64 ? 4 : D + 1 <= 80 ? 5 : 8;
    const size_t sm = sizeof(float) * ((size_t)(D + 2) * (16 * nb + 1) + 4);
    static bool chol_raised = false;
    if (sm > 64 * 1024 && (rc = raise_lds_limit((const void*)&gl_chol_solve_kernel<8>, &chol_raised))) return rc;
#define GL_CHOL(NB_) GL_LS_LAUNCH(1, gl_chol_solve_kernel<NB_>, dim3(B), dim3(256), sm, stream, sw.partial, sw.n_chunks, n_sum, D, \
                                  sw.Dp, 1e-6f, coeffs, sw.todo)
    if (nb == 4) GL_CHOL(4); else if (nb == 5) GL_CHOL(5); else GL_CHOL(8);
#undef GL_CHOL
    GL_HIP(hipGetLastError());
    todo = sw.todo;
  }
  if (D <= LS_LDS_MAXN) {  // A and V in LDS: up to 129 KB of the CU's 160 (above 64 KB the kernel has to be told once)
    const size_t sm = sizeof(float) * ((size_t)2 * D * (D | 1) + 8 * D + 8);
    static bool eigh_raised = false;
    if (sm > 64 * 1024 && (rc = raise_lds_limit((const void*)&gl_eigh_solve_kernel<2, false>, &eigh_raised))) return rc;
    GL_LS_LAUNCH(2, (gl_eigh_solve_kernel<2, false>), dim3(B), dim3(64), sm, stream, sw.partial, sw.n_chunks, n_sum, D, sw.Dp,
                 1e-6f, coeffs, (float*)nullptr, todo);
  } else {  // the two matrices in the workspace (L2), the vectors in LDS; four registers hold the tridiagonal
    const size_t sm = sizeof(float) * ((size_t)8 * D + 8);
    GL_LS_LAUNCH(2, (gl_eigh_solve_kernel<4, true>), dim3(B), dim3(64), sm, stream, sw.partial, sw.n_chunks, n_sum, D, sw.Dp,
                 1e-6f, coeffs, sw.mats, todo);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// the workspace of gl_lstsq_solve_stack: partials, the eigen solve's matrices above LS_LDS_MAXN unknowns, the flags
SolveWs carve_solve_stack(int B, int D, int HW, int wgs, void* base, size_t* bytes) {
  SolveWs w{};
  size_t off = 0;
  char* p = (char*)base;
  auto take = [&](size_t n) { float* q = (float*)(p + off); off += align_up(n * sizeof(float), 256); return q; };
  w.Dp = (D + 1 + 3) & ~3;
  lstsq_chunks((long long)HW, B, wgs, &w.chunk, &w.n_chunks);
  w.partial = take((size_t)B * w.n_chunks * w.Dp * w.Dp);
  w.mats = D > LS_LDS_MAXN ? take((size_t)B * 2 * D * (D | 1)) : nullptr;
  w.todo = (int*)take((size_t)B);
  *bytes = off;
  return w;
}

int check_solve_stack_shape(int B, int D, int HW, int workgroups) {
  if (B <= 0 || B > 65535) return fail(GL_EINVAL, "batch size %d outside [1, 65535]", B);
  if (D <= 0 || HW <= 0 || workgroups <= 0) return fail(GL_EINVAL, "D, HW and workgroups must be positive");
  if (D > LS_MAXN) return fail(GL_EUNSUPPORTED, "%d linear coefficients exceed the %d the solve serves", D, LS_MAXN);
  return GL_OK;
}
}  // namespace

size_t gl_lstsq_solve_stack_workspace_bytes(int B, int D, int HW, int workgroups) {
  if (check_solve_stack_shape(B, D, HW, workgroups)) return 0;
  size_t bytes = 0;
  carve_solve_stack(B, D, HW, workgroups, nullptr, &bytes);
  return bytes;
}

int gl_lstsq_solve_stack(const float* stack, const float* obs, const float* err, int B, int D, int HW, int workgroups,
                         int cholesky, float* coeffs, int* flags_or_null, float* normal_or_null, void* workspace,
                         size_t workspace_bytes, void* hip_stream) {
  if (!stack || !obs || !err || !coeffs || !workspace) return fail(GL_EINVAL, "null argument");
  if (int rc = check_solve_stack_shape(B, D, HW, workgroups)) return rc;
  size_t bytes = 0;
  const SolveWs sw = carve_solve_stack(B, D, HW, workgroups, workspace, &bytes);
  if (workspace_bytes < bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  if (int rc = lstsq_solve(stack, obs, err, B, D, HW, sw, false, cholesky != 0, coeffs, stream)) return rc;
  if (flags_or_null) {  // no attempt: every system went to the eigenvalue solve
    if (cholesky && D <= LS_LDS_MAXN)
      GL_HIP(hipMemcpyAsync(flags_or_null, sw.todo, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, stream));
    else
      GL_HIP(hipMemsetD32Async((hipDeviceptr_t)flags_or_null, 1, (size_t)B, stream));
  }
  if (normal_or_null) {
    const int DpDp = sw.Dp * sw.Dp;
    // 2..8 chunks: the solve kernels summed the partials themselves; this pass repeats their additions in their order, so the
    // matrix handed out is a re-sum, bitwise equal to the values they consumed, not a copy of them
    if (sw.n_chunks > 1 && sw.n_chunks <= 8) {
      hipLaunchKernelGGL(gl_partial_sum_kernel, dim3((DpDp + 255) / 256, B), dim3(256), 0, stream, sw.partial, sw.n_chunks, DpDp);
      GL_HIP(hipGetLastError());
    }
    GL_HIP(hipMemcpy2DAsync(normal_or_null, sizeof(float) * DpDp, sw.partial, sizeof(float) * (size_t)sw.n_chunks * DpDp,
                            sizeof(float) * DpDp, (size_t)B, hipMemcpyDeviceToDevice, stream));
  }
  return GL_OK;
}

int gl_lstsq_last_kernels(char* normal, char* chol, char* eigen, size_t cap) {
  if (!normal || !chol || !eigen || cap == 0) return fail(GL_EINVAL, "bad argument");
  char* out[3] = {normal, chol, eigen};
  if (!g_lstsq_last_fn[2].load()) return fail(GL_EINVAL, "no linear solve has been launched in this process yet");
  for (int k = 0; k < 3; ++k) {
    const void* fn = g_lstsq_last_fn[k].load();
    const char* name = fn ? hipKernelNameRefByPtr(fn, nullptr) : "";
    if (!name) return fail(GL_ELAUNCH, "hipKernelNameRefByPtr returned no name");
    snprintf(out[k], cap, "%s", name);
  }
  return GL_OK;
}

size_t gl_lstsq_workspace_bytes(const gl_model* m, int B) {
  if (!m || B <= 0) return 0;
  return carve_lstsq(m, B, nullptr, carve(m, B, nullptr, launch_plan(m, B))).bytes;
}

int gl_lstsq_solve_flags(const gl_model* m, int B, size_t* offset_bytes) {
  if (!m || B <= 0 || !offset_bytes) return fail(GL_EINVAL, "bad argument");
  if ((int)m->lin_cols.size() > LS_LDS_MAXN || !m->lstsq_chol)
    return fail(GL_EUNSUPPORTED, "no Cholesky attempt for this model: every system goes through the eigenvalue solve");
  const LstsqWs lw = carve_lstsq(m, B, nullptr, carve(m, B, nullptr, launch_plan(m, B)));
  *offset_bytes = (size_t)((const char*)lw.todo - (const char*)nullptr);
  return GL_OK;
}

int gl_lstsq_fwd(const gl_model* m, const float* params, const float* obs, const float* err, int B, unsigned parts,
                 float* coeffs_or_null, float* stacked_or_null, float* image_or_null, void* workspace,
                 size_t workspace_bytes, void* hip_stream) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (int rp = refuse_planes(m, "gl_lstsq_fwd")) return rp;
  if (m->has_user && !m->user_fn[IMG_BASIS]) return fail(GL_EUNSUPPORTED, "the basis-stack kernel of this model with user-written profiles was not built");
  const int D = (int)m->lin_cols.size();
  if (D == 0) return fail(GL_EINVAL, "the model has no linear (light amplitude) coefficients");
  if (!params || !workspace) return fail(GL_EINVAL, "params / workspace is null");
  if (B <= 0 || B > 65535) return fail(GL_EINVAL, "batch size %d outside [1, 65535]", B);
  if (int rc = check_ready(m, true, false)) return rc;
  const bool solve = coeffs_or_null || image_or_null;
  if (solve && D > LS_MAXN)  // the basis stack alone (return_stacked) is served at any depth
    return fail(GL_EUNSUPPORTED, "%d linear coefficients exceed the %d the solve serves", D, LS_MAXN);
  if (solve && (!obs || !err)) return fail(GL_EINVAL, "obs / err_map are required to solve for the coefficients");
  if (!solve && !stacked_or_null) return fail(GL_EINVAL, "nothing to compute");
  if (!(parts & (GL_PART_LENS_LIGHT | GL_PART_SOURCE_LIGHT)) || parts > 7u) return fail(GL_EINVAL, "bad parts");
  const LaunchPlan plan = launch_plan(m, B);
  const Workspace w = carve(m, B, workspace, plan);
  LstsqWs lw = carve_lstsq(m, B, workspace, w);
  if (workspace_bytes < lw.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lw.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  const int chunk = plan.chunk, n_chunks = plan.n_chunks;
  int rc;
  const int HW = (m->height / m->supersample) * (m->width / m->supersample);
  // unit amplitudes -> derived constants -> basis stack
  hipLaunchKernelGGL(gl_unit_amplitudes_kernel, dim3((unsigned)(((long long)B * m->P + 255) / 256)), dim3(256), 0,
                     stream, params, m->P, B, m->d_lin_cols, D, w.params);
  GL_HIP(hipGetLastError());
  if ((rc = run_prep(m, w.params, nullptr, B, plan, w, stream))) return rc;
  MainArgs a = base_args(m, w, chunk);
  a.parts = parts | GL_PART_LENS_LIGHT | GL_PART_SOURCE_LIGHT;
  a.n_lin = D;
  if ((rc = run_order(m, B, w, &a, stream))) return rc;
  // One shapelet source as the only light component, no PSF / supersampling / pixel list, the stack not asked for: the normal
  // matrix straight from the bases (gl_shp_normal_kernel), no stack in HBM; a fitted image is rendered from the solved amplitudes
  const bool fused = solve && !stacked_or_null && !m->has_post && !m->d_pix && m->shp_kernel && m->static_id == ST_EPLSHEAR_SHAPELETS &&
                     m->n_ll == 0 && m->comps.back().iparam <= SH_CAP && D == sh_layers(m->comps.back().iparam) &&
                     (a.parts & (GL_PART_DEFLECT | GL_PART_SOURCE_LIGHT)) == (GL_PART_DEFLECT | GL_PART_SOURCE_LIGHT) &&
                     m->lstsq_fused;  // (a scaled source has static_id 0: the stack path, whose bases the interpreter renders at beta_s)
  if (fused) {
    lw.n_chunks = lw.n_chunks_f;
    const bool interp = (m->comps.back().flags & GL_FLAG_SHAPELETS_INTERPOLATE) != 0;
    constexpr int NPS = SH_SQ / 2;
    ShpNormalArgs sn{obs, err, lw.partial, D, lw.Dp};
    MainArgs fa = a;
    // (table mode on a whole image: 8 x 16 blocks of the image as wave-tiles, like gl_shp_kernel)
    fa.blk_w = (interp && m->shp_blocked && m->width % 16 == 0 && m->height % 8 == 0 && (long long)a.N == (long long)m->width * m->height) ? m->width : 0;
    const int nt = (D + 1 + 15) / 16;
    const size_t red = (size_t)(nt * (nt + 1) / 2 * 256 + 8) * sizeof(float);
    const size_t sh = (size_t)((m->D + 3) & ~3) * sizeof(float) +
                      std::max((size_t)4 * shn_wave_floats(NPS) * sizeof(float), red);
    const dim3 grid(lw.n_chunks, B), block(WG);
#define GL_SHPN(NT_, I_)                                                                                        \
  do {                                                                                                          \
    /* (table mode, five tile rows: 17 spilled VGPRs under the 128-register budget of four waves per SIMD since the live-pixel \
       list of round 4 -- three waves there) */                                                                  \
    m->last_main_fn = (const void*)&gl_shp_normal_kernel<NT_, ((I_ && NT_ < 5) ? 4 : 3), L_EplShear, NPS, I_>;              \
    g_lstsq_last_fn[0] = m->last_main_fn.load();                                                                \
    hipLaunchKernelGGL((gl_shp_normal_kernel<NT_, ((I_ && NT_ < 5) ? 4 : 3), L_EplShear, NPS, I_>), grid, block, sh, stream, fa, sn);  \
  } while (0)
    if (nt == 1) { if (interp) GL_SHPN(1, true); else GL_SHPN(1, false); }
    else if (nt == 2) { if (interp) GL_SHPN(2, true); else GL_SHPN(2, false); }
    else if (nt == 3) { if (interp) GL_SHPN(3, true); else GL_SHPN(3, false); }
    else if (nt == 4) { if (interp) GL_SHPN(4, true); else GL_SHPN(4, false); }
    else { if (interp) GL_SHPN(5, true); else GL_SHPN(5, false); }
#undef GL_SHPN
    GL_HIP(hipGetLastError());
  }
  float* target = m->has_post ? lw.stack_ss : lw.stack;
  if (!fused) {
  if (m->d_pix) GL_HIP(hipMemsetAsync(target, 0, sizeof(float) * (size_t)B * D * m->height * m->width, stream));
  a.img = target;
  if ((rc = launch_main<IMG_BASIS>(m, a, B, n_chunks, stream))) return rc;
  if (m->has_post && (rc = post_fwd(m, B * D, lw.stack_ss, lw.stack, stream, 1.f))) return rc;  // no det(T) here (:226-240)
  if (stacked_or_null)
    GL_HIP(hipMemcpyAsync(stacked_or_null, lw.stack, sizeof(float) * (size_t)B * D * HW, hipMemcpyDeviceToDevice, stream));
  }  // !fused
  if (!solve) return GL_OK;
  float* coeffs = coeffs_or_null ? coeffs_or_null : lw.coeffs;
  const SolveWs sw{lw.partial, lw.mats, lw.todo, lw.Dp, lw.chunk, lw.n_chunks};
  if ((rc = lstsq_solve(lw.stack, obs, err, B, D, HW, sw, fused, m->lstsq_chol, coeffs, stream))) return rc;
  if (image_or_null && fused) {
    // image = sum_d coeffs_d basis_d = the ordinary render with the solved amplitudes in their parameter columns (no det(T):
    // the stack carries none, tf/simulator.py:226-240)
    hipLaunchKernelGGL(gl_set_amplitudes_kernel, dim3((unsigned)(((long long)B * m->P + 255) / 256)), dim3(256), 0, stream,
                       params, m->P, B, m->d_lin_cols, D, coeffs, w.params);
    GL_HIP(hipGetLastError());
    if ((rc = run_prep(m, w.params, nullptr, B, plan, w, stream))) return rc;
    MainArgs ia = base_args(m, w, chunk);
    ia.parts = a.parts;
    ia.order = a.order;
    ia.img = image_or_null;
    ia.out_scale = 1.f;
    if ((rc = launch_main<IMG_FWD>(m, ia, B, n_chunks, stream))) return rc;
  } else if (image_or_null) {
    hipLaunchKernelGGL(gl_combine_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, stream, lw.stack, coeffs, D, HW,
                       image_or_null);
    GL_HIP(hipGetLastError());
  }
  return GL_OK;
}

namespace {
// a free-standing component as the point kernels take it (an EPL without a series length gets the default, epl.py:15)
CompDesc point_comp(const gl_component* comp) {
  CompDesc cd{};
  cd.kind = comp->kind;
  cd.iparam = comp->iparam;
  cd.flags = comp->flags;
  cd.n_par = kind_num_params(comp->kind, comp->iparam);
  if (cd.kind == GL_EPL && cd.iparam <= 0) cd.iparam = 50;
  return cd;
}

// The catalogue arguments of the plugin-level calls, in the order they are reported: base kind, sizes (`sizes_ok`: the caller's own
// counts), the series order (`order`; 0 where there is none), the scale columns.  `series`: the wording of the series calls.
int check_catalogue_args(bool series, int base_kind, bool sizes_ok, int order, const int32_t scale_col[3], int n_scales) {
  if (base_kind != GL_DPIS && base_kind != GL_DPIE && base_kind != GL_DPIEP)
    return series ? fail(GL_EUNSUPPORTED, "series expansion over profile kind %d is not built (dPIS, dPIE, dPIEP are)", base_kind)
                  : fail(GL_EUNSUPPORTED, "ScalingRelation over profile kind %d is not built (dPIS, dPIE, dPIEP are)", base_kind);
  if (!sizes_ok || n_scales < 1 || n_scales > 3) return fail(GL_EINVAL, "bad sizes");
  if (order < 0 || order > SERIES_MAX_ORDER) return fail(GL_EINVAL, "order %d outside [0, %d]", order, SERIES_MAX_ORDER);
  for (int k = 0; k < 3; ++k)
    if (scale_col[k] >= n_scales) return fail(GL_EINVAL, "scale_col[%d]=%d outside the %d scales", k, scale_col[k], n_scales);
  return GL_OK;
}

// the window of the lens-equation solver (`search` wording) and of the critical curves
int check_window(bool search, float x_lo, float x_hi, float y_lo, float y_hi) {
  if ((x_hi > x_lo) && (y_hi > y_lo) && std::isfinite(x_hi - x_lo) && std::isfinite(y_hi - y_lo)) return GL_OK;
  return search ? fail(GL_EINVAL, "empty or non-finite search window [%g, %g] x [%g, %g]", x_lo, x_hi, y_lo, y_hi)
                : fail(GL_EINVAL, "empty or non-finite window [%g, %g] x [%g, %g]", x_lo, x_hi, y_lo, y_hi);
}
}  // namespace

// process-lifetime table for plugin-level table-mode shapelets (n_max = cap), built on first use
static int point_shapelet_table(float** tab_out, int* stride_out) {
  static float* s_tab = nullptr;
  static int s_stride = 0;
  if (!s_tab) {
    std::vector<float> tab;
    glh::build_shapelet_table(GL_SHAPELETS_NMAX_CAP, tab, &s_stride);
    float* p = nullptr;
    GL_HIP(hipMalloc((void**)&p, tab.size() * sizeof(float)));
    GL_HIP(hipMemcpy(p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    s_tab = p;
  }
  *tab_out = s_tab;
  *stride_out = s_stride;
  return GL_OK;
}

static int series_precompute(bool hessian, int base_kind, int n_galaxies, const int32_t scale_col[3],
                             const float* table_dev, const float* scales, int n_scales, int order, const float* x_dev,
                             const float* y_dev, int64_t n_pts, float* coeffs_dev, void* hip_stream) {
  if (!scale_col || !table_dev || !scales || !x_dev || !y_dev || !coeffs_dev) return fail(GL_EINVAL, "null argument");
  if (int rc = check_catalogue_args(true, base_kind, n_galaxies > 0 && n_pts > 0, order, scale_col, n_scales)) return rc;
  if (scale_col[2] < 0) return fail(GL_EINVAL, "the series variable r_cut must be a scaled parameter");
  ScaledDesc sd{base_kind, n_galaxies, {scale_col[0], scale_col[1], scale_col[2]}};
  float s[3] = {1.f, 1.f, 1.f};
  for (int k = 0; k < n_scales; ++k) s[k] = scales[k];
  dim3 grid((unsigned)((n_pts + 63) / 64)), block(64);
  hipStream_t stream = (hipStream_t)hip_stream;
#define GL_SERIES_LAUNCH(KERNEL, NN) \
  hipLaunchKernelGGL((KERNEL<NN>), grid, block, 0, stream, sd, table_dev, s[0], s[1], s[2], order, x_dev, y_dev, \
                     (long long)n_pts, coeffs_dev)
  if (hessian) {
    if (order <= 3) GL_SERIES_LAUNCH(gl_series_hessian_precompute_kernel, 3);
    else GL_SERIES_LAUNCH(gl_series_hessian_precompute_kernel, 5);
  } else {
    if (order <= 3) GL_SERIES_LAUNCH(gl_series_precompute_kernel, 3);
    else GL_SERIES_LAUNCH(gl_series_precompute_kernel, 5);
  }
#undef GL_SERIES_LAUNCH
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_series_precompute(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev,
                         const float* scales, int n_scales, int order, const float* x_dev, const float* y_dev,
                         int64_t n_pts, float* coeffs_dev, void* hip_stream) {
  return series_precompute(false, base_kind, n_galaxies, scale_col, table_dev, scales, n_scales, order, x_dev, y_dev,
                           n_pts, coeffs_dev, hip_stream);
}

int gl_series_precompute_hessian(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev,
                                 const float* scales, int n_scales, int order, const float* x_dev, const float* y_dev,
                                 int64_t n_pts, float* coeffs_dev, void* hip_stream) {
  return series_precompute(true, base_kind, n_galaxies, scale_col, table_dev, scales, n_scales, order, x_dev, y_dev,
                           n_pts, coeffs_dev, hip_stream);
}

int gl_series_hessian_eval(const float* coeffs_dev, int order, int64_t n_pts, int B, const float* theta_E,
                           const float* r_cut, float r0, float* out, void* hip_stream) {
  if (!coeffs_dev || !theta_E || !r_cut || !out) return fail(GL_EINVAL, "null argument");
  if (order < 0 || order > SERIES_MAX_ORDER || n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "bad sizes");
  const long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_series_fields_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)hip_stream, coeffs_dev, 3, order, (long long)n_pts, B, theta_E, r_cut, r0, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_model_set_series_hessian(gl_model* m, int component, const float* coeffs_dev) {
  if (!m || !coeffs_dev) return fail(GL_EINVAL, "null argument");
  if (component < 0 || component >= m->n_lens || m->comps[component].kind != K_SERIES)
    return fail(GL_EINVAL, "component %d is not a GL_SERIES lens", component);
  const int slot = (int)m->comps[component].flags;
  SeriesDev& sv = m->series[slot];
  if (!sv.coef) return fail(GL_EINVAL, "gl_model_set_series must be called on component %d first", component);
  const size_t n = 3 * (size_t)(sv.order + 1) * m->N;
  glk::DevBuf<float>& buf = m->series_buf[slot].hcoef;
  if (!buf) GL_HIP(buf.alloc(n));  // (allocated once: the field of a slot keeps its size)
  sv.hcoef = buf;
  GL_HIP(buf.write(coeffs_dev, n, hipMemcpyDeviceToDevice));
  GL_HIP(m->d_series.write(m->series.data(), m->series.size()));
  return GL_OK;
}

int gl_model_set_light_image(gl_model* m, int component, int h, int w, const float* image_host) {
  if (!m || !image_host) return fail(GL_EINVAL, "null argument");
  if (component < m->n_lens || component >= (int)m->comps.size() || m->comps[component].kind != K_INTERPOL)
    return fail(GL_EINVAL, "component %d is not a GL_INTERPOL light", component);
  if (h < 1 || h > GL_INTERPOL_MAX_SIDE || w < 1 || w > GL_INTERPOL_MAX_SIDE)
    return fail(GL_EINVAL, "image of %d x %d pixels: height and width must lie in 1..%d", h, w, GL_INTERPOL_MAX_SIDE);
  for (size_t i = 0; i < (size_t)h * w; ++i)
    if (!std::isfinite(image_host[i])) return fail(GL_EINVAL, "image pixel %zu is not finite", i);
  // the two-pixel zero apron is added here, on the host: an in-range lane of the kernels needs no per-tap bounds test
  const int ws = w + 2 * glp::INT_APRON, hs = h + 2 * glp::INT_APRON;
  std::vector<float> padded((size_t)hs * ws, 0.f);
  for (int j = 0; j < h; ++j)
    std::copy(image_host + (size_t)j * w, image_host + (size_t)(j + 1) * w, padded.begin() + (size_t)(j + glp::INT_APRON) * ws + glp::INT_APRON);
  const int slot = m->comps[component].iparam;
  glk::DevBuf<float>& buf = m->interp_buf[slot];
  const bool first = !buf;
  GL_HIP(buf.upload(padded.data(), padded.size()));
  m->interp[slot] = InterpDev{buf.get(), h, w};
  if (first) ++m->n_interp_set;
  if (!m->d_interp) GL_HIP(m->d_interp.alloc(m->interp.size()));
  GL_HIP(m->d_interp.write(m->interp.data(), m->interp.size()));
  return GL_OK;
}

int gl_interpol_eval(const gl_component* comp, int h, int w, const float* image_dev, const float* x, const float* y,
                     int64_t n_pts, int B, int xy_batched, const float* params, float* out, int basis, void* hip_stream) {
  if (!comp || !image_dev || !x || !y || !params || !out) return fail(GL_EINVAL, "null argument");
  if (comp->kind != GL_INTERPOL) return fail(GL_EINVAL, "kind %d is not GL_INTERPOL", comp->kind);
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  if (h < 1 || h > GL_INTERPOL_MAX_SIDE || w < 1 || w > GL_INTERPOL_MAX_SIDE)
    return fail(GL_EINVAL, "image of %d x %d pixels: height and width must lie in 1..%d", h, w, GL_INTERPOL_MAX_SIDE);
  CompDesc cd{};
  cd.kind = comp->kind;
  cd.flags = comp->flags & GL_FLAG_INTERPOL_LINEAR;
  cd.n_par = kind_num_params(comp->kind, 0);
  const InterpDev tb{image_dev, h, w};
  const long long total = (long long)n_pts * B;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (basis)
    hipLaunchKernelGGL(gl_basis_point_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, cd, x, y, (long long)n_pts, B,
                       xy_batched, params, out, (const float*)nullptr, 0, tb);
  else
    hipLaunchKernelGGL(gl_point_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, cd, x, y, (long long)n_pts, B, xy_batched,
                       params, out, (float*)nullptr, (const float*)nullptr, 0, tb);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_model_set_series(gl_model* m, int component, float r0, const float* coeffs_dev) {
  if (!m || !coeffs_dev) return fail(GL_EINVAL, "null argument");
  if (component < 0 || component >= m->n_lens || m->comps[component].kind != K_SERIES)
    return fail(GL_EINVAL, "component %d is not a GL_SERIES lens", component);
  const int slot = (int)m->comps[component].flags;
  SeriesDev& sv = m->series[slot];
  const size_t n = 2 * (size_t)(sv.order + 1) * m->N;
  glk::DevBuf<float>& buf = m->series_buf[slot].coef;
  if (!buf) {  // (allocated once: the field of a slot keeps its size)
    GL_HIP(buf.alloc(n));
    sv.coef = buf;
    ++m->n_series_set;
  }
  GL_HIP(buf.write(coeffs_dev, n, hipMemcpyDeviceToDevice));
  sv.r0 = r0;
  if (!m->d_series) GL_HIP(m->d_series.alloc(m->series.size()));
  GL_HIP(m->d_series.write(m->series.data(), m->series.size()));
  return GL_OK;
}

int gl_series_eval(const float* coeffs_dev, int order, int64_t n_pts, int B, const float* theta_E, const float* r_cut,
                   float r0, float* out0, float* out1, void* hip_stream) {
  if (!coeffs_dev || !theta_E || !r_cut || !out0 || !out1) return fail(GL_EINVAL, "null argument");
  if (order < 0 || order > SERIES_MAX_ORDER || n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "bad sizes");
  const long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_series_eval_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     coeffs_dev, order, (long long)n_pts, B, theta_E, r_cut, r0, out0, out1);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_model_set_catalogue(gl_model* m, int component, int base_kind, int n_galaxies, const int32_t scale_col[3],
                           const float* table) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (component < 0 || component >= m->n_lens || m->comps[component].kind != K_SCALED)
    return fail(GL_EINVAL, "component %d is not a GL_SCALED lens", component);
  if (base_kind != GL_DPIS && base_kind != GL_DPIE && base_kind != GL_DPIEP)
    return fail(GL_EUNSUPPORTED, "ScalingRelation over profile kind %d is not built (dPIS, dPIE, dPIEP are)", base_kind);
  if (n_galaxies <= 0 || !scale_col || !table) return fail(GL_EINVAL, "empty catalogue");
  CompDesc& cd = m->comps[component];
  int used = 0;
  for (int k = 0; k < 3; ++k) {
    if (scale_col[k] >= cd.n_par) return fail(GL_EINVAL, "scale_col[%d]=%d outside the component's %d scales", k, scale_col[k], cd.n_par);
    if (scale_col[k] >= 0) {
      if (used & (1 << scale_col[k])) return fail(GL_EINVAL, "scale column %d used twice", scale_col[k]);
      used |= 1 << scale_col[k];
    }
  }
  if (used != (1 << cd.n_par) - 1) return fail(GL_EINVAL, "every one of the %d scales must drive one of theta_E, r_core, r_cut", cd.n_par);
  gl_model::Cat cat{};
  cat.dev.base_kind = base_kind;
  cat.dev.n_gal = n_galaxies;
  cat.dev.comp = component;
  for (int k = 0; k < 3; ++k) cat.dev.col[k] = scale_col[k];
  cat.table.assign(table, table + (size_t)7 * n_galaxies);
  if (cd.iparam >= 0) m->cats[cd.iparam] = cat;
  else { cd.iparam = (int)m->cats.size(); m->cats.push_back(cat); }
  // rebuild the model-wide galaxy arrays
  std::vector<CatDev> devs;
  std::vector<float> tab, stat;
  int G = 0;
  for (auto& c : m->cats) {
    c.dev.g_off = G;
    G += c.dev.n_gal;
    devs.push_back(c.dev);
    tab.insert(tab.end(), c.table.begin(), c.table.end());
    for (int g = 0; g < c.dev.n_gal; ++g) {
      float ds[DP_NS];
      scaled_static<float>(c.dev.base_kind, c.table.data() + (size_t)7 * g, ds);
      stat.insert(stat.end(), ds, ds + DP_NS);
    }
  }
  m->G = G;
  GL_HIP(m->d_cats.upload(devs.data(), devs.size()));
  GL_HIP(m->d_gal_table.upload(tab.data(), tab.size()));
  GL_HIP(m->d_gal_static.upload(stat.data(), stat.size()));
  GL_HIP(m->d_comps.write(m->comps.data(), m->comps.size()));
  return GL_OK;
}

int gl_scaled_eval(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev, const float* x,
                   const float* y, int64_t n_pts, int B, int xy_batched, const float* scales, int n_scales,
                   float* out0, float* out1, void* hip_stream) {
  if (!scale_col || !table_dev || !x || !y || !scales || !out0 || !out1) return fail(GL_EINVAL, "null argument");
  if (int rc = check_catalogue_args(false, base_kind, n_galaxies > 0 && n_pts > 0 && B > 0, 0, scale_col, n_scales)) return rc;
  ScaledDesc sd{base_kind, n_galaxies, {scale_col[0], scale_col[1], scale_col[2]}};
  long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_scaled_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)hip_stream, sd, table_dev, x, y, (long long)n_pts, B, xy_batched, scales, n_scales,
                     out0, out1);
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

int gl_model_set_positions(gl_model* m, int n_families, const int* family_sizes, const float* x, const float* y,
                           const float* err_x, const float* err_y) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (n_families <= 0 || !family_sizes || !x || !y || !err_x || !err_y) return fail(GL_EINVAL, "bad position tables");
  std::vector<int> off(n_families + 1, 0);
  for (int f = 0; f < n_families; ++f) {
    if (family_sizes[f] <= 0) return fail(GL_EINVAL, "image family %d is empty", f);
    off[f + 1] = off[f] + family_sizes[f];
  }
  const int J = off[n_families];
  std::vector<float> tab((size_t)4 * J);
  for (int j = 0; j < J; ++j) { tab[j] = x[j]; tab[J + j] = y[j]; tab[2 * J + j] = err_x[j]; tab[3 * J + j] = err_y[j]; }
  GL_HIP(m->d_pos.upload(tab.data(), tab.size()));
  GL_HIP(m->d_fam.upload(off.data(), off.size()));
  m->pos_J = J;
  m->pos_F = n_families;
  m->pos_fam_off = off;
  m->pos_scaled = false;  // new tables: every family back on the reference plane
  m->d_pos_scale.reset();
  return GL_OK;
}

namespace {
// n deflection scales: finite and > 0; *any = some scale differs from 1
int check_scales(const float* scales, int n, int expect, const char* what, bool* any) {
  if (!scales) return fail(GL_EINVAL, "scales is null");
  if (n != expect) return fail(GL_EINVAL, "%d scales for %d %s", n, expect, what);
  *any = false;
  for (int i = 0; i < n; ++i) {
    if (!(std::isfinite(scales[i]) && scales[i] > 0.f)) return fail(GL_EINVAL, "scale %d (%g) is not finite and > 0", i, scales[i]);
    *any = *any || scales[i] != 1.f;
  }
  return GL_OK;
}
}  // namespace

int gl_model_set_source_scales(gl_model* m, const float* scales, int n_src) {
  if (!m) return fail(GL_EINVAL, "model is null");
  bool any;
  if (int rc = check_scales(scales, n_src, m->n_src, "source light component(s)", &any)) return rc;
  if (any && m->mp_K >= 2) return fail(GL_EINVAL, "the model has lens planes (gl_model_set_lens_planes): their source couplings replace per-source scales");
  if (any && m->has_user)
    return fail(GL_EUNSUPPORTED, "per-source deflection scales are not served on the pixel grid for models with user-written profiles");
  if (any) GL_HIP(m->d_src_scale.upload(scales, (size_t)n_src));
  else m->d_src_scale.reset();
  m->src_scaled = any;
  // A scaled model is the interpreter's (and the scaled cluster kernel's) in EVERY respect, not only at the launch: the chunking
  // rule, the tapered end of the cost-ordered dispatch (only the pair kernels decode that grid) and the stack-free linear solve all
  // key on static_id, exactly as for a model created with GIGALENS_HIP_STATIC=0.  The workspace layout follows the launch plan:
  // callers size it again after this call (gl_workspace_bytes).
  m->static_id = any ? 0 : m->static_matched;
  return GL_OK;
}

int gl_model_set_position_scales(gl_model* m, const float* scales, int n_families) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  bool any;
  if (int rc = check_scales(scales, n_families, m->pos_F, "image famil(ies)", &any)) return rc;
  if (any) {
    std::vector<float> per_image((size_t)m->pos_J);
    for (int f = 0; f < m->pos_F; ++f)
      for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) per_image[j] = scales[f];
    GL_HIP(m->d_pos_scale.upload(per_image.data(), per_image.size()));
  } else {
    m->d_pos_scale.reset();
  }
  m->pos_scaled = any;
  return GL_OK;
}

int gl_positions_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                         float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rp = refuse_planes(m, "gl_positions_fwd_bwd")) return rp;
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w);
  if (rc) return rc;
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if (!loglike || !chi2) return fail(GL_EINVAL, "loglike / chi2 is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = run_positions(m, params, B, w, grad_params_or_null != nullptr, stream))) return rc;
  GL_HIP(hipMemcpyAsync(loglike, w.pos_ll, sizeof(float) * B, hipMemcpyDeviceToDevice, stream));
  GL_HIP(hipMemcpyAsync(chi2, w.pos_chi2, sizeof(float) * B, hipMemcpyDeviceToDevice, stream));
  if (grad_params_or_null)
    GL_HIP(hipMemcpyAsync(grad_params_or_null, w.pos_grad, sizeof(float) * (size_t)B * m->P, hipMemcpyDeviceToDevice, stream));
  return GL_OK;
}

int gl_profile_hessian(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                       const float* params, float* out, void* hip_stream) {
  if (!comp || !x || !y || !params || !out) return fail(GL_EINVAL, "null argument");
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  if (!((comp->kind >= GL_EPL && comp->kind <= GL_DPIEP) || comp->kind == GL_NFW_ELLIPSE || comp->kind == GL_TNFW))
    return fail(GL_EINVAL, "kind %d is not a free-standing mass profile", comp->kind);
  const CompDesc cd = point_comp(comp);
  const long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_profile_hessian_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream,
                     cd, x, y, (long long)n_pts, B, xy_batched, params, out);
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
  hipLaunchKernelGGL(gl_lens_maps_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream, a,
                     x, y, (long long)n_pts, xy_batched, out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- lensing potential (gl_potential.hip.h) --------------------------------------------------------------------
namespace {
bool potential_kind(int kind) {
  return (kind >= GL_EPL && kind <= GL_DPIEP) || kind == GL_NFW_ELLIPSE || kind == GL_TNFW;
}
}  // namespace

int gl_lens_potential(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts,
                      int xy_batched, float* out, void* hip_stream) {
  if (!m || !params || !out) return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_lens_potential")) return rp;
  if ((x == nullptr) != (y == nullptr)) return fail(GL_EINVAL, "x and y must both be given or both be null");
  if (B <= 0 || n_pts <= 0) return fail(GL_EINVAL, "B and n_pts must be positive");
  for (int l = 0; l < m->n_lens; ++l) {
    const int kind = m->comps[l].kind;
    if (kind == GL_SERIES)
      return fail(GL_EUNSUPPORTED, "lens %d is a series expansion: its precomputed field holds the deflection, no potential", l);
    if (kind == GL_USER_MASS)
      return fail(GL_EUNSUPPORTED, "lens %d is a user-written body (or a run-time compiled ScalingRelation member loop): "
                                   "a body defines the deflection only, no potential", l);
    if (!potential_kind(kind) && kind != GL_SCALED) return fail(GL_EUNSUPPORTED, "lens %d: kind %d has no potential", l, kind);
  }
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
namespace {
struct ImgLayout { size_t map, cand, n_cand, n_over, scale, bytes; };
ImgLayout img_layout(int B, int n_src, int n_cells) {
  ImgLayout l{};
  const size_t V = (size_t)(n_cells + 1) * (size_t)(n_cells + 1), BS = (size_t)B * (size_t)n_src;
  l.map = 0;
  l.cand = l.map + align_up((size_t)B * V * sizeof(float2), 256);
  l.n_cand = l.cand + align_up(BS * IMG_MAXC * sizeof(float2), 256);
  l.n_over = l.n_cand + align_up(BS * sizeof(int), 256);
  l.scale = l.n_over + align_up(BS * sizeof(int), 256);  // [n_src] deflection scales of gl_image_positions_scaled
  l.bytes = l.scale + align_up((size_t)n_src * sizeof(float), 256);
  return l;
}
constexpr int IMG_MAX_CELLS = 8192;
}  // namespace

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
  } else {
    hipLaunchKernelGGL(gl_img_map_kernel, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  }
  hipLaunchKernelGGL(gl_img_scan_kernel, dim3((unsigned)pairs), dim3(IMG_SCAN_WG), 0, stream, g);
  if (m->has_user) {
    void* args[] = {&a, &g};
    GL_HIP(hipModuleLaunchKernel(m->user_point_fn[6], (unsigned)pairs, 1, 1, 64, 1, 1, 0, stream, args, nullptr));
  } else {
    hipLaunchKernelGGL(gl_img_newton_kernel, dim3((unsigned)pairs), dim3(64), 0, stream, a, g);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- critical curves and caustics (gl_critical.hip.h) ----------------------------------------------------------
namespace {
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
}  // namespace

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
  const bool cat = m->n_scaled > 0;  // catalogues take the build whose evaluation is a function call (gl_critical.hip.h, crit_eval)
  if (cat) hipLaunchKernelGGL(gl_crit_map_kernel<true>, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  else hipLaunchKernelGGL(gl_crit_map_kernel<false>, dim3((unsigned)map_blocks), dim3(256), 0, stream, a, g);
  hipLaunchKernelGGL(gl_crit_scan_kernel, dim3((unsigned)B), dim3(CRIT_WG), 0, stream, g);
  if (cat) hipLaunchKernelGGL(gl_crit_refine_kernel<true>, dim3((unsigned)refine_blocks), dim3(64), 0, stream, a, g);
  else hipLaunchKernelGGL(gl_crit_refine_kernel<false>, dim3((unsigned)refine_blocks), dim3(64), 0, stream, a, g);
  hipLaunchKernelGGL(gl_crit_cells_kernel, dim3((unsigned)B), dim3(CRIT_WG), 0, stream, g);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- pixelated source reconstruction (gl_pixsrc.hip.h) -----------------------------------------------------------
namespace {
constexpr size_t PIX_CHUNK_BUDGET = (size_t)256 << 20;  // operator, normal matrices and factors of one chunk of samples
constexpr size_t PIX_PLANE_BUDGET = (size_t)32 << 20;   // basis planes (supersampled and pooled) of one post-processing launch
constexpr int PIX_MAX_L_SLICE = 4;                      // factors held at once per sample
constexpr int PIX_MAX_PLANES = 4096;
struct PixLayout {
  int cb, lch, pc, n_pad;  // samples per chunk, strengths per slice, planes per post-processing launch
  size_t planes_ss, planes_lo, Fw, yw, A0, bvec, M, bytes;
};
PixLayout pix_layout(const gl_model* m, int B, int L, int S, int n_used) {
  PixLayout l{};
  const size_t HsWs = (size_t)m->height * m->width, HW = HsWs / ((size_t)m->supersample * m->supersample);
  l.n_pad = (n_used + PIX_TK - 1) / PIX_TK * PIX_TK;
  l.lch = std::min(L, PIX_MAX_L_SLICE);
  const size_t per_sample = sizeof(float) * ((size_t)S * l.n_pad + l.n_pad + (size_t)S * S * (1 + l.lch) + S);
  l.cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, PIX_CHUNK_BUDGET / per_sample));
  const size_t per_plane = sizeof(float) * ((m->has_post ? HsWs : 0) + HW);
  l.pc = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)l.cb * S, PIX_MAX_PLANES), PIX_PLANE_BUDGET / per_plane));
  l.planes_ss = 0;
  l.planes_lo = l.planes_ss + align_up(m->has_post ? sizeof(float) * (size_t)l.pc * HsWs : 0, 256);
  l.Fw = l.planes_lo + align_up(sizeof(float) * (size_t)l.pc * HW, 256);
  l.yw = l.Fw + align_up(sizeof(float) * (size_t)l.cb * S * l.n_pad, 256);
  l.A0 = l.yw + align_up(sizeof(float) * (size_t)l.cb * l.n_pad, 256);
  l.bvec = l.A0 + align_up(sizeof(float) * (size_t)l.cb * S * S, 256);
  l.M = l.bvec + align_up(sizeof(float) * (size_t)l.cb * S, 256);
  l.bytes = l.M + align_up(sizeof(float) * (size_t)l.cb * l.lch * S * S, 256);
  return l;
}
bool pix_sizes_ok(const gl_model* m, int B, int L, int ny, int nx, int n_used) {
  if (!m || B <= 0 || B > 65535 || L <= 0 || L > 65535 || ny <= 0 || nx <= 0 || (long long)ny * nx > PIX_MAX_S) return false;
  const long long HW = (long long)(m->height / m->supersample) * (m->width / m->supersample);
  return n_used > 0 && n_used <= HW;
}
}  // namespace

size_t gl_pixsrc_workspace_bytes(const gl_model* m, int B, int n_strength, int ny, int nx, int n_used) {
  if (!pix_sizes_ok(m, B, n_strength, ny, nx, n_used)) return 0;
  return pix_layout(m, B, n_strength, ny * nx, n_used).bytes;
}

int gl_pixsrc_reconstruct(const gl_model* m, const float* beta_x, const float* beta_y, int B, const float* obs, const float* sigma,
                          const float* lens_light, const int* pix, int n_used, int ny, int nx, const float* pose, int regularization,
                          const float* strength, int n_strength, float* source, float* model_image, double* scalars, int* ok,
                          void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !beta_x || !beta_y || !obs || !sigma || !pix || !pose || !strength || !source || !model_image || !scalars || !ok)
    return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_pixsrc_reconstruct")) return rp;
  if (ny <= 0 || nx <= 0) return fail(GL_EINVAL, "source grid %d x %d: both sides must be positive", ny, nx);
  if ((long long)ny * nx > PIX_MAX_S) return fail(GL_EUNSUPPORTED, "source grid %d x %d has more than %d nodes", ny, nx, PIX_MAX_S);
  if (regularization < PIX_REG_IDENTITY || regularization > PIX_REG_CURVATURE) return fail(GL_EINVAL, "unknown regularization %d", regularization);
  if (!pix_sizes_ok(m, B, n_strength, ny, nx, n_used))
    return fail(GL_EINVAL, "bad sizes: B = %d, strengths = %d (both in 1..65535), used pixels = %d (1..H W)", B, n_strength, n_used);
  const int S = ny * nx, L = n_strength;
  const PixLayout lay = pix_layout(m, B, L, S, n_used);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  float* planes_lo = (float*)(base + lay.planes_lo);
  float* planes_ss = m->has_post ? (float*)(base + lay.planes_ss) : planes_lo;
  PixArgs a{};
  a.ny = ny; a.nx = nx; a.S = S;
  a.HsWs = m->height * m->width;
  a.HW = a.HsWs / (m->supersample * m->supersample);
  a.n_used = n_used; a.n_pad = lay.n_pad;
  a.reg = regularization;
  a.L_total = L;
  a.pix = pix;
  a.Fw = (float*)(base + lay.Fw);
  a.yw = (float*)(base + lay.yw);
  a.A0 = (float*)(base + lay.A0);
  a.bvec = (float*)(base + lay.bvec);
  a.M = (float*)(base + lay.M);
  const int T = (S + PIX_TK - 1) / PIX_TK;
  for (int b0 = 0; b0 < B; b0 += lay.cb) {
    const int nb = std::min(lay.cb, B - b0);
    a.B = nb;
    a.beta_x = beta_x + (size_t)b0 * a.HsWs;
    a.beta_y = beta_y + (size_t)b0 * a.HsWs;
    a.pose = pose + (size_t)b0 * 3;
    a.sigma = sigma + (size_t)b0 * n_used;
    a.obs = obs + (size_t)b0 * n_used;
    a.lens_light = lens_light ? lens_light + (size_t)b0 * a.HW : nullptr;
    // the operator, a launch of basis planes at a time
    for (int p0 = 0; p0 < nb * S; p0 += lay.pc) {
      const int np = std::min(lay.pc, nb * S - p0);
      hipLaunchKernelGGL(gl_pix_planes_kernel, dim3((a.HsWs + PIX_WG - 1) / PIX_WG, np), dim3(PIX_WG), 0, stream, a, p0,
                         m->has_post ? 1.f : m->conversion_factor, planes_ss);
      if (m->has_post)
        if (int rc = post_fwd(m, np, planes_ss, planes_lo, stream, m->conversion_factor)) return rc;
      hipLaunchKernelGGL(gl_pix_gather_kernel, dim3((a.n_pad + PIX_WG - 1) / PIX_WG, np), dim3(PIX_WG), 0, stream, a, p0, planes_lo);
    }
    hipLaunchKernelGGL(gl_pix_rhs_prep_kernel, dim3((a.n_pad + PIX_WG - 1) / PIX_WG, nb), dim3(PIX_WG), 0, stream, a);
    hipLaunchKernelGGL(gl_pix_normal_kernel, dim3(T * (T + 1) / 2, nb), dim3(PIX_WG), 0, stream, a);
    hipLaunchKernelGGL(gl_pix_rhs_kernel, dim3((S + PIX_WG / 64 - 1) / (PIX_WG / 64), nb), dim3(PIX_WG), 0, stream, a);
    for (int l0 = 0; l0 < L; l0 += lay.lch) {
      const int nl = std::min(lay.lch, L - l0);
      const size_t o = (size_t)b0 * L + l0;
      a.L = nl;
      a.strength = strength + o;
      a.source = source + o * S;
      a.model = model_image + o * a.HW;
      a.scal = scalars + 3 * o;
      a.ok = ok + o;
      hipLaunchKernelGGL(gl_pix_solve_kernel, dim3(nb, nl), dim3(PIX_WG), 0, stream, a);
      hipLaunchKernelGGL(gl_pix_combine_kernel, dim3(nb, nl), dim3(PIX_WG), 0, stream, a);
    }
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// ---- lens planes at redshifts of their own (gl_multiplane.hip.h) ---------------------------------------------------
namespace {
MpArgs mp_args(const gl_model* m) {
  MpArgs a{};
  a.order = m->d_mp_lens;
  a.plane = m->d_mp_lens + m->n_lens;
  a.scale = m->d_mp_scale;
  return a;
}

// the model's image of `parts` on its planes: into `img` [B][H][W] (x conversion factor), through the PSF + pooling launch of the
// single-plane render where the model has one
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

int check_planes_set(const gl_model* m) {
  return m->mp_K >= 2 ? GL_OK : fail(GL_EINVAL, "gl_model_set_lens_planes has not been called on this model");
}

// The VJP of mp_render's kernel (gl_multiplane_bwd.hip.h): cotangent `gimg` [B][Hs Ws] of the supersampled frame (x out_scale) ->
// one row of accumulators per (sample, chunk of the plan) in w.partial, for run_finalize.  Reads w.derived: run_prep comes first.
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
  for (const CompDesc& c : m->comps) xf = xf || c.kind == K_NFW_ELLIPSE || c.kind == K_TNFW || c.kind == K_CORE_SERSIC;
  const size_t shmem = (size_t)(((m->D + 3) & ~3) + m->ncols * m->Apad) * sizeof(float);
  const dim3 grid((unsigned)plan.n_chunks, (unsigned)B), block(MP_WG);
  if (xf) hipLaunchKernelGGL(gl_mp_bwd_kernel<true>, grid, block, shmem, stream, mp_args(m), r);
  else hipLaunchKernelGGL(gl_mp_bwd_kernel<false>, grid, block, shmem, stream, mp_args(m), r);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// pixel likelihood of the multi-plane image of `params` (packed rows; w.derived holds their derived rows when want_grad):
// render -> [PSF + pooling] -> image statistics [with cotangent -> transposes -> VJP kernel].  w.stats holds chi2 and the
// normalisation for run_finalize (extra_stats), w.partial the accumulator rows when want_grad.
int mp_likelihood(const gl_model* m, const float* params, int B, const LaunchPlan& plan, const Workspace& w, const float* obs,
                  const float* err, const float* mask, float bg_rms, float exp_time, bool want_grad, hipStream_t stream) {
  if (int rc = mp_render(m, params, B, 7u, w.img_tmp, w, stream)) return rc;
  const int HW = (m->height / m->supersample) * (m->width / m->supersample);
  hipLaunchKernelGGL(gl_imgstats_kernel, dim3(B), dim3(256), 0, stream, w.img_tmp, obs, err, mask, bg_rms * bg_rms, 1.0f / exp_time, HW,
                     w.stats, want_grad ? w.img_tmp : nullptr);
  GL_HIP(hipGetLastError());
  if (!want_grad) return GL_OK;
  if (!m->has_post) return mp_render_bwd(m, B, plan, w, w.img_tmp, m->conversion_factor, stream);
  if (int rc = post_bwd(m, B, w.img_tmp, w.img_ss, stream, m->conversion_factor)) return rc;
  return mp_render_bwd(m, B, plan, w, w.img_ss, 1.f, stream);
}
}  // namespace

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
  if (m->src_scaled) return fail(GL_EINVAL, "the model carries per-source deflection scales (gl_model_set_source_scales): the source couplings of the planes replace them");
  for (int l = 0; l < m->n_lens; ++l)
    if (m->comps[l].kind == K_SCALED)
      return fail(GL_EUNSUPPORTED, "lens %d: galaxy catalogues (GL_SCALED) are not served on lens planes", l);
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

int gl_multiplane_simulate(const gl_model* m, const float* params, int B, unsigned parts, float* img, void* workspace,
                           size_t workspace_bytes, void* hip_stream) {
  LaunchPlan plan;
  Workspace w;
  if (int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w)) return rc;
  if (int rc = check_planes_set(m)) return rc;
  if (!img) return fail(GL_EINVAL, "img is null");
  if (parts == 0 || parts > 7u) return fail(GL_EINVAL, "parts must be a non-empty subset of {1,2,4}");
  return mp_render(m, params, B, parts, img, w, (hipStream_t)hip_stream);
}

int gl_multiplane_loglike(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                          const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                          void* workspace, size_t workspace_bytes, void* hip_stream) {
  return gl_multiplane_loglike_fwd_bwd(m, params, obs, err_or_null, mask_or_null, bg_rms, exp_time, B, loglike, chi2, nullptr, workspace,
                                       workspace_bytes, hip_stream);  // the forward half: the same launches, no front end, no VJP
}

int gl_multiplane_simulate_bwd(const gl_model* m, const float* params, const float* grad_img, int B, float* grad_params,
                               void* workspace, size_t workspace_bytes, void* hip_stream) {
  LaunchPlan plan;
  Workspace w;
  if (int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w)) return rc;
  if (int rc = check_planes_set(m)) return rc;
  if (!grad_img || !grad_params) return fail(GL_EINVAL, "grad_img / grad_params is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  if (int rc = run_prep(m, params, nullptr, B, plan, w, stream)) return rc;
  const float* gimg = grad_img;
  float out_scale = m->conversion_factor;
  if (m->has_post) {
    if (int rc = post_bwd(m, B, grad_img, w.img_ss, stream, m->conversion_factor)) return rc;
    gimg = w.img_ss;
    out_scale = 1.f;
  }
  if (int rc = mp_render_bwd(m, B, plan, w, gimg, out_scale, stream)) return rc;
  return run_finalize(m, params, B, plan.n_chunks, w, nullptr, nullptr, grad_params, stream);
}

int gl_multiplane_loglike_fwd_bwd(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                                  const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                                  float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  LaunchPlan plan;
  Workspace w;
  if (int rc = check_call(m, params, B, workspace, workspace_bytes, &plan, &w)) return rc;
  if (int rc = check_planes_set(m)) return rc;
  if (!obs || !loglike || !chi2) return fail(GL_EINVAL, "obs / loglike / chi2 is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  const bool want_grad = grad_params_or_null != nullptr;
  if (want_grad)
    if (int rc = run_prep(m, params, nullptr, B, plan, w, stream)) return rc;
  if (int rc = mp_likelihood(m, params, B, plan, w, obs, err_or_null, mask_or_null, bg_rms, exp_time, want_grad, stream)) return rc;
  return run_finalize(m, params, B, plan.n_chunks, w, loglike, chi2, grad_params_or_null, stream, nullptr, nullptr, nullptr, 1.f,
                      w.stats, want_grad ? 1 : 0);
}

int gl_multiplane_logprob_fwd_bwd(const gl_model* m, const float* z, const float* obs, const float* err_or_null,
                                  const float* mask_or_null, float bg_rms, float exp_time, int B, float* logprob, float* loglike,
                                  float* red_chi2, float* grad_z_or_null, float chi2_divisor, unsigned terms, void* workspace,
                                  size_t workspace_bytes, void* hip_stream) {
  LaunchPlan plan;
  Workspace w;
  if (int rc = check_call(m, z, B, workspace, workspace_bytes, &plan, &w)) return rc;
  if (int rc = check_planes_set(m)) return rc;
  if (terms != GL_TERM_PIXELS)
    return fail(GL_EINVAL, "terms = %u: a model with lens planes has the pixel term alone (no multi-plane position likelihood)", terms);
  if (!(chi2_divisor > 0.f)) return fail(GL_EINVAL, "chi2_divisor must be positive");
  if (!m->d_zcols) return fail(GL_EINVAL, "gl_model_set_prior has not been called on this model");
  if (!obs || !logprob || !loglike || !red_chi2) return fail(GL_EINVAL, "obs / logprob / loglike / red_chi2 is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  const bool want_grad = grad_z_or_null != nullptr;
  if (int rc = run_prep(m, nullptr, z, B, plan, w, stream)) return rc;  // constrained rows -> w.params, derived rows
  if (int rc = mp_likelihood(m, w.params, B, plan, w, obs, err_or_null, mask_or_null, bg_rms, exp_time, want_grad, stream)) return rc;
  return run_finalize(m, w.params, B, plan.n_chunks, w, loglike, red_chi2, nullptr, stream, z, logprob, grad_z_or_null,
                      1.0f / chi2_divisor, w.stats, want_grad ? 1 : 0);
}

int gl_model_set_prior(gl_model* m, const gl_zcolumn* cols, int d, const float* const_row) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (d < 0 || (d > 0 && !cols)) return fail(GL_EINVAL, "bad prior column table");
  std::vector<int> src(std::max(m->P, 1), -1);
  std::vector<ZCol> zc(std::max(d, 1));
  for (int k = 0; k < d; ++k) {
    const gl_zcolumn& c = cols[k];
    if (c.param_col < 0 || c.param_col >= m->P) return fail(GL_EINVAL, "z column %d: param_col %d out of range", k, c.param_col);
    if (src[c.param_col] >= 0) return fail(GL_EINVAL, "packed column %d driven by two z columns", c.param_col);
    if (c.bijector < 0 || c.bijector > 2 || c.prior < 0 || c.prior > 3) return fail(GL_EINVAL, "z column %d: unknown bijector/prior", k);
    src[c.param_col] = k;
    zc[k] = ZCol{c.param_col, c.bijector, c.prior, c.a, c.b, c.lo, c.hi, c.log_norm};
  }
  std::vector<float> cr(std::max(m->P, 1), 0.f);
  for (int p = 0; p < m->P; ++p) {
    if (src[p] < 0) {
      if (!const_row) return fail(GL_EINVAL, "packed column %d has neither a z column nor a constant", p);
      cr[p] = const_row[p];
    }
  }
  GL_HIP(m->d_zcols.upload(zc.data(), zc.size()));
  GL_HIP(m->d_src.upload(src.data(), src.size()));
  GL_HIP(m->d_const.upload(cr.data(), cr.size()));
  m->d_z = d;
  return GL_OK;
}

int gl_logprob_fwd_bwd(const gl_model* m, const float* z, const float* obs, const float* err_or_null,
                       const float* mask_or_null, float bg_rms, float exp_time, int B, float* logprob, float* loglike,
                       float* chi2, float* grad_z_or_null, float chi2_divisor, unsigned terms, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
  if (int rp = refuse_planes(m, "gl_logprob_fwd_bwd")) return rp;
  LaunchPlan plan;
  Workspace w;
  int rc = check_call(m, z, B, workspace, workspace_bytes, &plan, &w);
  if (rc) return rc;
  const bool pix = terms & GL_TERM_PIXELS, pos = terms & GL_TERM_POSITIONS;
  if (!pix && !pos) return fail(GL_EINVAL, "terms selects no likelihood term");
  if (pix && !(chi2_divisor > 0.f)) return fail(GL_EINVAL, "chi2_divisor must be positive");
  if (!m->d_zcols) return fail(GL_EINVAL, "gl_model_set_prior has not been called on this model");
  if (pos && !m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if ((pix && !obs) || !logprob || !loglike || !chi2) return fail(GL_EINVAL, "obs / logprob / loglike / chi2 is null");
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = run_prep(m, nullptr, z, B, plan, w, stream))) return rc;
  const float* extra = nullptr;
  int use_partial = 0, fin_rows = plan.n_chunks;
  // red_chi2 = (red_pix + red_pos) / n_chi  (tf/model.py:150-162)
  const float n_chi = (pix ? 1.f : 0.f) + (pos ? 1.f : 0.f);
  if (pix && (rc = run_likelihood(m, B, plan, w, obs, err_or_null, mask_or_null, bg_rms, exp_time,
                                  grad_z_or_null != nullptr, stream, &extra, &use_partial, &fin_rows)))
    return rc;
  if (pos && (rc = run_positions(m, w.params, B, w, grad_z_or_null != nullptr, stream))) return rc;
  return run_finalize(m, w.params, B, fin_rows, w, loglike, chi2, nullptr, stream, z, logprob, grad_z_or_null,
                      pix ? 1.0f / (chi2_divisor * n_chi) : 0.f, extra, use_partial, pos,
                      pos ? 1.0f / (2.0f * (float)m->pos_J * n_chi) : 0.f);
}

int gl_profile_eval(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                    const float* params, float* out0, float* out1, void* hip_stream) {
  if (!comp || !x || !y || !params || !out0) return fail(GL_EINVAL, "null argument");
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  int npar = kind_num_params(comp->kind, comp->iparam);
  if (npar < 0) return fail(GL_EINVAL, "unknown profile kind %d", comp->kind);
  if (comp->kind == GL_SCALED) return fail(GL_EINVAL, "GL_SCALED needs its catalogue: use gl_scaled_eval");
  if (comp->kind == GL_SERIES) return fail(GL_EINVAL, "GL_SERIES needs its coefficient field: use gl_series_eval");
  if (comp->kind == GL_INTERPOL) return fail(GL_EINVAL, "GL_INTERPOL needs its image: use gl_interpol_eval");
  const bool mass = comp->kind <= GL_DPIEP || comp->kind == GL_NFW_ELLIPSE || comp->kind == GL_TNFW;
  if (mass && !out1) return fail(GL_EINVAL, "out1 is required for mass profiles");
  const CompDesc cd = point_comp(comp);
  hipStream_t stream = (hipStream_t)hip_stream;
  float* s_tab = nullptr;
  int s_stride = 0, rc_tab = 0;
  if (cd.kind == GL_SHAPELETS && (cd.iparam < 0 || cd.iparam > GL_SHAPELETS_NMAX_CAP))
    return fail(GL_EUNSUPPORTED, "shapelets n_max=%d outside [0,%d]", cd.iparam, GL_SHAPELETS_NMAX_CAP);
  if (cd.kind == GL_SHAPELETS && (cd.flags & GL_FLAG_SHAPELETS_INTERPOLATE) && (rc_tab = point_shapelet_table(&s_tab, &s_stride)))
    return rc_tab;
  long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, cd, x, y,
                     (long long)n_pts, B, xy_batched, params, out0, mass ? out1 : nullptr, s_tab, s_stride, InterpDev{nullptr, 0, 0});
  GL_HIP(hipGetLastError());
  return GL_OK;
}


#ifdef GL_EIGH_STAMPS
int gl_debug_eigh_stamps(long long* out) {
  GL_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(glk::g_eigh_stamps), sizeof(long long) * 8));
  return GL_OK;
}
#endif

int gl_adam_update(float* x, const float* grad, float* m, float* v, int64_t n, float grad_scale, float lr, float beta1,
                   float beta2, float eps, int64_t t, double* t_dev_or_null, void* hip_stream) {
  if (!x || !grad || !m || !v) return fail(GL_EINVAL, "null argument");
  if (n <= 0) return fail(GL_EINVAL, "n must be positive");
  if (!t_dev_or_null && t < 1) return fail(GL_EINVAL, "the step count t starts at 1");
  // t_dev layout: [0] the counter as a double, [1] 8 bytes of launch ticket (zero-initialised by the caller)
  unsigned* ticket = t_dev_or_null ? reinterpret_cast<unsigned*>(t_dev_or_null + 1) : nullptr;
  const float c1 = (float)(1.0 - std::pow((double)beta1, (double)t)), c2 = (float)(1.0 - std::pow((double)beta2, (double)t));
  hipLaunchKernelGGL(gl_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, x, grad, m,
                     v, (long long)n, grad_scale, lr, beta1, beta2, eps, (double)t, t_dev_or_null, ticket, c1, c2);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_svi_sample(const float* mu, const float* l_packed, int d, int full_rank, const float* eps, int n, float diag_shift,
                  float* z, void* hip_stream) {
  if (!mu || !l_packed || !eps || !z) return fail(GL_EINVAL, "null argument");
  if (d <= 0 || n <= 0) return fail(GL_EINVAL, "d and n must be positive");
  const long long total = (long long)n * d;
  hipLaunchKernelGGL(gl_svi_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, mu,
                     l_packed, d, full_rank, eps, n, diag_shift, z);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_svi_grad(const float* l_packed, int d, int full_rank, const float* eps, const float* logp, const float* grad_z, int n,
                float diag_shift, float* buf, void* hip_stream) {
  if (!l_packed || !eps || !logp || !grad_z || !buf) return fail(GL_EINVAL, "null argument");
  if (d <= 0 || n <= 0) return fail(GL_EINVAL, "d and n must be positive");
  const int n_out = 1 + d + (full_rank ? d * (d + 1) / 2 : d);
  hipLaunchKernelGGL(gl_svi_grad_kernel, dim3(n_out), dim3(256), 0, (hipStream_t)hip_stream, l_packed, d, full_rank, eps,
                     logp, grad_z, n, diag_shift, buf);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_hmc_kick_drift(const float* p_in, const float* grad, float kick, const float* z_in, const float* sigma, float eps, int n,
                      int d, float* p_out, float* z_out, void* hip_stream) {
  if (!p_in || !grad || !z_in || !sigma || !p_out || !z_out) return fail(GL_EINVAL, "null argument");
  if (n <= 0 || d <= 0 || d > 4096) return fail(GL_EINVAL, "n must be positive and d in [1, 4096]");
  hipLaunchKernelGGL(gl_hmc_kick_drift_kernel, dim3(n), dim3(HMC_WG), sizeof(float) * d, (hipStream_t)hip_stream, p_in, grad,
                     kick, z_in, sigma, eps, n, d, p_out, z_out);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_hmc_accept(float* z, float* grad, float* logp, const float* z_new, const float* grad_new, const float* logp_new,
                  const float* p0, const float* p_new, float kick, const float* scale_tril, const float* uniforms, int n, int d,
                  float* accept_prob, void* hip_stream) {
  if (!z || !grad || !logp || !z_new || !grad_new || !logp_new || !p0 || !p_new || !scale_tril || !uniforms || !accept_prob)
    return fail(GL_EINVAL, "null argument");
  if (n <= 0 || d <= 0 || d > 4096) return fail(GL_EINVAL, "n must be positive and d in [1, 4096]");
  hipLaunchKernelGGL(gl_hmc_accept_kernel, dim3(n), dim3(HMC_WG), sizeof(float) * 2 * d, (hipStream_t)hip_stream, z, grad, logp,
                     z_new, grad_new, logp_new, p0, p_new, kick, scale_tril, uniforms, n, d, accept_prob);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_profile_basis(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                     const float* params, float* out, void* hip_stream) {
  if (!comp || !x || !y || !params || !out) return fail(GL_EINVAL, "null argument");
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  int npar = kind_num_params(comp->kind, comp->iparam);
  if (npar < 0) return fail(GL_EINVAL, "unknown profile kind %d", comp->kind);
  if (kind_num_linear(comp->kind, comp->iparam) <= 0) return fail(GL_EINVAL, "kind %d has no linear amplitudes", comp->kind);
  if (comp->kind == GL_INTERPOL) return fail(GL_EINVAL, "GL_INTERPOL needs its image: use gl_interpol_eval");
  const CompDesc cd = point_comp(comp);
  float* s_tab = nullptr;
  int s_stride = 0, rc_tab = 0;
  if (cd.kind == GL_SHAPELETS) {
    if (cd.iparam < 0 || cd.iparam > GL_SHAPELETS_NMAX_CAP)
      return fail(GL_EUNSUPPORTED, "shapelets n_max=%d outside [0,%d]", cd.iparam, GL_SHAPELETS_NMAX_CAP);
    if ((cd.flags & GL_FLAG_SHAPELETS_INTERPOLATE) && (rc_tab = point_shapelet_table(&s_tab, &s_stride))) return rc_tab;
  }
  long long total = (long long)n_pts * B;
  hipLaunchKernelGGL(gl_basis_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     cd, x, y, (long long)n_pts, B, xy_batched, params, out, s_tab, s_stride, InterpDev{nullptr, 0, 0});
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
