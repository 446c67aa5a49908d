// gigalens_hip.hip -- the core of the C ABI (include/gigalens_hip.h): models, the launch plan and workspace of a call, front end,
// finalize and PSF + pooling launchers, the render / likelihood / log-prob entries.  The other feature families have a unit each
// (gl_api_*.hip) and reach this one through gl_host.hip.h.  gfx950 only.  No per-call allocation, no host synchronisation: every entry point enqueues on
// the caller's stream and returns (hipGraph-capturable).
#include <algorithm>
#include <cmath>
#include <memory>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "gl_host_tables.h"
#include "gl_host.hip.h"
#include "gl_static.hip.h"
#include "gl_post.hip.h"
#include "gl_frontend.hip.h"
#include "gl_finalize.hip.h"

using namespace glk;

static thread_local char g_err[512] = "";

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

int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

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

}  // namespace

namespace glk {  // ---- what the other host units call (gl_host.hip.h)

LaunchPlan launch_plan(const gl_model* m, int B) {
  LaunchPlan p{};
  chunking(m, B, &p.chunk, &p.n_chunks);
  p.tail_rows = tail_plan(m, B, p.n_chunks, &p.tail_from, &p.n_rows);
  return p;
}

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
    w.pos_dadj = take((size_t)B * m->pos_J);  // (with or without delays: gl_model_set_position_delays leaves the layout alone)
    if (m->mpd_n_delay) {  // delays on lens planes (gl_model_set_position_plane_delays): every other model keeps its size
      auto wide = [&](size_t n) { double* q = (double*)(p + off); off += align_up(n * sizeof(double), 256); return q; };
      w.mpd_trace = wide((size_t)B * m->pos_J * 5);
      w.mpd_src = wide((size_t)B * m->pos_F * 2);
      w.mpd_aj = wide((size_t)B * m->pos_J);
    }
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
  a.careful_tiles = m->careful_tiles;
  a.shp_stride = m->shp_stride;
  a.parts = 7u;
  a.cats = m->d_cats;
  a.gal_static = m->d_gal_static;
  a.gal_dyn = w.gal_dyn;
  a.G = m->G;
  a.scaled_first = m->cats.empty() ? -1 : m->cats[0].dev.comp;
  a.series = m->d_series;
  a.interp = m->d_interp;
  a.interp_mass = m->d_interp_mass;
  a.src_scale = m->src_scaled ? m->d_src_scale.get() : nullptr;
  return a;
}

int check_ready(const gl_model* m, bool with_series, bool counted) {
  const int no_cat = m->n_scaled - (int)m->cats.size(), no_field = m->n_series - m->n_series_set;
  if (no_cat)
    return counted ? fail(GL_EINVAL, "%d GL_SCALED component(s) without a catalogue (gl_model_set_catalogue)", no_cat)
                   : fail(GL_EINVAL, "GL_SCALED component without a catalogue");
  if (m->n_interp != m->n_interp_set)
    return fail(GL_EINVAL, "%d GL_INTERPOL component(s) without an image (gl_model_set_light_image)", m->n_interp - m->n_interp_set);
  if (m->n_interp_mass != m->n_interp_mass_set)
    return fail(GL_EINVAL, "%d GL_INTERPOL_MASS component(s) without deflection maps (gl_model_set_lens_maps)",
                m->n_interp_mass - m->n_interp_mass_set);
  if (with_series && no_field)
    return counted ? fail(GL_EINVAL, "%d GL_SERIES component(s) without a coefficient field (gl_model_set_series)", no_field)
                   : fail(GL_EINVAL, "GL_SERIES component without a coefficient field");
  return GL_OK;
}

int refuse_planes(const gl_model* m, const char* what) {
  if (m && m->mp_K >= 2)
    return fail(GL_EUNSUPPORTED, "%s does not serve a model with %d lens planes (gl_model_set_lens_planes): lens maps, renders, "
                                 "pixel statistics and their gradients through the gl_multiplane_* entries alone", what, m->mp_K);
  return GL_OK;
}

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
    // LDS: one parameter row per wavefront of the workgroup (0: rows too long, read back from global memory)
    const size_t row_bytes = (size_t)4 * m->P * sizeof(float), rows = (m->prep_lds && row_bytes <= 48 * 1024) ? row_bytes : 0;
    // the rank the sort must split deterministically: which samples run the tapered end may not depend on the order the atomics
    // of the counting sort leave inside a cost bin
    const int split_rank = plan.tail_rows ? plan.tail_from : -1;
    hipLaunchKernelGGL(gl_prep_wave_kernel, dim3((B + 3) / 4 + (ord ? 1 : 0)), dim3(256), rows, stream, m->d_comps.get(), n_comp,
                       params, z, d_z, zcols, src, const_row, m->P, B, rows_out, w.derived, m->D, cost, m->epl_comp,
                       ord ? w.order : nullptr, rows ? 1 : 0, split_rank, m->d_interp.get(), m->d_interp_mass.get());
  } else {  // thread per component
    hipLaunchKernelGGL(gl_prep_kernel, dim3((B * n_comp + 127) / 128), dim3(128), 0, stream, m->d_comps.get(), n_comp, params, z,
                       d_z, zcols, src, const_row, m->P, B, rows_out, w.derived, m->D, cost, m->epl_comp, m->d_interp.get(),
                       m->d_interp_mass.get());
  }
  if (m->G) {  // per (sample, galaxy) constants of the catalogue members, from the constrained parameter rows
    const long long total = (long long)B * m->G;
    hipLaunchKernelGGL(gl_galprep_kernel, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, stream, m->d_comps, m->d_cats,
                       (int)m->cats.size(), z ? w.params : params, m->P, B, m->d_gal_table, m->d_gal_static, w.gal_dyn, m->G);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int run_finalize(const gl_model* m, const float* params, int B, int n_chunks, const Workspace& w, float* loglike,
                 float* chi2, float* grad, hipStream_t stream, const float* z, float* logprob, float* grad_z,
                 float chi2_scale, const float* extra_stats, int use_partial, bool with_positions, float pos_chi2_scale) {
  size_t shmem = (size_t)(((m->A + 3) & ~3) + ((m->P + 3) & ~3) + ((m->d_z + 3) & ~3) + 4 * m->d_z + 4 + m->P) * sizeof(float);
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
  bool basic = true;
  for (const CompDesc& c : m->comps)
    basic = basic && (c.kind == K_EPL || c.kind == K_SIE || c.kind == K_SHEAR || c.kind == K_SIS || c.kind == K_SERSIC || c.kind == K_SERSIC_ELLIPSE);
  const int nc = GL_DBG(m->dbg_flags, 8) ? -1 : n_chunks;
  if (basic) hipLaunchKernelGGL(gl_finalize_kernel<true>, dim3(B), dim3(128), shmem, stream, m->d_comps, f, w.partial, nc);
  else hipLaunchKernelGGL(gl_finalize_kernel<false>, dim3(B), dim3(128), shmem, stream, m->d_comps, f, w.partial, nc);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

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

}  // namespace glk

namespace {
int render_ss(const gl_model* m, MainArgs a, int B, int n_chunks, const Workspace& w, hipStream_t stream) {
  if (m->d_pix) GL_HIP(hipMemsetAsync(w.img_ss, 0, sizeof(float) * (size_t)B * m->height * m->width, stream));
  a.img = w.img_ss;
  a.out_scale = 1.f;  // NaN -> 0 happens in the kernel; the det(T) scale is applied after pooling (tf/simulator.py:156)
  return launch_main<IMG_FWD>(m, a, B, n_chunks, stream);
}

// Pixel likelihood after prep.  One plane without PSF / supersampling: the fused kernel, the image never has to exist.  Else the
// image is materialised: render (launch_main, or mp_render on lens planes, which reads the packed rows `params`) -> [PSF + pooling]
// -> pixel statistics (-> transposes -> VJP of the render).  Tells finalize where chi2 / normalisation come from.
// `fin_rows`: the partial rows per sample finalize must reduce (the plan's chunks, or its rows when the tapered end ran).
int run_likelihood(const gl_model* m, const float* params, int B, const LaunchPlan& plan, const Workspace& w, const float* obs,
                   const float* err, const float* mask, float bg_rms, float exp_time, bool want_grad,
                   hipStream_t stream, const float** extra_stats, int* use_partial, int* fin_rows) {
  int rc;
  const int n_chunks = plan.n_chunks;
  const bool planes = m->mp_K >= 2;
  MainArgs a = base_args(m, w, plan.chunk);
  a.obs = obs; a.err = err; a.mask = mask;
  a.bg2 = bg_rms * bg_rms; a.inv_t = 1.0f / exp_time;
  *extra_stats = nullptr; *use_partial = 1; *fin_rows = n_chunks;
  if (planes) {
    if ((rc = mp_render(m, params, B, 7u, w.img_tmp, w, stream))) return rc;
  } else {
    if ((rc = run_order(m, B, w, &a, stream))) return rc;
    if (!m->has_post && a.order && want_grad) {  // (the rounds are counted for the gradient kernels' occupancy; forward-only calls keep the plain grid)
      a.tail_rows = plan.tail_rows; a.tail_from = plan.tail_from;
      a.n_rows = plan.n_rows; a.n_samples = B;
      *fin_rows = plan.n_rows;
    }
    if (!m->has_post) return want_grad ? launch_main<LL_GRAD>(m, a, B, n_chunks, stream) : launch_main<LL_FWD>(m, a, B, n_chunks, stream);
    if ((rc = render_ss(m, a, B, n_chunks, w, stream))) return rc;
    if ((rc = post_fwd(m, B, w.img_ss, w.img_tmp, stream, m->conversion_factor))) return rc;
  }
  const int HW = (m->height / m->supersample) * (m->width / m->supersample);
  hipLaunchKernelGGL(gl_imgstats_kernel, dim3(B), dim3(256), 0, stream, w.img_tmp, obs, err, mask, a.bg2, a.inv_t, HW,
                     w.stats, want_grad ? w.img_tmp : nullptr);
  GL_HIP(hipGetLastError());
  *extra_stats = w.stats;
  *use_partial = want_grad ? 1 : 0;
  if (!want_grad) return GL_OK;
  // the cotangent of the frame the render wrote: the final image itself, or the supersampled one through the transposes
  const float* gimg = w.img_tmp;
  float out_scale = m->conversion_factor;
  if (m->has_post) {
    if ((rc = post_bwd(m, B, w.img_tmp, w.img_ss, stream, m->conversion_factor))) return rc;
    gimg = w.img_ss;
    out_scale = 1.f;
  }
  if (planes) return mp_render_bwd(m, B, plan, w, gimg, out_scale, stream);
  a.gimg = gimg;
  a.out_scale = out_scale;
  return launch_main<IMG_BWD>(m, a, B, n_chunks, stream);
}

// ---- the four pixel-grid pipelines: each serves the single-plane entries and their gl_multiplane_* twins and branches on
// m->mp_K >= 2 at the step that differs.  An entry is check_family plus one of them.
// check_family: the family check and the checks every pixel-grid call shares, in the order the entries report them -- a single-plane
// entry (`planes` false) refuses a model with planes first, a multi-plane entry a model without planes once the shared arguments
// are sound.  On success (m->mp_K >= 2) == planes.
struct Call { LaunchPlan plan; Workspace w; };
int check_family(const gl_model* m, bool planes, const char* what, const void* params, int B, void* ws, size_t ws_bytes, Call* c) {
  if (!planes)
    if (int rc = refuse_planes(m, what)) return rc;
  if (int rc = check_call(m, params, B, ws, ws_bytes, &c->plan, &c->w)) return rc;
  return planes ? check_planes_set(m) : GL_OK;
}

// the image of `parts` [B][H][W]
int render_parts(const gl_model* m, const float* params, int B, unsigned parts, float* img, const LaunchPlan& plan,
                 const Workspace& w, hipStream_t stream) {
  if (!img) return fail(GL_EINVAL, "img is null");
  if (parts == 0 || parts > 7u) return fail(GL_EINVAL, "parts must be a non-empty subset of {1,2,4}");
  if (m->mp_K >= 2) return mp_render(m, params, B, parts, img, w, stream);  // (from the packed rows themselves: no front end)
  int rc;
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

// the VJP of render_parts (every part): cotangent `grad_img` [B][H][W] -> `grad_params` [B][P]
int render_vjp(const gl_model* m, const float* params, const float* grad_img, int B, float* grad_params, const LaunchPlan& plan,
               const Workspace& w, hipStream_t stream) {
  if (!grad_img || !grad_params) return fail(GL_EINVAL, "grad_img / grad_params is null");
  int rc;
  if ((rc = run_prep(m, params, nullptr, B, plan, w, stream))) return rc;
  const float* gimg = grad_img;
  float out_scale = m->conversion_factor;
  if (m->has_post) {
    if ((rc = post_bwd(m, B, grad_img, w.img_ss, stream, m->conversion_factor))) return rc;
    gimg = w.img_ss;
    out_scale = 1.f;
  }
  if (m->mp_K >= 2) {
    if ((rc = mp_render_bwd(m, B, plan, w, gimg, out_scale, stream))) return rc;
  } else {
    MainArgs a = base_args(m, w, plan.chunk);
    a.gimg = gimg;
    a.out_scale = out_scale;
    if ((rc = run_order(m, B, w, &a, stream))) return rc;
    if ((rc = launch_main<IMG_BWD>(m, a, B, plan.n_chunks, stream))) return rc;
  }
  return run_finalize(m, params, B, plan.n_chunks, w, nullptr, nullptr, grad_params, stream);
}

// pixel log-likelihood and chi2 [B] of the packed rows, with d loglike / d params [B][P] when `grad_params` is given
int loglike_grad(const gl_model* m, const float* params, const float* obs, const float* err, const float* mask, float bg_rms,
                 float exp_time, int B, float* loglike, float* chi2, float* grad_params, const LaunchPlan& plan, const Workspace& w,
                 hipStream_t stream) {
  if (!obs || !loglike || !chi2) return fail(GL_EINVAL, "obs / loglike / chi2 is null");
  int rc;
  const bool want_grad = grad_params != nullptr;
  // (the forward render on lens planes reads the packed rows themselves: no front end)
  if ((m->mp_K < 2 || want_grad) && (rc = run_prep(m, params, nullptr, B, plan, w, stream))) return rc;
  const float* extra = nullptr;
  int use_partial = 1, fin_rows = plan.n_chunks;
  if ((rc = run_likelihood(m, params, B, plan, w, obs, err, mask, bg_rms, exp_time, want_grad, stream, &extra, &use_partial, &fin_rows)))
    return rc;
  return run_finalize(m, params, B, fin_rows, w, loglike, chi2, grad_params, stream, nullptr, nullptr, nullptr, 1.f, extra, use_partial);
}

// log-prob of the unconstrained rows z [B][d_z]: bijectors -> likelihood term(s) -> finalize with the prior, d logprob / d z when
// `grad_z` is given.  `chi2`: the reduced chi2 over the terms (tf/model.py:150-162).
int logprob_grad(const gl_model* m, const float* z, const float* obs, const float* err, const float* mask, float bg_rms,
                 float exp_time, int B, float* logprob, float* loglike, float* chi2, float* grad_z, float chi2_divisor, unsigned terms,
                 const LaunchPlan& plan, const Workspace& w, hipStream_t stream) {
  const bool planes = m->mp_K >= 2;
  const bool pix = terms & GL_TERM_PIXELS, pos = terms & GL_TERM_POSITIONS;
  if (!pix && !pos) return fail(GL_EINVAL, "terms selects no likelihood term");
  if (pix && !(chi2_divisor > 0.f)) return fail(GL_EINVAL, "chi2_divisor must be positive");
  if (!m->d_zcols) return fail(GL_EINVAL, "gl_model_set_prior has not been called on this model");
  if (pos && !m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if (pos && planes && !m->pos_targets)
    return fail(GL_EINVAL, "the image positions of a model with lens planes need the couplings of their families: "
                           "gl_model_set_position_targets has not been called");
  if ((pix && !obs) || !logprob || !loglike || !chi2)
    return fail(GL_EINVAL, "obs / logprob / loglike / %s is null", planes ? "red_chi2" : "chi2");
  int rc;
  const bool want_grad = grad_z != nullptr;
  if ((rc = run_prep(m, nullptr, z, B, plan, w, stream))) return rc;  // constrained rows -> w.params, derived rows
  const float* extra = nullptr;
  int use_partial = 0, fin_rows = plan.n_chunks;
  // red_chi2 = (red_pix + red_pos) / n_chi  (tf/model.py:150-162)
  const float n_chi = (pix ? 1.f : 0.f) + (pos ? 1.f : 0.f);
  if (pix && (rc = run_likelihood(m, w.params, B, plan, w, obs, err, mask, bg_rms, exp_time, want_grad, stream, &extra, &use_partial,
                                  &fin_rows)))
    return rc;
  // a model that holds fluxes (gl_model_set_position_fluxes): the flux ratios are part of the point-image term, whose reduced chi2
  // then divides by 2 J + n_flux
  // ... and likewise the time delays of a model that holds arrival times (gl_model_set_position_delays): 2 J + n_flux + n_delay
  // ... on lens planes those of gl_model_set_position_plane_delays
  const bool flux = pos && m->pos_n_flux > 0, delays = pos && m->pos_n_delay > 0, plane_delays = pos && planes && m->mpd_n_delay > 0;
  if (pos && (rc = run_positions(m, w.params, B, w, want_grad, stream,
                                 (flux ? POS_BOTH : POS_POSITIONS) | (delays ? POS_DELAYS : 0) | (plane_delays ? POS_PLANE_DELAYS : 0))))
    return rc;
  float n_point = flux ? 2.0f * (float)m->pos_J + (float)m->pos_n_flux : 2.0f * (float)m->pos_J;
  if (delays) n_point += (float)m->pos_n_delay;
  if (plane_delays) n_point += (float)m->mpd_n_delay;
  return run_finalize(m, w.params, B, fin_rows, w, loglike, chi2, nullptr, stream, z, logprob, grad_z,
                      pix ? 1.0f / (chi2_divisor * n_chi) : 0.f, extra, use_partial, pos,
                      pos ? 1.0f / (n_point * n_chi) : 0.f);
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
    const bool is_mass_kind = (c.kind >= GL_EPL && c.kind <= GL_TNFW) || c.kind == GL_USER_MASS || c.kind == GL_INTERPOL_MASS || c.kind == GL_MULTIPOLE;
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
    if (c.kind == GL_NFW_ELLIPSE || c.kind == GL_TNFW || c.kind == GL_CORE_SERSIC || c.kind == GL_INTERPOL || c.kind == GL_INTERPOL_MASS ||
        c.kind == GL_MULTIPOLE)
      m->fam = 2;
    if (c.kind == GL_SERIES && (iparam < 0 || iparam > SERIES_MAX_ORDER))
      return fail(GL_EINVAL, "component %d: series order %d outside [0, %d]", i, iparam, SERIES_MAX_ORDER);
    if (c.kind == GL_MULTIPOLE) {
      if (iparam < MPL_MMIN || iparam > MPL_MMAX)
        return fail(GL_EINVAL, "component %d: multipole order m = %d outside [%d, %d]", i, iparam, MPL_MMIN, MPL_MMAX);
      ++m->n_multipole;
    }
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
    if (c.kind == GL_INTERPOL_MASS) {  // table slot; the maps arrive with gl_model_set_lens_maps
      cd.iparam = m->n_interp_mass++;
      cd.flags = 0;
      m->interp_mass.push_back(InterpMassDev{nullptr, nullptr, 0, 0, 0.f});
      m->interp_mass_buf.emplace_back();
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
  if (m->has_user && m->n_interp_mass)
    return fail(GL_EUNSUPPORTED, "a model that mixes user-written profiles with GL_INTERPOL_MASS lenses is not served: the run-time "
                                 "compiled kernels carry no deflection maps");
  if (m->has_user && m->n_multipole)
    return fail(GL_EUNSUPPORTED, "a model that mixes user-written profiles with GL_MULTIPOLE lenses is not served: the run-time "
                                 "compiled kernels are built without that case");
  if (m->n_multipole && m->n_interp_mass)
    return fail(GL_EUNSUPPORTED, "a model that holds both GL_MULTIPOLE and GL_INTERPOL_MASS lenses is not served: each build of the "
                                 "position kernel carries one of the two cases");
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
  m->careful_tiles = env_int("GIGALENS_HIP_CAREFUL_TILES", 0) != 0;  // tests: 1 = no select-free whole tiles in the pair kernels (read once)
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
  const int kh = grid->psf ? grid->psf_h : 1, kw = grid->psf ? grid->psf_w : 1, ss = grid->supersample;
  m->psf_h = kh;
  m->psf_w = kw;
  {  // the PSF as given inside a two-node zero apron: the table of the point-image kernels (gl_ptimg.hip.h)
    std::vector<float> tab((size_t)(kh + 4) * (kw + 4), 0.f);
    for (int u = 0; u < kh; ++u)
      for (int v = 0; v < kw; ++v) tab[(size_t)(u + 2) * (kw + 4) + v + 2] = grid->psf ? grid->psf[(size_t)u * kw + v] : 1.f;
    if (int rc = put(m->d_ptimg_tab, tab.data(), tab.size())) return rc;
  }
  if (!m->has_post) return GL_OK;
  // flat = flip(psf) cross-correlated with SAME padding (tf/simulator.py:62-70,145-147), then box(ss)/ss^2 pooling
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

int gl_model_workspace_layout(const gl_model* m, int B, int component, gl_workspace_layout* out) {
  if (!m || !out) return fail(GL_EINVAL, "null argument");
  if (B < 1 || B > 65535) return fail(GL_EINVAL, "batch size %d outside [1, 65535]", B);
  if (component < -1 || component >= (int)m->comps.size()) return fail(GL_EINVAL, "component index out of range");
  const Workspace w = carve(m, B, nullptr, launch_plan(m, B));  // the carve of every call on B samples: nothing is launched
  auto off = [](const void* p) { return (size_t)((const char*)p - (const char*)nullptr); };
  *out = gl_workspace_layout{};
  out->params_offset = off(w.params);
  out->derived_offset = off(w.derived);
  out->order_offset = off(w.order);
  out->cost_offset = off(w.cost);
  out->params_count = (size_t)B * m->P;
  out->derived_count = (size_t)B * m->D;
  out->order_count = (size_t)B;
  out->cost_count = (size_t)B;
  out->P = m->P;
  out->D = m->D;
  out->p_off = component >= 0 ? m->comps[component].p_off : -1;
  out->d_off = component >= 0 ? m->comps[component].d_off : -1;
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
  Call c;
  if (int rc = check_family(m, false, "gl_simulate_parts_fwd", params, B, workspace, workspace_bytes, &c)) return rc;
  return render_parts(m, params, B, parts, img, c.plan, c.w, (hipStream_t)hip_stream);
}

int gl_multiplane_simulate(const gl_model* m, const float* params, int B, unsigned parts, float* img, void* workspace,
                           size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, true, "gl_multiplane_simulate", params, B, workspace, workspace_bytes, &c)) return rc;
  return render_parts(m, params, B, parts, img, c.plan, c.w, (hipStream_t)hip_stream);
}

int gl_simulate_bwd(const gl_model* m, const float* params, const float* grad_img, int B, float* grad_params,
                    void* workspace, size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, false, "gl_simulate_bwd", params, B, workspace, workspace_bytes, &c)) return rc;
  return render_vjp(m, params, grad_img, B, grad_params, c.plan, c.w, (hipStream_t)hip_stream);
}

int gl_multiplane_simulate_bwd(const gl_model* m, const float* params, const float* grad_img, int B, float* grad_params,
                               void* workspace, size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, true, "gl_multiplane_simulate_bwd", params, B, workspace, workspace_bytes, &c)) return rc;
  return render_vjp(m, params, grad_img, B, grad_params, c.plan, c.w, (hipStream_t)hip_stream);
}

int gl_loglike_fwd_bwd(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                       const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                       float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, false, "gl_loglike_fwd_bwd", params, B, workspace, workspace_bytes, &c)) return rc;
  return loglike_grad(m, params, obs, err_or_null, mask_or_null, bg_rms, exp_time, B, loglike, chi2, grad_params_or_null, c.plan, c.w,
                      (hipStream_t)hip_stream);
}

int gl_multiplane_loglike_fwd_bwd(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                                  const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                                  float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, true, "gl_multiplane_loglike_fwd_bwd", params, B, workspace, workspace_bytes, &c)) return rc;
  return loglike_grad(m, params, obs, err_or_null, mask_or_null, bg_rms, exp_time, B, loglike, chi2, grad_params_or_null, c.plan, c.w,
                      (hipStream_t)hip_stream);
}

int gl_multiplane_loglike(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                          const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                          void* workspace, size_t workspace_bytes, void* hip_stream) {
  return gl_multiplane_loglike_fwd_bwd(m, params, obs, err_or_null, mask_or_null, bg_rms, exp_time, B, loglike, chi2, nullptr, workspace,
                                       workspace_bytes, hip_stream);  // the forward half: the same launches, no front end, no VJP
}

int gl_logprob_fwd_bwd(const gl_model* m, const float* z, const float* obs, const float* err_or_null,
                       const float* mask_or_null, float bg_rms, float exp_time, int B, float* logprob, float* loglike,
                       float* chi2, float* grad_z_or_null, float chi2_divisor, unsigned terms, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, false, "gl_logprob_fwd_bwd", z, B, workspace, workspace_bytes, &c)) return rc;
  return logprob_grad(m, z, obs, err_or_null, mask_or_null, bg_rms, exp_time, B, logprob, loglike, chi2, grad_z_or_null, chi2_divisor,
                      terms, c.plan, c.w, (hipStream_t)hip_stream);
}

int gl_multiplane_logprob_fwd_bwd(const gl_model* m, const float* z, const float* obs, const float* err_or_null,
                                  const float* mask_or_null, float bg_rms, float exp_time, int B, float* logprob, float* loglike,
                                  float* red_chi2, float* grad_z_or_null, float chi2_divisor, unsigned terms, void* workspace,
                                  size_t workspace_bytes, void* hip_stream) {
  Call c;
  if (int rc = check_family(m, true, "gl_multiplane_logprob_fwd_bwd", z, B, workspace, workspace_bytes, &c)) return rc;
  return logprob_grad(m, z, obs, err_or_null, mask_or_null, bg_rms, exp_time, B, logprob, loglike, red_chi2, grad_z_or_null,
                      chi2_divisor, terms, c.plan, c.w, (hipStream_t)hip_stream);
}

int gl_model_num_linear(const gl_model* m) { return m ? (int)m->lin_cols.size() : fail(GL_EINVAL, "model is null"); }
int gl_model_linear_column(const gl_model* m, int k) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (k < 0 || k >= (int)m->lin_cols.size()) return fail(GL_EINVAL, "linear coefficient index out of range");
  return m->lin_cols[k];
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

int gl_model_set_lens_maps(gl_model* m, int component, int h, int w, const float* alpha_x_host, const float* alpha_y_host, double pitch) {
  if (!m || !alpha_x_host || !alpha_y_host) return fail(GL_EINVAL, "null argument");
  if (component < 0 || component >= m->n_lens || m->comps[component].kind != K_INTERPOL_MASS)
    return fail(GL_EINVAL, "component %d is not a GL_INTERPOL_MASS lens", component);
  if (h < 1 || h > GL_INTERPOL_MAX_SIDE || w < 1 || w > GL_INTERPOL_MAX_SIDE)
    return fail(GL_EINVAL, "deflection maps of %d x %d pixels: height and width must lie in 1..%d", h, w, GL_INTERPOL_MAX_SIDE);
  if (!(std::isfinite(pitch) && pitch > 0.0 && std::isfinite((float)(1.0 / pitch)) && (float)(1.0 / pitch) > 0.f))
    return fail(GL_EINVAL, "pitch %g is not finite and > 0", pitch);
  for (size_t i = 0; i < (size_t)h * w; ++i)
    if (!std::isfinite(alpha_x_host[i]) || !std::isfinite(alpha_y_host[i])) return fail(GL_EINVAL, "deflection map pixel %zu is not finite", i);
  // both maps in one buffer, each with the two-pixel zero apron of gl_model_set_light_image; everything that can refuse the call
  // has done so by here, and the slot changes only after the upload
  const int ws = w + 2 * glp::INT_APRON, hs = h + 2 * glp::INT_APRON;
  const size_t plane = (size_t)hs * ws;
  std::vector<float> padded(2 * plane, 0.f);
  for (int j = 0; j < h; ++j) {
    const size_t to = (size_t)(j + glp::INT_APRON) * ws + glp::INT_APRON;
    std::copy(alpha_x_host + (size_t)j * w, alpha_x_host + (size_t)(j + 1) * w, padded.begin() + to);
    std::copy(alpha_y_host + (size_t)j * w, alpha_y_host + (size_t)(j + 1) * w, padded.begin() + plane + to);
  }
  const int slot = m->comps[component].iparam;
  glk::DevBuf<float> fresh;
  GL_HIP(fresh.upload(padded.data(), padded.size()));
  if (!m->d_interp_mass) GL_HIP(m->d_interp_mass.alloc(m->interp_mass.size()));
  std::vector<InterpMassDev> tabs = m->interp_mass;
  tabs[slot] = InterpMassDev{fresh.get(), fresh.get() + plane, h, w, (float)(1.0 / pitch)};
  GL_HIP(m->d_interp_mass.write(tabs.data(), tabs.size()));
  const bool first = !m->interp_mass_buf[slot];
  m->interp_mass_buf[slot] = std::move(fresh);
  m->interp_mass = std::move(tabs);
  if (first) ++m->n_interp_mass_set;
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
  m->pos_targets = false;  // ... and, behind lens planes, without couplings until gl_model_set_position_targets
  m->d_pos_target.reset();
  m->pos_n_flux = 0;  // ... and without fluxes until gl_model_set_position_fluxes
  m->d_pos_flux.reset();
  m->pos_n_delay = 0;  // ... and without arrival times until gl_model_set_position_delays
  m->d_pos_delay.reset();
  m->pos_fam_delay.clear();
  m->pos_fam_scale.clear();
  m->clear_plane_delays();  // ... nor, on lens planes, those of gl_model_set_position_plane_delays
  m->pos_target_rows.clear();
  return GL_OK;
}

int gl_model_set_position_fluxes(gl_model* m, const float* flux, const float* flux_err, int n_images) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (!m->pos_J) return fail(GL_EINVAL, "gl_model_set_positions has not been called on this model");
  if (!flux) {  // no fluxes: the model as gl_model_set_positions left it
    m->pos_n_flux = 0;
    m->d_pos_flux.reset();
    return GL_OK;
  }
  if (!flux_err) return fail(GL_EINVAL, "flux_err is null");
  if (n_images != m->pos_J) return fail(GL_EINVAL, "%d fluxes for %d image(s)", n_images, m->pos_J);
  int n_flux = 0;
  for (int f = 0; f < m->pos_F; ++f) {
    int n = 0;
    for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) {
      if (std::isnan(flux[j])) continue;  // not measured
      if (!std::isfinite(flux[j])) return fail(GL_EINVAL, "flux %d (%g) is not finite", j, flux[j]);
      if (!(std::isfinite(flux_err[j]) && flux_err[j] > 0.f))
        return fail(GL_EINVAL, "flux error %d (%g) is not finite and > 0", j, flux_err[j]);
      ++n;
    }
    if (n == 1)
      return fail(GL_EINVAL, "image family %d has one measured flux: the term constrains flux ratios, a family takes two or more, or none", f);
    n_flux += n;
  }
  if (!n_flux) {  // every flux is NaN: none
    m->pos_n_flux = 0;
    m->d_pos_flux.reset();
    return GL_OK;
  }
  std::vector<float> tab((size_t)2 * m->pos_J);
  std::copy(flux, flux + m->pos_J, tab.begin());
  std::copy(flux_err, flux_err + m->pos_J, tab.begin() + m->pos_J);
  m->pos_n_flux = 0;
  GL_HIP(m->d_pos_flux.upload(tab.data(), tab.size()));
  m->pos_n_flux = n_flux;
  return GL_OK;
}

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
  if (m->mp_K >= 2)
    return fail(GL_EINVAL, "the model has lens planes (gl_model_set_lens_planes): one scale names no plane, the families take their "
                           "couplings from gl_model_set_position_targets");
  bool any;
  if (int rc = check_scales(scales, n_families, m->pos_F, "image famil(ies)", &any)) return rc;
  for (int f = 0; f < (int)m->pos_fam_delay.size(); ++f)
    if (m->pos_fam_delay[f] && scales[f] != 1.f)
      return fail(GL_EUNSUPPORTED, "image family %d holds arrival times (gl_model_set_position_delays): the Fermat potential of a "
                                   "scaled source plane (scale %g) is not served", f, scales[f]);
  if (any) {
    std::vector<float> per_image((size_t)m->pos_J);
    for (int f = 0; f < m->pos_F; ++f)
      for (int j = m->pos_fam_off[f]; j < m->pos_fam_off[f + 1]; ++j) per_image[j] = scales[f];
    GL_HIP(m->d_pos_scale.upload(per_image.data(), per_image.size()));
  } else {
    m->d_pos_scale.reset();
  }
  m->pos_scaled = any;
  m->pos_fam_scale.assign(scales, scales + n_families);  // (the host copy the delay setter reads: after the upload has succeeded)
  return GL_OK;
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

}  // extern "C"
