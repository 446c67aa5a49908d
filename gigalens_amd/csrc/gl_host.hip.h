// gl_host.hip.h -- what the host units of libgigalens_hip.so share (gigalens_hip.hip and the gl_api_*.hip units, one per feature
// family): the launch plan and the workspace of a pixel-grid call, its argument checks, and the launchers of the kernels that only
// ONE unit compiles -- front end, finalize and PSF + pooling in gigalens_hip.hip, the point family in gl_api_points.hip.  A unit
// calls these and never includes another unit's kernel header: every kernel lives in one code object.  All of hidden visibility.
#pragma once
#include "gl_model.h"

#define GL_INTERNAL __attribute__((visibility("hidden")))

namespace glk {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The launch shape of one call on B samples.  Computed once per entry point and passed down: the workspace layout (carve), the
// rank the front end's sort splits at (run_prep) and the main kernel's grid (run_likelihood) all read the same plan.
struct LaunchPlan {
  int chunk, n_chunks;  // pixels per workgroup, workgroups per sample (chunking)
  int tail_rows;        // workgroups per sample of the tapered end, 0 = the shape has none (tail_plan)
  int tail_from;        // first rank of the tapered end (B without one)
  int n_rows;           // partial rows a sample owns in the workspace: max(n_chunks, tail_rows)
};
GL_INTERNAL LaunchPlan launch_plan(const gl_model* m, int B);

struct Workspace {
  float* derived;
  float* partial;
  float* params;  // [B,P] constrained rows produced from z (gl_logprob_fwd_bwd)
  int* order;     // [B] cost-ordered dispatch
  int* cost;      // [B] per-sample dispatch cost written by prep (single-EPL models)
  float* gal_dyn;  // [B][G][DP_ND] catalogue members' per-sample constants
  float *pos_w, *pos_adj, *pos_g, *pos_fam, *pos_ll, *pos_chi2, *pos_grad;  // image-position likelihood
  float* pos_dadj;  // [B][J] d loglike / d Fermat potential of the time-delay term (gl_tdelays.hip.h)
  // the time-delay term on lens planes (gl_multiplane_tdelays.hip.h), only while the model holds plane delays: the traced rays
  // [B][J][5], mean beta [B][F][2] and a_j [B][J]
  double *mpd_trace, *mpd_src, *mpd_aj;
  float* img_ss;   // supersampled / pre-PSF image or its cotangent (PSF path only)
  float* img_tmp;  // final-resolution image / its cotangent (PSF path only)
  float* stats;    // [B][2] chi2, normalisation of the materialised image (PSF path only)
  size_t bytes;
};
// (the partial rows are sized for the tapered end whenever the shape has one, whether or not the call at hand uses it)
GL_INTERNAL Workspace carve(const gl_model* m, int B, void* base, const LaunchPlan& plan);
GL_INTERNAL MainArgs base_args(const gl_model* m, const Workspace& w, int chunk);

// "The model is ready": every GL_SCALED lens has its catalogue, every GL_INTERPOL light its image and (with_series) every GL_SERIES
// lens its coefficient field.  The pixel-grid entry points report how many are missing and the call that attaches them
// (counted = true), the others name the kind.
GL_INTERNAL int check_ready(const gl_model* m, bool with_series, bool counted);
// A model with lens planes (gl_model_set_lens_planes) is served by the gl_multiplane_* entries alone: every single-plane entry
// refuses it instead of tracing its lenses as if they shared a plane -- and the multi-plane entries refuse a model without planes.
GL_INTERNAL int refuse_planes(const gl_model* m, const char* what);
inline int check_planes_set(const gl_model* m) {
  return m->mp_K >= 2 ? GL_OK : fail(GL_EINVAL, "gl_model_set_lens_planes has not been called on this model");
}
// the arguments every pixel-grid call shares; on success the call's launch plan and its workspace, carved
GL_INTERNAL int check_call(const gl_model* m, const void* params, int B, void* ws, size_t ws_bytes, LaunchPlan* plan, Workspace* w);
// n deflection scales: finite and > 0; *any = some scale differs from 1
GL_INTERNAL int check_scales(const float* scales, int n, int expect, const char* what, bool* any);

// The front end of a call: derived constants, dispatch cost and (wavefront form) the cost order of every sample, then the catalogue
// members' constants.  The rows come packed (`params` [B,P], z null) or unconstrained (`z` [B,d_z], params null: the constrained
// rows are written to w.params through the model's bijectors).
GL_INTERNAL int run_prep(const gl_model* m, const float* params, const float* z, int B, const LaunchPlan& plan, const Workspace& w,
                         hipStream_t stream);
GL_INTERNAL int run_finalize(const gl_model* m, const float* params, int B, int n_chunks, const Workspace& w, float* loglike,
                             float* chi2, float* grad, hipStream_t stream, const float* z = nullptr, float* logprob = nullptr,
                             float* grad_z = nullptr, float chi2_scale = 1.f, const float* extra_stats = nullptr,
                             int use_partial = 1, bool with_positions = false, float pos_chi2_scale = 0.f);
// heaviest samples first (only EPL has a data-dependent cost)
GL_INTERNAL int run_order(const gl_model* m, int B, const Workspace& w, MainArgs* a, hipStream_t stream);

// PSF + pooling (gl_post.hip.h): supersampled pre-PSF image S [B,Hs,Ws] -> final image [B,H,W] (x scale), and the transpose:
// cotangent of the final image [B,H,W] -> cotangent of S [B,Hs,Ws]
GL_INTERNAL int post_fwd(const gl_model* m, int B, const float* S, float* out, hipStream_t stream, float scale);
GL_INTERNAL int post_bwd(const gl_model* m, int B, const float* gP, float* gS, hipStream_t stream, float scale);

// ---- gl_api_points.hip --------------------------------------------------------------------------------------------------
// point-image likelihood on the packed parameter rows `params` [B,P] (already on the device): the image positions, the flux ratios
// of a model that holds fluxes (gl_model_set_position_fluxes), the time delays of one that holds arrival times
// (gl_model_set_position_delays; on lens planes gl_model_set_position_plane_delays, POS_PLANE_DELAYS) or any sum of them, in
// w.pos_ll / pos_chi2 / pos_grad.  amp [B][F] and model_flux [B][J]: the flux
// term's optional outputs (S_f, S_f m_j), or null; delay_out: those of the delay term (lambda_f, T_f [B][F], model delays [B][J])
enum PosTerms { POS_POSITIONS = 1, POS_FLUXES = 2, POS_BOTH = 3, POS_DELAYS = 4, POS_PLANE_DELAYS = 8 };
struct DelayOut { float *scale, *offset, *model_delay; };
GL_INTERNAL int run_positions(const gl_model* m, const float* params, int B, const Workspace& w, bool want_grad, hipStream_t stream,
                              int what = POS_POSITIONS, float* amp = nullptr, float* model_flux = nullptr,
                              const DelayOut* delay_out = nullptr);
// the model's image of `parts` on its lens planes: into `img` [B][H][W] (x conversion factor), through the PSF + pooling launch of
// the single-plane render where the model has one
GL_INTERNAL int mp_render(const gl_model* m, const float* params, int B, unsigned parts, float* img, const Workspace& w,
                          hipStream_t stream);
// The VJP of mp_render's kernel: cotangent `gimg` [B][Hs Ws] of the supersampled frame (x out_scale) -> one row of accumulators
// per (sample, chunk of the plan) in w.partial, for run_finalize.  Reads w.derived: run_prep comes first.
GL_INTERNAL int mp_render_bwd(const gl_model* m, int B, const LaunchPlan& plan, const Workspace& w, const float* gimg, float out_scale,
                              hipStream_t stream);

// ---- gl_api_plugin.hip --------------------------------------------------------------------------------------------------
// a free-standing component as the point kernels take it (an EPL without a series length gets the default, epl.py:15)
GL_INTERNAL CompDesc point_comp(const gl_component* comp);
// The catalogue arguments of the plugin-level calls, in the order they are reported: base kind, sizes (`sizes_ok`: the caller's own
// counts), the series order (`order`; 0 where there is none), the scale columns.  `series`: the wording of the series calls.
GL_INTERNAL int check_catalogue_args(bool series, int base_kind, bool sizes_ok, int order, const int32_t scale_col[3], int n_scales);

}  // namespace glk
