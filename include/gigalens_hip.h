/* gigalens_hip.h -- C ABI of the MI355X-native gigalens hot path.
 *
 * Plain pointers and sizes only: no torch / C++ types cross this boundary.
 * Every device buffer is owned by the caller (PyTorch in this repo); the
 * library allocates device memory only inside gl_model_create and the
 * gl_model_set_* set-up calls (model descriptor, grid, PSF, prior table, image
 * positions, galaxy catalogues, series fields) and never per compute call, so
 * every compute entry point is hipGraph-capturable.  All arithmetic is fp32, as in
 * the reference (two documented exceptions run in fp64: the one-off series
 * precompute and the core of the TNFW bracket)
 * (every constant there is tf.float32: tf/simulator.py:27-32,46-51;
 * tf/model.py:63-68,301-306).
 *
 * The reference (furcelay/gigalens) has no FFI -- its plugin boundary is a set
 * of Python ABCs.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference repo root).  INTEGRATION.md shows
 * the ctypes stub a reference maintainer would add.
 */
#ifndef GIGALENS_HIP_H
#define GIGALENS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error convention: 0 on success, negative gl_status otherwise; the message is
 * available through gl_last_error() (thread local).  Numerical NaN is data,
 * not an error (mirrors the reference: tf/simulator.py:140, tf/inference.py:44). */
typedef enum gl_status {
  GL_OK = 0,
  GL_EINVAL = -1,       /* bad argument (null pointer, negative size, unknown kind) */
  GL_EUNSUPPORTED = -2, /* valid request this build cannot serve */
  GL_ELAUNCH = -3,      /* HIP runtime / launch failure */
  GL_ENOMEM = -4,       /* allocation failure in gl_model_create, or workspace too small */
  GL_ENODEVICE = -5     /* no HIP device */
} gl_status;

/* Profile kinds.  Parameter order inside the packed parameter row is the
 * reference's `_params` list (+ `_amp` for light profiles, profile.py:40-41). */
typedef enum gl_kind {
  /* mass profiles: MassProfile.deriv (profile.py:63-82) */
  GL_EPL = 1,   /* tf/profiles/mass/epl.py:13   [theta_E,gamma,e1,e2,center_x,center_y] */
  GL_SIE = 2,   /* tf/profiles/mass/sie.py:8    [theta_E,e1,e2,center_x,center_y] */
  GL_NFW = 3,   /* tf/profiles/mass/nfw.py:8    [Rs,alpha_Rs,center_x,center_y] */
  GL_SHEAR = 4, /* tf/profiles/mass/shear.py:8  [gamma1,gamma2] */
  GL_SIS = 5,   /* tf/profiles/mass/sis.py:7    [theta_E,center_x,center_y] */
  GL_DPIS = 6,  /* tf/profiles/mass/piemd.py:27 [theta_E,r_core,r_cut,center_x,center_y] */
  GL_DPIE = 7,  /* tf/profiles/mass/piemd.py:99 [theta_E,r_core,r_cut,center_x,center_y,e1,e2] */
  GL_DPIEP = 8, /* tf/profiles/mass/piep.py:23  [theta_E,Ra,Rs,center_x,center_y,e1,e2] */
  GL_SCALED = 9, /* tf/profiles/mass/scaling_relation.py:6-70 (DPIESubhalo, dpie_subhalo.py:6-21): a catalogue of
                    galaxies of one dPIE-family profile whose theta_E / r_core / r_cut follow (L/L*)^power * scale;
                    the packed parameters are the scales, in the order of the reference's `scaling_params`;
                    iparam = their number (1..3); the catalogue is attached with gl_model_set_catalogue */
  GL_SERIES = 10, /* tf/series/series_profile.py:9-95 with dpie_series.py / scaling_series.py / dpie_subhalo_series.py:
                     the (scaled) dPIE deflection expanded in the cut radius around r0, precomputed on the model grid;
                     parameters [theta_E, r_cut]; iparam = order (0..5); field attached with gl_model_set_series */
  GL_NFW_ELLIPSE = 11, /* tf/profiles/mass/nfw.py:100   [Rs,alpha_Rs,e1,e2,center_x,center_y] */
  GL_TNFW = 12,        /* tf/profiles/mass/tnfw.py:12   [Rs,alpha_Rs,r_trunc,center_x,center_y] */
  GL_USER_MASS = 13,   /* profile.py:63-82 as an extension point: a body the user wrote (gl_model_create_user); iparam = parameter
                          count, flags = index of the body */
  GL_INTERPOL_MASS = 14, /* beyond the reference: a lens given as two deflection maps on a grid, interpolated (lenstronomy's
                            INTERPOL_SCALED by name) [scale_factor,center_x,center_y]; maps attached with gl_model_set_lens_maps */
  GL_MULTIPOLE = 15, /* beyond the reference: an m-th order multipole of the potential (lenstronomy's MULTIPOLE by name)
                        [a_m,phi_m,center_x,center_y]; iparam = m, 2 <= m <= 8 (GL_EINVAL otherwise) */
  /* light profiles: LightProfile.light (profile.py:24-60) */
  GL_SERSIC = 16,         /* tf/profiles/light/sersic.py:23-24 [R_sersic,n_sersic,center_x,center_y,Ie] */
  GL_SERSIC_ELLIPSE = 17, /* sersic.py:68-69 [R_sersic,n_sersic,e1,e2,center_x,center_y,Ie] */
  GL_SHAPELETS = 18,      /* tf/profiles/light/shapelets.py:18,34-36 [beta,center_x,center_y,amp0..amp{L-1}] */
  GL_CORE_SERSIC = 19,    /* sersic.py:85-96 [R_sersic,n_sersic,Rb,alpha,gamma,e1,e2,center_x,center_y,Ie] */
  GL_USER_LIGHT = 20,     /* profile.py:24-60 as an extension point: a user-written light body (gl_model_create_user) */
  GL_INTERPOL = 21        /* beyond the reference: a pixelated source image, interpolated (lenstronomy's INTERPOL by name)
                             [center_x,center_y,phi,scale,amp]; flags: GL_FLAG_INTERPOL_LINEAR; image attached with
                             gl_model_set_light_image */
} gl_kind;

#define GL_SHAPELETS_NMAX_CAP 20 /* largest n_max served (231 amplitudes); above 10 the runtime-order path of the interpreter kernel runs */
#define GL_SHAPELETS_TABLE_NODES 6000
#define GL_FLAG_SHAPELETS_INTERPOLATE 1u /* shapelets.py:20 interpolate=True (table mode) */
#define GL_FLAG_INTERPOL_LINEAR 1u /* GL_INTERPOL: bilinear interpolation (order 1) instead of Keys' cubic convolution (order 3) */
#define GL_INTERPOL_MAX_SIDE 2048 /* largest height / width of an interpolated image */

typedef struct gl_component {
  int32_t kind;   /* gl_kind */
  int32_t iparam; /* EPL: niter cap (epl.py:15, default 50); SHAPELETS: n_max; SCALED: number of scales; else 0 */
  uint32_t flags; /* GL_FLAG_* */
  int32_t reserved; /* GL_USER_LIGHT: 1 = the last parameter is the profile's linear amplitude (lstsq_simulate solves for it); else 0 */
} gl_component;

/* Pixel grid and camera set-up == what LensSimulator.__init__ precomputes
 * (tf/simulator.py:14-70).  All pointers are HOST pointers, copied at create. */
typedef struct gl_grid {
  int32_t height;      /* rows of the supersampled image  (wcs.n_x * supersample) */
  int32_t width;       /* cols of the supersampled image  (wcs.n_y * supersample) */
  int32_t supersample; /* simulator.py:27 */
  int32_t n_region;    /* N = number of evaluated pixels (rows of tf.where(region), tf/simulator.py:43) */
  const float* grid_x; /* [N] img_X, f64 arithmetic cast to f32 (simulator.py:52-55) */
  const float* grid_y; /* [N] img_Y */
  const int32_t* pix_index; /* [N] row*width+col of each evaluated pixel, or NULL == full grid in row-major order */
  float conversion_factor;  /* det(transform_pix2angle) of the un-supersampled transform (tf/simulator.py:27-29) */
  const float* psf;    /* [psf_h*psf_w] PSF already sampled on the supersampled grid and NOT flipped, or NULL
                          (tf/simulator.py:62-70 flips it and cross-correlates, i.e. a true convolution) */
  int32_t psf_h, psf_w;
} gl_grid;

typedef struct gl_model gl_model; /* opaque; immutable once set up (create + the gl_model_set_* calls, which are host-side
                                     set-up and must not race with compute calls); then safe to share between host threads */

/* Build the model descriptor for PhysicalModel(lenses, lens_light, source_light)
 * (model.py:24-44, tf/model.py:290-306) on LensSimulator's grid.  `comps` lists the
 * n_lens mass profiles, then n_lens_light, then n_src light profiles. */
int gl_model_create(const gl_component* comps, int n_lens, int n_lens_light, int n_src,
                    const gl_grid* grid, gl_model** out);
void gl_model_destroy(gl_model* m);

int gl_model_num_params(const gl_model* m);    /* P: packed constrained parameters per sample */
int gl_model_param_offset(const gl_model* m, int component); /* column of the component's first parameter */
int64_t gl_model_num_pixels(const gl_model* m); /* N */

/* Bytes of caller-owned scratch the calls below need for a batch of B samples. */
size_t gl_workspace_bytes(const gl_model* m, int B);

/* LensSimulator.simulate (tf/simulator.py:109-156): params [B,P] -> img [B,H,W]
 * (H = height/supersample, W = width/supersample), NaN->0, PSF, average-pool, x conversion_factor. */
int gl_simulate_fwd(const gl_model* m, const float* params, int B, float* img,
                    void* workspace, size_t workspace_bytes, void* hip_stream);

/* Partial renders (forward only): LensSimulator.simulate(no_deflection=True) (tf/simulator.py:125-126),
 * simulate_source (:242-269), simulate_lens_light (:271-297), simulate_images (:299-328).
 * parts is a bit set: 1 = apply the deflection, 2 = lens light, 4 = source light
 * (simulate == 7, no_deflection == 6, simulate_source == 4, simulate_lens_light == 2, simulate_images == 5). */
#define GL_PART_DEFLECT 1u
#define GL_PART_LENS_LIGHT 2u
#define GL_PART_SOURCE_LIGHT 4u
int gl_simulate_parts_fwd(const gl_model* m, const float* params, int B, unsigned parts, float* img,
                          void* workspace, size_t workspace_bytes, void* hip_stream);

/* Vector-Jacobian product of the above (what tf.GradientTape supplies, tf/inference.py:33-39):
 * grad_img [B,H,W] -> grad_params [B,P]. */
int gl_simulate_bwd(const gl_model* m, const float* params, const float* grad_img, int B,
                    float* grad_params, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ForwardProbModel.stats_pixels (tf/model.py:89-101) fused with simulate() and, when
 * grad_params != NULL, with its gradient d loglike / d params [B,P].
 *   obs [H,W]; err_or_null [H,W] (error_map, wins over bg_rms/exp_time, tf/model.py:92-95);
 *   mask_or_null [H,W] (simulator.img_region weights); loglike [B]; chi2 [B] (= chi^2, NOT reduced:
 *   the caller divides by count_nonzero(img_region), tf/model.py:100). */
int gl_loglike_fwd_bwd(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                       const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike,
                       float* chi2, float* grad_params_or_null, void* workspace, size_t workspace_bytes,
                       void* hip_stream);

/* Unconstrained-space front end: ForwardProbModel.log_prob (tf/model.py:126-167) in one launch sequence.
 * Column k of z is the k-th leaf of the prior in tf.nest.flatten order (tf/model.py:76-87); each column
 * carries its default event-space bijector and its scalar prior (TFP semantics restated):
 *   bijector 0 Identity | 1 Exp | 2 Sigmoid(lo,hi);  prior 0 Normal(a,b) | 1 LogNormal(a,b) | 2 Uniform(lo,hi)
 *   | 3 TruncatedNormal(a,b,lo,hi) with log_norm = log(Phi((hi-a)/b) - Phi((lo-a)/b)).
 * const_row [P] supplies the packed columns no z column drives (the *_constants of PhysicalModel). */
typedef struct gl_zcolumn {
  int32_t param_col;
  int32_t bijector;
  int32_t prior;
  float a, b, lo, hi, log_norm;
} gl_zcolumn;
int gl_model_set_prior(gl_model* m, const gl_zcolumn* cols, int d, const float* const_row);

/* z [B,d] -> logprob [B] = loglike + log prior(x) + log|dx/dz|, loglike [B], red_chi2 [B] = chi^2 / chi2_divisor
 * (the caller passes count_nonzero(img_region), tf/model.py:100) and, when grad_z_or_null != NULL,
 * d logprob / d z [B,d] (what tf.GradientTape returns at tf/inference.py:33-39). */
#define GL_TERM_PIXELS 1u    /* include_pixels    (tf/model.py:152-156) */
#define GL_TERM_POSITIONS 2u /* include_positions (tf/model.py:157-161), needs gl_model_set_positions */
int gl_logprob_fwd_bwd(const gl_model* m, const float* z, const float* obs, const float* err_or_null,
                       const float* mask_or_null, float bg_rms, float exp_time, int B, float* logprob,
                       float* loglike, float* red_chi2, float* grad_z_or_null, float chi2_divisor, unsigned terms,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* Image-position likelihood, ForwardProbModel.stats_positions (tf/model.py:103-124) with LensSimulator.beta and
 * .magnification (tf/simulator.py:72-91): observed positions of multiply-imaged sources, grouped in families.
 * x, y, err_x, err_y: concatenation over families (HOST pointers, copied).  loglike [B], chi2 [B] (sum over
 * families, not reduced: the caller divides by n_position = 2 * total images, tf/model.py:74,123) and the
 * gradient w.r.t. the packed parameters [B,P] (zero outside the lens columns). */
int gl_model_set_positions(gl_model* m, int n_families, const int* family_sizes, const float* x, const float* y,
                           const float* err_x, const float* err_y);
int gl_positions_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                         float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Source planes at different redshifts behind the one lens plane (beyond the reference).  A source light or an image family at
 * redshift z_s sees the deflection scaled by  c = [D_LS / D_S](z_s) / [D_LS / D_S](z_ref):  beta = theta - c sum alpha,
 * A = I - c H.  The scales are constants of the model (HOST pointers, copied), each finite and > 0; all 1 (or never set) is the
 * single source plane, served by exactly the kernels and arithmetic of a model without scales.
 *   gl_model_set_source_scales    one scale per source light component (n_src = the model's): every pixel-grid call renders
 *                                 source s at its own beta_s and carries its cotangent into the lens gradients times c_s.  A model
 *                                 with some scale != 1 runs the interpreter kernel (or gl_clusterw_scaled_kernel for N x NFW |
 *                                 N x Sersic models in the gradient modes), never a specialised composition.
 *                                 The launch plan changes with it (chunking as for the interpreter, no tapered dispatch), and
 *                                 with the plan the workspace: size it again with gl_workspace_bytes after this call.
 *                                 GL_EUNSUPPORTED: some scale != 1 on a model with user-written profiles.
 *   gl_model_set_position_scales  one scale per image family of gl_model_set_positions, which must have been called (and which
 *                                 resets the scales to 1): the image-position likelihood and its gradient use c_f of image j's family.
 * GL_EINVAL: a count that does not match, a scale that is not finite or not > 0. */
int gl_model_set_source_scales(gl_model* m, const float* scales, int n_src);
int gl_model_set_position_scales(gl_model* m, const float* scales, int n_families);

/* Flux ratios of the image families (beyond the reference): the second observable of a lensed quasar or supernova.  With beta_j and
 * A_j of the observed images as the position likelihood traces them, m_j = 1 / |det A_j|; an image with a measured flux F_j and error
 * s_j enters with weight w_j = 1 / s_j^2.  The unlensed flux S_f of the family's source is profiled out in closed form:
 *   S_f = sum w F m / sum w m^2 ,  chi2_f = sum w (F - S_f m)^2 ,  ll_f = -1/2 (chi2_f + sum log(2 pi s^2)) ,
 * and, S_f minimising chi2_f, the gradient is the partial derivative at fixed S_f.  Only ratios are constrained: (F, s) -> (c F, c s)
 * leaves chi2_f alone.
 *   gl_model_set_position_fluxes  flux, flux_err [n_images] (HOST pointers, copied) in the concatenated image order of
 *       gl_model_set_positions, which must have been called (and which clears the fluxes); a NaN flux marks an image without a
 *       measurement, flux = NULL (or every flux NaN) clears them.  GL_EINVAL, the model left as it was: n_images that does not
 *       match, a measured flux that is not finite or whose error is not finite and > 0, a family with exactly one measured flux.
 *       While the model holds fluxes, GL_TERM_POSITIONS of gl_logprob_fwd_bwd / gl_multiplane_logprob_fwd_bwd is the sum of both
 *       terms and its reduced chi2 divides by 2 J + n_flux (n_flux: the measured fluxes); gl_positions_fwd_bwd and
 *       gl_multiplane_positions_fwd_bwd keep computing the positions alone, with unchanged bits.
 *   gl_position_fluxes_fwd_bwd    the flux term alone, on one plane (with the scales of gl_model_set_position_scales) or on lens
 *       planes (gl_model_set_position_targets) alike: loglike, chi2 [B] (summed over the families, not reduced), and when given
 *       d loglike / d params [B][P], amplitude [B][n_families] = S_f and model_flux [B][n_images] = S_f m_j (NaN for a family without
 *       fluxes).  Workspace of gl_workspace_bytes(m, B); enqueues on the caller's stream without allocation or synchronisation;
 *       two calls give identical bits.  GL_EINVAL before gl_model_set_positions / gl_model_set_position_fluxes; GL_EUNSUPPORTED
 *       for a GL_SERIES lens, as gl_positions_fwd_bwd. */
int gl_model_set_position_fluxes(gl_model* m, const float* flux, const float* flux_err, int n_images);
int gl_position_fluxes_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2, float* grad_params_or_null,
                               float* amplitude_or_null, float* model_flux_or_null, void* workspace, size_t workspace_bytes,
                               void* hip_stream);

/* Time delays of the image families (beyond the reference): the third observable of a lensed quasar or supernova.  Family f has
 * images theta_j with beta_j as the position likelihood traces them and the source  mean beta  over ALL its images.  An image with a
 * measured arrival time t_j (days, relative to any zero) and error s_j enters with weight w_j = 1 / s_j^2.  With
 *   phi_j = 1/2 |theta_j - mean beta|^2 - psi(theta_j)   (arcsec^2; psi as gl_lens_potential),  phi~, t~: minus their w-weighted means,
 *   lambda_f = the family's given scale, or profiled out:  sum w t~ phi~ / sum w phi~^2 ,
 *   chi2_f = sum w (t~ - lambda_f phi~)^2 ,  ll_f = -1/2 (chi2_f + sum log(2 pi s^2)) ,  T_f = t_bar - lambda_f phi_bar ,
 * the zero T_f of the family's clock is always profiled out: only delay differences are constrained.  T_f, and lambda_f where it is
 * profiled, minimise chi2_f, so the gradient is the partial derivative at fixed (lambda_f, T_f).  lambda_f is D_dt / c in
 * days / arcsec^2: D_dt [Mpc] x 0.0280 (LensSimulator.DAYS_PER_MPC_ARCSEC2).
 *   gl_model_set_position_delays  delay, delay_err [n_images] (HOST pointers, copied) in the concatenated image order of
 *       gl_model_set_positions, which must have been called (and which clears the delays); a NaN time marks an image without a
 *       measurement, delay = NULL (or every time NaN) clears them.  scale_per_family [n_families]: lambda_f, or NaN to profile it.
 *       GL_EINVAL, the model left as it was: counts that do not match, a measured time that is not finite or whose error is not
 *       finite and > 0, a family with exactly one measured time, a family with two measured times and a NaN scale (the fit would be
 *       exact).  GL_EUNSUPPORTED, the model left as it was: lens planes (gl_model_set_lens_planes, which in turn refuses a model that
 *       holds delays), a family with delays whose deflection scale differs from 1 (gl_model_set_position_scales, which in turn
 *       refuses such a scale), a GL_SERIES or GL_USER_MASS lens -- the set gl_lens_potential refuses.  A negative or huge profiled
 *       lambda_f is data, not an error.  The workspace layout does not change.  The checks run in this order: the tables (GL_EINVAL),
 *       then -- only if some time is measured; a table of NaN clears and returns GL_OK like delay = NULL -- planes, scales, lens kinds.
 *       While the model holds delays, GL_TERM_POSITIONS of gl_logprob_fwd_bwd is the sum of the point terms and its reduced chi2
 *       divides by 2 J + n_flux + n_delay (n_delay: the measured times); gl_positions_fwd_bwd and gl_position_fluxes_fwd_bwd keep
 *       their bits.
 *   gl_position_delays_fwd_bwd    the delay term alone: loglike, chi2 [B] (summed over the families, not reduced), and when given
 *       d loglike / d params [B][P], scale [B][n_families] = lambda_f, offset [B][n_families] = T_f and model_delay [B][n_images] =
 *       lambda_f phi_j + T_f in days (NaN for a family without delays).  Workspace of gl_workspace_bytes(m, B); enqueues on the
 *       caller's stream without allocation or synchronisation; no atomics: two calls give identical bits.  GL_EINVAL before
 *       gl_model_set_positions / gl_model_set_position_delays. */
int gl_model_set_position_delays(gl_model* m, const float* delay, const float* delay_err, int n_images, const float* scale_per_family,
                                 int n_families);
int gl_position_delays_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2, float* grad_params_or_null,
                               float* scale_or_null, float* offset_or_null, float* model_delay_or_null, void* workspace,
                               size_t workspace_bytes, void* hip_stream);

/* ... on lens planes (gl_model_set_lens_planes): family f sits behind the planes 0 .. K_f - 1 (the non-zero head of its coupling row,
 * gl_model_set_position_targets), its images are traced as gl_multiplane_positions_fwd_bwd traces them, its source is mean beta, and
 * the Fermat potential is the arrival time of the ray through the planes (gl_multiplane_fermat),
 *   phi_j = sum_{i<K_f} [ geom_f,i |theta_j,i - theta_j,next(i)|^2 / 2 - pot_i psi_i(theta_j,i) ] ,  theta_j,next(K_f - 1) = mean beta ,
 * in arcsec^2 c / H0 with the weights of MultiPlane.delay_weights(z_f).  Everything after phi_j is the term above; lambda_f is in
 * days per (arcsec^2 c / H0): c / H0 [Mpc] x 0.0280, so a profiled lambda_f is the Hubble distance, H0 = c / (lambda_f / 0.0280).
 * The gradient is the partial derivative at fixed (lambda_f, T_f): through mean beta into the beta adjoints of the position
 * likelihood on planes, and a_j d phi_j / d params at fixed mean beta in forward mode through the plane recursion (the ray
 * positions behind the owning lens move with the parameter).
 *   gl_model_set_position_plane_delays  after gl_model_set_positions, gl_model_set_lens_planes and gl_model_set_position_targets,
 *       each of which clears the plane delays, as delay = NULL (or every time NaN) does.  delay, delay_err [n_images] and
 *       scale_per_family [n_families] (lambda_f, NaN: profiled) as gl_model_set_position_delays; geom [n_families][n_planes] and pot
 *       [n_planes] HOST doubles, copied: row f = the geometric weights of MultiPlane.delay_weights(z_f), pot the potential weights of
 *       the planes (those of the farthest family with delays).  GL_EINVAL, the model left as it was: the count, finiteness and
 *       family-size rules of gl_model_set_position_delays; a model without planes or without targets; n_planes other than the
 *       model's; a weight that is not finite or is negative; a geom row whose non-zero head differs from that of the family's
 *       coupling row.  GL_EUNSUPPORTED, the model left as it was: a lens without a potential (the set gl_multiplane_fermat refuses).
 *       The state is apart from that of gl_model_set_position_delays, which keeps refusing a model with planes, as
 *       gl_model_set_lens_planes keeps refusing one that holds single-plane delays.  The workspace GROWS while the model holds plane
 *       delays (by [B][n_images][5] + [B][n_families][2] + [B][n_images] doubles): size it again with gl_workspace_bytes after this
 *       call; every other model keeps its size.  While the model holds plane delays, GL_TERM_POSITIONS of
 *       gl_multiplane_logprob_fwd_bwd includes the term and its reduced chi2 divides by 2 J + n_flux + n_delay;
 *       gl_multiplane_positions_fwd_bwd and gl_position_fluxes_fwd_bwd keep their bits.
 *   gl_multiplane_position_delays_fwd_bwd  the twin of gl_position_delays_fwd_bwd: the term alone, with the same optional outputs
 *       (scale = lambda_f).  GL_EINVAL before gl_model_set_position_plane_delays; GL_EUNSUPPORTED for the gradient with a
 *       GL_MULTIPOLE lens, as the other point terms on planes (values are served).  No atomics: two calls give identical bits. */
int gl_model_set_position_plane_delays(gl_model* m, const float* delay, const float* delay_err, int n_images, const double* geom,
                                       const double* pot, const float* scale_per_family, int n_families, int n_planes);
int gl_multiplane_position_delays_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                                          float* grad_params_or_null, float* scale_or_null, float* offset_or_null,
                                          float* model_delay_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Per-family read-back of the point likelihood (a test and diagnostic aid): copies w_fam [B][n_families][2] = (log_like, chi2) of
 * every (sample, family) -- as the most recent gl_positions_fwd_bwd / gl_multiplane_positions_fwd_bwd / gl_position_fluxes_fwd_bwd /
 * gl_position_delays_fwd_bwd / GL_TERM_POSITIONS call with the same B left it in `workspace` -- to out (DEVICE) on the caller's
 * stream.  One device-to-device copy: no launch, and no store is added to any of those calls.  The per-sample outputs of those
 * calls are the sums of these elements over the families in family order.  GL_EINVAL before gl_model_set_positions. */
int gl_position_family_terms(const gl_model* m, void* workspace, size_t workspace_bytes, int B, float* out, void* hip_stream);

/* ScalingRelation.hessian on arbitrary points (scaling_relation.py:72-83): out [4][n_pts][B] = f_xx, f_xy, f_yx, f_yy
 * summed over the catalogue; other arguments as gl_scaled_eval. */
int gl_scaled_hessian(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev, const float* x,
                      const float* y, int64_t n_pts, int B, int xy_batched, const float* scales, int n_scales,
                      float* out, void* hip_stream);

/* Series-expansion accelerator (MassSeries.set_grid / set_constants / set_deriv, tf/series/series_profile.py:54-62;
 * ScalingRelationSeries.precompute_deriv, scaling_series.py:19-35; DPIESeries.precompute_deriv, dpie_series.py:19-33).
 * gl_series_precompute: Taylor coefficients C_n, n = 0..order, of the population's deflection per unit amplitude in the
 *   cut-radius scale, at arbitrary points: coeffs [2][order+1][n_pts] (x components then y components).  Catalogue
 *   arguments as gl_model_set_catalogue / gl_scaled_eval (table_dev: DEVICE [n_galaxies][7]); scales: HOST [n_scales],
 *   the entry of theta_E is ignored (amplitude 1), the entry of r_cut is the expansion point r0 and must be scaled.
 *   The reference's f_n (n-th derivatives, summed with 1/n!) are n! C_n.
 * gl_model_set_series: attach a field computed on the model's own pixel list ([2][order+1][N], DEVICE; copied) to a
 *   GL_SERIES lens; at run time  alpha = theta_E * sum_n C_n (r_cut - r0)^n  (series_profile.py:76-95).
 * gl_series_eval: that polynomial on a field, out0/out1 [n_pts][B]  (MassSeries.deriv at plugin level).
 * The Hessian half (MassSeries.set_hessian / .hessian, series_profile.py:64-65,83-89; DPIESeries.precompute_hessian,
 * dpie_series.py:35-49; ScalingRelationSeries.precompute_hessian, scaling_series.py:37-54):
 * gl_series_precompute_hessian: same arguments, coeffs [3][order+1][n_pts] = series of f_xx, f_xy, f_yy.
 * gl_series_hessian_eval: out [3][n_pts][B] = theta_E * sum_n C_n (r_cut - r0)^n per field.
 * gl_model_set_series_hessian: attach the Hessian field of a GL_SERIES lens ([3][order+1][N], DEVICE; copied) so that
 *   gl_lens_maps on the model's own grid (x = y = NULL) can include the lens; gl_model_set_series must come first. */
int gl_series_precompute(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev,
                         const float* scales, int n_scales, int order, const float* x_dev, const float* y_dev,
                         int64_t n_pts, float* coeffs_dev, void* hip_stream);
int gl_model_set_series(gl_model* m, int component, float r0, const float* coeffs_dev);
int gl_series_eval(const float* coeffs_dev, int order, int64_t n_pts, int B, const float* theta_E, const float* r_cut,
                   float r0, float* out0, float* out1, void* hip_stream);
int gl_series_precompute_hessian(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev,
                                 const float* scales, int n_scales, int order, const float* x_dev, const float* y_dev,
                                 int64_t n_pts, float* coeffs_dev, void* hip_stream);
int gl_series_hessian_eval(const float* coeffs_dev, int order, int64_t n_pts, int B, const float* theta_E,
                           const float* r_cut, float r0, float* out, void* hip_stream);
int gl_model_set_series_hessian(gl_model* m, int component, const float* coeffs_dev);

/* Linear-amplitude solve, LensSimulator.lstsq_simulate (tf/simulator.py:158-240): every light component is rendered
 * as `depth` basis images of unit amplitude (Sersic: 1; Shapelets: (n_max+1)(n_max+2)/2), NaN -> 0, PSF and
 * pooling per channel, then  coeffs = pinv(X^T X, rcond=1e-6) X^T Y  with X = stack / err_map, Y = obs / err_map.
 *   params   [B,P]; the amplitude columns (gl_model_linear_column) are ignored
 *   parts    GL_PART_DEFLECT | GL_PART_LENS_LIGHT | GL_PART_SOURCE_LIGHT; drop GL_PART_DEFLECT for no_deflection=True
 *   coeffs   [B,D] (return_coeffs) | stacked [B,D,H,W] (return_stacked; the reference's layout is (B,H,W,D)) |
 *   image    [B,H,W] = sum_d coeffs_d stack_d (default return; no det(T) factor, it is absorbed by the coefficients);
 *            any of the three may be NULL.  obs, err: [H,W], required unless only `stacked` is requested.
 * Equivalent forward parameters: amplitude_k = coeffs_k / conversion_factor. */
int gl_model_num_linear(const gl_model* m);            /* D = sum of the light profiles' depth */
int gl_model_linear_column(const gl_model* m, int k);  /* packed-parameter column of linear coefficient k */
size_t gl_lstsq_workspace_bytes(const gl_model* m, int B);
int gl_lstsq_fwd(const gl_model* m, const float* params, const float* obs, const float* err, int B, unsigned parts,
                 float* coeffs_or_null, float* stacked_or_null, float* image_or_null, void* workspace,
                 size_t workspace_bytes, void* hip_stream);
/* Measurement aid: where, inside a workspace of gl_lstsq_workspace_bytes(m, B), the per-sample int32 flags of the most recent
 * solve live: 0 = the Cholesky attempt proved tf.linalg.pinv's rcond cut idle and solved the system (csrc/gl_lstsq.hip.h
 * gl_chol_solve_kernel), 1 = left to the eigenvalue solve.  GL_EUNSUPPORTED for systems the attempt does not serve (> 127). */
int gl_lstsq_solve_flags(const gl_model* m, int B, size_t* offset_bytes);
/* The solve half of gl_lstsq_fwd on a caller's own basis stack -- no gl_model: the normal-matrix kernel, the sum of the chunk
 * partials, the Cholesky attempt and the eigenvalue solve, launched exactly as gl_lstsq_fwd launches them for a model with D linear
 * coefficients on HW pixels (gl_lstsq_fwd runs this function after rendering its stack).
 *   stack [B][D][HW], obs [HW], err [HW]   device pointers; err = +inf masks a pixel (weight 0)
 *   workgroups   target of workgroups in flight of the normal-matrix kernel (gl_lstsq_fwd: 2048): sets the pixels per chunk
 *   cholesky     0 = every system through the eigenvalue solve
 *   coeffs [B][D];  flags_or_null [B] int32 as gl_lstsq_solve_flags (1 everywhere when no attempt ran);
 *   normal_or_null [B][Dp][Dp], Dp = D + 1 rounded up to a multiple of 4: the summed normal matrix of the augmented system
 *   [X | Y] the solve kernels consumed (lower triangle; row D = X^T Y, Y^T Y; columns D + 1 .. Dp - 1 are padding), copied from the
 *   partials after the solve.
 * GL_EUNSUPPORTED: D > 255.  GL_EINVAL: null pointers, non-positive sizes.  GL_ENOMEM: a workspace under
 * gl_lstsq_solve_stack_workspace_bytes (0 for arguments the call refuses).
 * gl_lstsq_last_kernels: the (mangled) symbols of the normal-matrix, Cholesky and eigenvalue kernel of this process's most
 * recent solve through either entry point, an empty string for a stage that did not run; after a gl_lstsq_fwd on its stack-free
 * path the first is the gl_shp_normal_kernel that formed the partials. */
size_t gl_lstsq_solve_stack_workspace_bytes(int B, int D, int HW, int workgroups);
int gl_lstsq_solve_stack(const float* stack, const float* obs, const float* err, int B, int D, int HW, int workgroups,
                         int cholesky, float* coeffs, int* flags_or_null, float* normal_or_null, void* workspace,
                         size_t workspace_bytes, void* hip_stream);
int gl_lstsq_last_kernels(char* normal, char* chol, char* eigen, size_t cap);

/* Galaxy catalogue of a GL_SCALED component (ScalingRelation.__init__, scaling_relation.py:27-55).  Must be attached
 * to every GL_SCALED component before gl_workspace_bytes / any compute call (the workspace holds one block of
 * constants per sample and galaxy).
 *   base_kind  GL_DPIS, GL_DPIE or GL_DPIEP (`profile`)
 *   table      HOST [n_galaxies][7] rows (theta_E, r_core, r_cut, center_x, center_y, e1, e2): for a scaling
 *              parameter the entry is (L_g/L*)^power (`_unscaled_params`, :52-55), otherwise the catalogue constant
 *              (`_galaxy_constants`, :48-51; e1, e2 ignored for GL_DPIS)
 *   scale_col  for theta_E, r_core, r_cut: position of its scale inside the component's parameter row, or -1 when
 *              the quantity is a catalogue constant */
int gl_model_set_catalogue(gl_model* m, int component, int base_kind, int n_galaxies, const int32_t scale_col[3],
                           const float* table);

/* Image of a GL_INTERPOL light component (beyond the reference: every light profile there is parametric).  With
 *   dx = px - center_x, dy = py - center_y,
 *   u = ( dx cos phi + dy sin phi) / scale + (w - 1) / 2      (column coordinate; scale = arcsec per image pixel, > 0)
 *   v = (-dx sin phi + dy cos phi) / scale + (h - 1) / 2      (row coordinate)
 * the component's surface brightness at (px, py) is  amp * sum_j sum_i k(v - j) k(u - i) image[j][i],  the image zero-extended
 * over all integers and k the hat function (GL_FLAG_INTERPOL_LINEAR) or Keys' cubic convolution kernel with a = -1/2: continuous
 * everywhere (C1 for the cubic), zero once u < -2, u > w + 1, v < -2 or v > h + 1 -- a coordinate that is not finite included --
 * with zero gradient there.  No division by scale^2: `amp` scales surface brightness.  The gradient calls differentiate with
 * respect to the five parameters and the evaluation point (so the lens parameters see it), not the pixels.
 *   image  HOST [h][w], copied with a two-pixel zero apron into a device buffer the model owns; one image per component, shared
 *          by the whole batch.  A set-up call like gl_model_set_series: the model is immutable once compute calls have begun.
 * Every GL_INTERPOL component needs its image before gl_workspace_bytes / any compute call (GL_EINVAL otherwise).  A model that
 * holds one runs the interpreter kernel in every mode.  GL_EINVAL: `component` is not a GL_INTERPOL light, h or w outside
 * 1..GL_INTERPOL_MAX_SIDE, a pixel that is not finite.  gl_model_create_user answers GL_EUNSUPPORTED for a model that mixes
 * user-written profiles with GL_INTERPOL (the run-time compiled kernels carry no image tables). */
int gl_model_set_light_image(gl_model* m, int component, int h, int w, const float* image_host);
/* Deflection maps of a GL_INTERPOL_MASS lens (beyond the reference: every lens there is parametric).  With
 *   u = (x - center_x) / pitch + (w - 1) / 2   (column coordinate; pitch = arcsec per map pixel, > 0)
 *   v = (y - center_y) / pitch + (h - 1) / 2   (row coordinate)
 * the lens deflects by  scale_factor * sum_j sum_i k(v - j) k(u - i) alpha_x[j][i]  (alpha_y likewise), the maps zero-extended over
 * all integers and k Keys' cubic convolution kernel with a = -1/2 (no bilinear order, no rotation): C1 everywhere, zero once
 * u < -2, u > w + 1, v < -2 or v > h + 1 -- a coordinate that is not finite included.  The Hessian of the lens is the derivative
 * of this interpolant entry by entry (f_xy and f_yx are not symmetrised); there is no potential: gl_lens_potential, the Fermat
 * potential and the time-delay term answer GL_EUNSUPPORTED, as do gl_model_set_lens_planes and gl_model_create_user beside
 * user-written profiles.  The gradient calls differentiate with respect to the three parameters, not the map pixels.
 *   alpha_x, alpha_y  HOST [h][w] (arcsec), copied with a two-pixel zero apron into a device buffer the model owns; shared by the
 *                     whole batch.  A set-up call like gl_model_set_light_image.
 * Every GL_INTERPOL_MASS lens needs its maps before gl_workspace_bytes / any compute call (GL_EINVAL otherwise).  A model that
 * holds one runs the interpreter kernel in every mode.  GL_EINVAL: `component` is not a GL_INTERPOL_MASS lens, h or w outside
 * 1..GL_INTERPOL_MAX_SIDE, a map value that is not finite, a pitch that is not finite and > 0; a refused call leaves the model
 * as it was. */
int gl_model_set_lens_maps(gl_model* m, int component, int h, int w, const float* alpha_x_host, const float* alpha_y_host, double pitch);
/* MassProfile.deriv (hessian == 0: out0 = alpha_x, out1 = alpha_y, [n_pts][B]) or .hessian (hessian != 0: out0 [4][n_pts][B] =
 * f_xx, f_xy, f_yx, f_yy, out1 unused) of a free-standing GL_INTERPOL_MASS lens on arbitrary points: arguments as gl_profile_eval,
 * params [B,3]; alpha_x_dev / alpha_y_dev: DEVICE [(h+4)][(w+4)], each map with its two-pixel zero apron. */
int gl_interpol_mass_eval(const gl_component* comp, int h, int w, const float* alpha_x_dev, const float* alpha_y_dev, double pitch,
                          const float* x, const float* y, int64_t n_pts, int B, int xy_batched, const float* params, float* out0,
                          float* out1, int hessian, void* hip_stream);
/* LightProfile.light of a free-standing GL_INTERPOL component on arbitrary points: arguments as gl_profile_eval (basis == 0;
 * params [B,5]) or gl_profile_basis (basis != 0: amplitude 1, out [1][n_pts][B]); image_dev: DEVICE [(h+4)][(w+4)], the image
 * with its two-pixel zero apron. */
int gl_interpol_eval(const gl_component* comp, int h, int w, const float* image_dev, const float* x, const float* y,
                     int64_t n_pts, int B, int xy_batched, const float* params, float* out, int basis, void* hip_stream);

/* ScalingRelation.deriv on arbitrary points (scaling_relation.py:61-70); arguments as gl_profile_eval, with
 * table a DEVICE pointer [n_galaxies][7] and scales [B][n_scales]. */
int gl_scaled_eval(int base_kind, int n_galaxies, const int32_t scale_col[3], const float* table_dev, const float* x,
                   const float* y, int64_t n_pts, int B, int xy_batched, const float* scales, int n_scales,
                   float* out0, float* out1, void* hip_stream);

/* LensSimulator.beta / .magnification / .convergence / .shear on arbitrary points (tf/simulator.py:72-107):
 * out [6][n_pts][B] = beta_x, beta_y, f_xx, f_xy, f_yx, f_yy, the Hessian summed over the lenses as `lens.hessian`
 * resolves it in the reference (tf/profile.py:9-43 autodiff; analytic overrides incl. piemd.py:62-83).
 * x, y as in gl_profile_eval ([n_pts,B] when xy_batched, else [n_pts]); params [B,P] (only lens columns are read).
 * x = y = NULL selects the model's own evaluation grid (n_pts must equal its size, xy_batched 0); that is the only
 * form a model with GL_SERIES lenses accepts -- their fields live on that grid (series_profile.py:76-89) -- and it
 * needs gl_model_set_series_hessian on each of them. */
int gl_lens_maps(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts,
                 int xy_batched, float* out, void* hip_stream);

/* The VJP of gl_lens_maps' ray-shoot beta = theta - sum alpha with respect to the lens parameters (beyond the reference, whose
 * tape does this): cot [2][n_pts][B] = the cotangents on beta_x, beta_y (DEVICE), x, y as in gl_lens_maps but never NULL;
 *   grad_params[b][p_off + k] = - sum_pt ( cot_x d alpha_x / d p_k + cot_y d alpha_y / d p_k )    [B][P], DEVICE,
 * columns that belong to no lens written as 0.  A point whose two cotangents are both exactly 0, or one of whose cotangents is not
 * finite, is skipped and its deflection never formed (an SIE at e = 0 or a ray at a centre has NaN derivatives there).  The sum
 * over the points has a fixed order (one partial per workgroup of 64 points in the workspace, then a second pass; no atomics):
 * two calls give identical bits and a sample does not depend on the others.  Served: the built-in mass kinds and GL_SCALED
 * catalogues.  GL_EUNSUPPORTED: GL_SERIES and GL_USER_MASS lenses, models with lens planes.  GL_EINVAL: null arguments, sizes
 * <= 0.  GL_ENOMEM: a workspace under gl_lens_maps_vjp_workspace_bytes(m, B, n_pts) (0 for a null model or sizes <= 0).  No host
 * synchronisation, no allocation. */
size_t gl_lens_maps_vjp_workspace_bytes(const gl_model* m, int B, int64_t n_pts);
int gl_lens_maps_vjp(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts, int xy_batched,
                     const float* cot, float* grad_params, void* workspace, size_t workspace_bytes, void* hip_stream);

/* The VJP of gl_lens_maps' summed Hessian with respect to the lens parameters (beyond the reference): cot [4][n_pts][B] = the
 * cotangents on f_xx, f_xy, f_yx, f_yy (DEVICE), x, y as in gl_lens_maps_vjp;
 *   grad_params[b][p_off + k] = sum_pt ( cot_xx d f_xx / d p_k + cot_xy d f_xy / d p_k + cot_yx d f_yx / d p_k + cot_yy d f_yy / d p_k ),
 * [B][P], DEVICE, columns that belong to no lens written as 0; f includes the dPIS convergence excess on f_xx and f_yy, as
 * gl_lens_maps returns it.  A point whose four cotangents are all exactly 0, or one of whose cotangents is not finite, is skipped
 * and its lens never evaluated.  Sum order, determinism, batch independence, the lenses served, the refusals, the error codes and
 * the workspace size are those of gl_lens_maps_vjp.  No host synchronisation, no allocation. */
size_t gl_lens_hessian_vjp_workspace_bytes(const gl_model* m, int B, int64_t n_pts);
int gl_lens_hessian_vjp(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts, int xy_batched,
                        const float* cot, float* grad_params, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Weak-lensing reduced-shear likelihood of a catalogue of n_gal background galaxies (beyond the reference).  x, y, e1, e2, sigma
 * and scale_or_null: [n_gal], DEVICE -- positions (arcsec), measured ellipticity components, their error per component (> 0) and
 * the deflection scale c of every galaxy's own redshift (NULL: every scale 1).  With f the Hessian of gl_lens_maps,
 *   kappa = c (f_xx + f_yy)/2, gamma1 = c (f_xx - f_yy)/2, gamma2 = c f_xy, g = (gamma1 + i gamma2)/(1 - kappa),
 *   g^ = g where |g|^2 <= 1, g/|g|^2 (= 1/g*) otherwise,
 *   chi2[b] = sum_i [(e1_i - g^1_i)^2 + (e2_i - g^2_i)^2]/sigma_i^2,   ll[b] = -1/2 (chi2[b] + 2 sum_i log(2 pi sigma_i^2)).
 * model_g_or_null [2][n_gal][B] receives g^; grad_params_or_null [B][P] receives d ll / d params through gl_lens_hessian_vjp's
 * kernels (columns of no lens 0).  Every sum has a fixed order: two calls give identical bits and a sample does not depend on the
 * others.  Refusals and error codes as gl_lens_hessian_vjp (GL_EINVAL: a null x, y, e1, e2, sigma, ll, chi2 or workspace, sizes
 * <= 0; GL_ENOMEM: a workspace under gl_shear_loglike_workspace_bytes(m, B, n_gal, want_grad), which is 0 for a null model or
 * sizes <= 0; want_grad = whether grad_params_or_null is given).  No host synchronisation, no allocation. */
size_t gl_shear_loglike_workspace_bytes(const gl_model* m, int B, int n_gal, int want_grad);
int gl_shear_loglike(const gl_model* m, const float* params, int B, const float* x, const float* y, const float* scale_or_null,
                     const float* e1, const float* e2, const float* sigma, int n_gal, float* ll, float* chi2, float* model_g_or_null,
                     float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Image-plane position likelihood of image families with its exact gradient (beyond the reference, whose position term is the
 * source-plane linearisation).  The n_images observed images of the n_families families are concatenated family by family:
 *   image_table  [5][n_images] DEVICE: x, y (arcsec), the isotropic error sigma (> 0), the cap (> 0) and the deflection scale c of
 *                the image's family (beta = theta - c sum alpha, A = I - c H, H the Hessian of gl_lens_maps);
 *   family_table [3][n_images] DEVICE: family, first image and image count of the family of every image;
 *   family_offsets_host [n_families + 1] HOST: the first image of every family, then n_images (read by the call's checks only);
 *   source_or_null [2][B][n_families] DEVICE: the source of every family, x then y; NULL: the barycentre of the family's back-traced
 *                observed images, (1/J_f) sum_k beta(theta_obs_k), which needs two or more images in every family.
 * The predicted image of observed image j is the root of beta(theta) = beta_f that Newton reaches from theta_obs_j (the iteration
 * of gl_image_positions with its polishing step, tol and max_iter as there, every step at most cap_j long).  It is LOST when
 * Newton has not converged, the point is not finite, |theta_pred - theta_obs_j| > cap_j or u_j below is not finite.  With
 * r_j = theta_pred_j - theta_obs_j,
 *   chi2[b] = sum_j min(|r_j|^2, cap_j^2)/sigma_j^2 (a lost image sits at the cap),  ll[b] = -chi2[b]/2 - sum_j log(2 pi sigma_j^2),
 * n_lost[b] the lost images of sample b; pred_or_null [2][n_images][B] receives theta_pred, x then y, NaN where lost.
 * Gradient by the implicit function theorem, u_j = J(theta_pred_j)^-T r_j / sigma_j^2 (0 where lost), J = I - c d alpha / d theta the
 * derivative of the deflection alone (A steers the Newton steps; the dPIS convergence excess in H belongs to no deflection):
 *   d ll / d p = sum_j u_j . d beta / d p at theta_pred_j - (sum_{j in f} u_j) . d beta_f / d p
 * into grad_params_or_null [B][P] through gl_lens_maps_vjp's kernels (columns of no lens 0), and grad_source_or_null
 * [2][B][n_families] = -sum_{j in f} u_j (explicit sources only).  Every sum has a fixed order: two calls give identical bits and a
 * sample does not depend on the others.  Lenses served and refusals as gl_lens_maps_vjp (GL_EUNSUPPORTED: lens planes, series
 * expansions, user-written bodies).  GL_EINVAL: a null table, ll, chi2, n_lost or workspace, sizes <= 0, offsets that do not run
 * from 0 to n_images, an empty family or one of more than 64 images, a one-image family without sources, grad_source without
 * sources, tol <= 0, max_iter < 1.  GL_ENOMEM: a workspace under gl_imgplane_loglike_workspace_bytes(m, B, n_images, with_source,
 * want_grad), which is 0 for a null model or sizes <= 0 (with_source: source_or_null given; want_grad: grad_params_or_null given).
 * All work on the caller's stream; no host synchronisation, no allocation. */
size_t gl_imgplane_loglike_workspace_bytes(const gl_model* m, int B, int n_images, int with_source, int want_grad);
int gl_imgplane_loglike(const gl_model* m, const float* params, int B, const float* image_table, const int32_t* family_table,
                        const int32_t* family_offsets_host, int n_images, int n_families, const float* source_or_null, float tol,
                        int max_iter, float* ll, float* chi2, int32_t* n_lost, float* pred_or_null, float* grad_params_or_null,
                        float* grad_source_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Lens planes at redshifts of their own: multi-plane ray tracing (beyond the reference, which bends every ray at one plane).
 * Planes are numbered 0 .. n_planes - 1 by ascending redshift; every lens keeps its parameters as the reduced deflection for the
 * model's reference plane.  With theta_0 = theta the ray meets plane j at
 *   theta_j = theta - sum_{i<j} C_ij a_i,   a_i = sum_{lenses l on plane i} alpha_l(theta_i),
 * and a target t (a source light, an arbitrary plane) at beta_t = theta - sum_i T_i a_i, with A_t = d beta_t / d theta (not
 * symmetric once two planes are offset).  C_ij = [D_ij / D_j] / [D_i,ref / D_ref]; T_i likewise for the target, 0 for the planes
 * at or behind it.
 *   gl_model_set_lens_planes  HOST arrays, copied to the device: plane_of_lens [n_lens]; lens_scales [n_planes][n_planes] = C,
 *       strictly upper triangular; source_scales [n_planes][n_src], the couplings of every source light component (> 0 on plane 0,
 *       0 from the first plane at or behind the source on).  n_planes in 2 .. 4, every plane holds a lens.  A model just created has
 *       no planes.  From this call on the single-plane entry points (gl_simulate_*, gl_loglike_fwd_bwd, gl_logprob_fwd_bwd,
 *       gl_lstsq_fwd, gl_positions_fwd_bwd, gl_lens_maps, gl_lens_potential, gl_image_positions*, gl_critical_curves*,
 *       gl_pixsrc_reconstruct) answer GL_EUNSUPPORTED for the model -- none of them falls back to one plane -- and the workspace
 *       changes: size it again with gl_workspace_bytes.  GL_EUNSUPPORTED: n_planes > 4, GL_SERIES lenses (their field lives on the
 *       grid theta, not on theta_j), GL_SCALED catalogues, user-written profiles, lights other than Sersic, SersicEllipse and
 *       CoreSersic.  GL_EINVAL: counts that do not match the
 *       model, a plane index out of range, an empty plane, couplings that are not finite or break the rules above.
 *   gl_multiplane_maps        the twin of gl_lens_maps on arbitrary points: x, y [n_pts] or [n_pts][B] (DEVICE), target_scales
 *       [n_planes] (HOST) = T; out [6][n_pts][B] = beta_x, beta_y, f_xx, f_xy, f_yx, f_yy with f = I - A_t.  No workspace.
 *   gl_multiplane_simulate    the twin of gl_simulate_parts_fwd: lens lights at theta, source s at beta_s of its own couplings
 *       (at theta without GL_PART_DEFLECT), NaN -> 0, the model's PSF + pooling launch, x conversion factor; img [B][H][W].
 *   gl_multiplane_loglike     the forward half of gl_loglike_fwd_bwd on that image (materialised in the workspace, then the
 *       image-statistics and finalize launches of the PSF path): loglike, chi2 [B].
 *   gl_multiplane_simulate_bwd     the twin of gl_simulate_bwd (every part): grad_img [B][H][W] -> grad_params [B][P], the VJP
 *       through the plane recursion (csrc/gl_multiplane_bwd.hip.h) of the image gl_multiplane_simulate returns.
 *   gl_multiplane_loglike_fwd_bwd  gl_multiplane_loglike plus, when grad_params_or_null != NULL, d loglike / d params [B][P]:
 *       render -> PSF + pooling -> image statistics with cotangent -> their transposes -> the VJP kernel -> finalize.  loglike and
 *       chi2 are the bits of gl_multiplane_loglike.
 *   gl_multiplane_logprob_fwd_bwd  the twin of gl_logprob_fwd_bwd: z [B][d] in (gl_model_set_prior), logprob, loglike, red_chi2
 *       and, when grad_z_or_null != NULL, d logprob / d z out; bijector and prior fused into the front end and finalize.  terms as
 *       there: GL_TERM_PIXELS, GL_TERM_POSITIONS or both, red_chi2 = (red_pix + red_pos) / n_terms.  GL_EINVAL if terms asks for
 *       GL_TERM_POSITIONS on a model without image positions (gl_model_set_positions) or without the couplings of their families
 *       (gl_model_set_position_targets).
 *   gl_model_set_position_targets  image families at redshifts of their own behind the planes: targets [n_families][n_planes]
 *       (HOST, copied), row f = the couplings T_f of family f (> 0 on plane 0, 0 from the first plane at or behind the family on).
 *       After gl_model_set_positions and gl_model_set_lens_planes, either of which resets the couplings.  GL_EINVAL: counts that do
 *       not match the model, a coupling that is not finite or negative or breaks the rule above, a family whose couplings are all
 *       zero.  gl_model_set_position_scales answers GL_EINVAL on a model with planes: one scale names no plane.
 *   gl_multiplane_positions_fwd_bwd  the twin of gl_positions_fwd_bwd (which keeps refusing planes): every observed image of
 *       family f is traced back with beta = theta - sum_i T_f,i a_i and A = d beta / d theta through the plane recursion
 *       (csrc/gl_multiplane_pos.hip.h), a dPIS lens adding its convergence excess times d theta_j / d theta on its own plane as in
 *       gl_multiplane_maps; the likelihood is that of gl_positions_fwd_bwd.  loglike, chi2 [B] and, when grad_params_or_null != NULL,
 *       d loglike / d params [B][P] (exactly zero in the columns of a lens at or behind every family that could meet it).  GL_EINVAL
 *       before gl_model_set_positions or gl_model_set_position_targets.
 * All enqueue on the caller's stream, without allocation or host synchronisation (a HIP graph may capture them); all but the
 * maps take a workspace of gl_workspace_bytes(m, B).  Deterministic: two calls give identical bits.  GL_EINVAL before
 * gl_model_set_lens_planes. */
int gl_model_set_lens_planes(gl_model* m, const int* plane_of_lens, int n_lens, int n_planes, const float* lens_scales,
                             const float* source_scales, int n_src);
int gl_multiplane_maps(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts, int xy_batched,
                       const float* target_scales, int n_planes, float* out, void* hip_stream);
int gl_multiplane_simulate(const gl_model* m, const float* params, int B, unsigned parts, float* img, void* workspace,
                           size_t workspace_bytes, void* hip_stream);
int gl_multiplane_loglike(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                          const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                          void* workspace, size_t workspace_bytes, void* hip_stream);
int gl_multiplane_simulate_bwd(const gl_model* m, const float* params, const float* grad_img, int B, float* grad_params,
                               void* workspace, size_t workspace_bytes, void* hip_stream);
int gl_multiplane_loglike_fwd_bwd(const gl_model* m, const float* params, const float* obs, const float* err_or_null,
                                  const float* mask_or_null, float bg_rms, float exp_time, int B, float* loglike, float* chi2,
                                  float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);
int gl_multiplane_logprob_fwd_bwd(const gl_model* m, const float* z, const float* obs, const float* err_or_null,
                                  const float* mask_or_null, float bg_rms, float exp_time, int B, float* logprob, float* loglike,
                                  float* red_chi2, float* grad_z_or_null, float chi2_divisor, unsigned terms, void* workspace,
                                  size_t workspace_bytes, void* hip_stream);
int gl_model_set_position_targets(gl_model* m, const float* targets, int n_families, int n_planes);
int gl_multiplane_positions_fwd_bwd(const gl_model* m, const float* params, int B, float* loglike, float* chi2,
                                    float* grad_params_or_null, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Lensing potential psi summed over the model's lenses (beyond the reference, which has none): out [n_pts][B].  Arguments and
 * conventions exactly those of gl_lens_maps, x = y = NULL for the model's own grid included.  psi is the potential whose gradient
 * is this library's deflection (gl_lens_maps' beta = theta - grad psi), reference quirks included; its additive constant is
 * chosen per kind (zero at the lens centre; Shear: zero at the origin) and only differences are physical.  Served: the built-in
 * mass kinds and GL_SCALED catalogues.  GL_EUNSUPPORTED: GL_SERIES lenses (the series stores the deflection only) and
 * GL_USER_MASS lenses (user-written bodies, the run-time compiled ScalingRelation member loops among them: a body defines a
 * deflection only).  No host synchronisation, no allocation. */
int gl_lens_potential(const gl_model* m, const float* params, int B, const float* x, const float* y, int64_t n_pts,
                      int xy_batched, float* out, void* hip_stream);

/* Lens-equation solver (beyond the reference, which maps image plane -> source plane only): the images theta of source
 * positions beta_s, beta(theta) = beta_s, for every sample.  params [B,P] (DEVICE); src_x, src_y [B][n_src] (DEVICE).
 * The window [x_lo, x_hi] x [y_lo, y_hi] is cut into n_cells x n_cells cells, two triangles each; beta is mapped at the vertices
 * (vertices where it is not finite, or that coincide bit for bit with the centre of a GL_SIS lens -- whose deflection is defined as 0
 * there --, are flagged and their triangles skipped); every triangle whose image in the source plane
 * contains beta_s (edge-function sign test, a point on a shared edge counted once) seeds Newton at the preimage of beta_s under
 * the triangle's affine map: theta <- theta + (I - H)^-1 (beta_s - beta(theta)), |step| <= one cell diagonal, until
 * |beta(theta) - beta_s| <= tol (then one polishing step) or max_iter steps.  Converged candidates closer than 0.05 of a cell
 * side are one image.  Outputs (DEVICE):
 *   out [B][n_src][max_images][3] = x, y, signed mu = 1 / det(I - H) (the Hessian as gl_lens_maps has it), images sorted by x
 *       then y, NaN-padded;
 *   n_images [B][n_src] images written;
 *   n_dropped [B][n_src] candidates that did not converge or converged outside the window + triangles that hit beyond the
 *       64 candidates one (sample, source) holds + images beyond max_images (nothing is truncated silently).  A candidate
 *       whose seed misses beta_s by more than a cell side (its triangle straddles a singular lens centre: SIS, SIE, EPL with
 *       gamma >= 2) and does not converge is no image and is not counted.
 * Guaranteed: every image inside the window whose neighbourhood is not folded more finely than one cell.  Not guaranteed: images
 * outside the window, two images closer than about one cell at a fold.  Deterministic (two calls give identical bits; a row does
 * not depend on the other rows).  No host synchronisation, no allocation: workspace of gl_image_positions_workspace_bytes
 * (0 for invalid sizes).  GL_EINVAL: sizes <= 0, n_cells > 8192, max_images outside [1, 64], an empty window, tol <= 0,
 * max_iter < 1; GL_EUNSUPPORTED: GL_SERIES lenses (their field exists on the model grid only).  Models with user-written lenses:
 * the map and Newton kernels are compiled with the point kernels (gl_lens_maps) when first asked for. */
size_t gl_image_positions_workspace_bytes(const gl_model* m, int B, int n_src, int n_cells, int max_images);
int gl_image_positions(const gl_model* m, const float* params, int B, const float* src_x, const float* src_y, int n_src,
                       float x_lo, float x_hi, float y_lo, float y_hi, int n_cells, int max_images, float tol, int max_iter,
                       float* out, int* n_images, int* n_dropped, void* workspace, size_t workspace_bytes, void* hip_stream);
/* ... with one deflection scale per source, src_scale [n_src] (HOST; null = all 1 = gl_image_positions): source s is solved on its
 * own plane, beta_s(theta) = theta - c_s sum alpha(theta), from the one map of the sample (the scan forms beta_s at the vertices,
 * Newton scales deflection and Hessian; mu = 1 / det(I - c_s H)).  The scales are copied on hip_stream into the call's workspace
 * (gl_image_positions_workspace_bytes holds room for them): the call is as re-entrant as gl_image_positions. */
int gl_image_positions_scaled(const gl_model* m, const float* params, int B, const float* src_x, const float* src_y, int n_src,
                              const float* src_scale, float x_lo, float x_hi, float y_lo, float y_hi, int n_cells, int max_images,
                              float tol, int max_iter, float* out, int* n_images, int* n_dropped, void* workspace,
                              size_t workspace_bytes, void* hip_stream);
/* Read-only view of the scan stage, for tests and diagnostics: copies the planes n_cand and n_over [B][n_src] (int32, DEVICE) --
 * triangle hits stored as Newton seeds (at most 64) and hits beyond them -- out of a workspace that gl_image_positions[_scaled] has
 * just filled with the same B, n_src, n_cells, on hip_stream (device-to-device; no host synchronisation).  A source that lies
 * exactly on a shared triangle edge or vertex is one hit; the final outputs cannot show a double claim (Newton merges duplicates).
 * The scan's window is half-open: an image exactly ON the window's boundary is found on two of the four sides only.  A side is
 * walked counter-clockwise around the window (bottom +x, right +y, top -x, left -y) by the one triangle that holds it, and is
 * claimed when that triangle owns the edge under the tie rule: with u that direction and A = I - H the Jacobian of the map there,
 * d = sign(det A) A u has d.y > 0, or d.y == 0 and d.x > 0.  So one of bottom / top and one of left / right is claimed, a corner
 * when both of its sides are; for the identity map: y = y_lo and x = x_hi with the corner (x_hi, y_lo).  An image on an unclaimed
 * side is not seeded and not counted in n_dropped.  Newton's own window test x_lo <= x <= x_hi, y_lo <= y <= y_hi is inclusive.
 * GL_EINVAL: null arguments, sizes out of range; GL_ENOMEM: workspace smaller than gl_image_positions_workspace_bytes;
 * GL_EUNSUPPORTED: a model with lens planes (its workspace holds one map per plane in front of the counts: the entry below).
 * gl_multiplane_image_positions_stage_counts reads the same two planes out of a workspace that gl_multiplane_image_positions has
 * just filled with the same B, n_src, n_cells (the layout of gl_multiplane_image_positions_workspace_bytes, on the model's number
 * of planes); GL_EINVAL also for a model without planes ("gl_model_set_lens_planes has not been called"). */
int gl_image_positions_stage_counts(const gl_model* m, int B, int n_src, int n_cells, const void* workspace,
                                    size_t workspace_bytes, int32_t* n_cand, int32_t* n_over, void* hip_stream);
int gl_multiplane_image_positions_stage_counts(const gl_model* m, int B, int n_src, int n_cells, const void* workspace,
                                               size_t workspace_bytes, int32_t* n_cand, int32_t* n_over, void* hip_stream);
/* The lens-equation solver on lens planes (after gl_model_set_lens_planes; gl_image_positions[_scaled] refuse such a model): source s
 * sits on a plane of its own with the couplings targets [n_src][n_planes] (HOST; row s = MultiPlane.target_scales(z_s): finite,
 * >= 0, 0 from the first lens plane at or behind the source on, not all 0 -- the rules of gl_model_set_position_targets) and is
 * solved for beta_t(theta) = theta - sum_i T_si a_i(theta) = beta_s, the recursion of gl_multiplane_maps.  The plane sums a_i do not
 * depend on the target, so one map of them per sample -- n_planes maps of the single-plane size -- serves every source of the call,
 * whatever its plane.  A vertex is flagged for a plane when a GL_SIS lens of that plane is centred bit for bit on the ray's position
 * ON THAT PLANE, when the ray reaches the plane not finite, or when the plane's sum is not finite; a plane at or behind a source
 * (coupling 0) never flags that source.  Scan, Newton (on the full, non-symmetric Jacobian A_t; the dPIS convergence excess as in
 * gl_multiplane_maps), merge, sort, window, outputs and counters are those of gl_image_positions; mu = 1 / det A_t, the signed
 * magnification on the source's own plane.  The rows are copied on hip_stream into the call's workspace.  Deterministic; no host
 * synchronisation, no allocation: workspace of gl_multiplane_image_positions_workspace_bytes (0 for invalid sizes and for a model
 * without planes) = the single-plane workspace + (n_planes - 1) maps + the coupling rows.  GL_EINVAL: the cases of
 * gl_image_positions, a model without planes ("gl_model_set_lens_planes has not been called"), n_planes that differs from the
 * model's, a bad coupling row.  No gradient. */
size_t gl_multiplane_image_positions_workspace_bytes(const gl_model* m, int B, int n_src, int n_cells, int max_images);
int gl_multiplane_image_positions(const gl_model* m, const float* params, int B, const float* src_x, const float* src_y, int n_src,
                                  const float* targets, int n_planes, float x_lo, float x_hi, float y_lo, float y_hi, int n_cells,
                                  int max_images, float tol, int max_iter, float* out, int32_t* n_images, int32_t* n_dropped,
                                  void* workspace, size_t workspace_bytes, void* hip_stream);
/* Arrival times on lens planes (after gl_model_set_lens_planes; gl_lens_potential keeps refusing such a model: one psi is not
 * defined across planes).  x, y [B][n_src][n_points] (DEVICE; NaN = no point, e.g. the padding of gl_multiplane_image_positions) are
 * image-plane positions theta of rays to the sources src_x, src_y [B][n_src] (DEVICE); out [B][n_src][n_points] (DEVICE, double) is
 *   T = sum_{i < Ks} [ geom_si |theta_i - theta_next(i)|^2 / 2 - pot_i psi_i(theta_i) ]
 * with theta_i the ray's position on plane i (the recursion of gl_multiplane_maps), psi_i the potential of the lenses of plane i
 * there, next(i) the plane behind i or, for the last plane in front of the source, the source itself.  geom [n_src][n_planes] and
 * pot [n_planes] (HOST, double; MultiPlane.delay_weights(z_s)): finite and >= 0; a geom row is 0 from the first plane at or behind
 * its source on and not all 0; pot_i is a constant of plane i (the row delay_weights gives for the farthest source of the call),
 * read for the planes in front of a source alone.  T is in arcsec^2 times the unit of the weights (c / H0 for delay_weights); only differences between
 * rays to ONE source are physical.  Everything is evaluated on double.  A NaN point gives NaN, and so does whatever is not finite
 * on the way (no lens is skipped).  One launch, one thread per (sample, source, point); the rows are copied on hip_stream into the
 * call's workspace of gl_multiplane_fermat_workspace_bytes (0 for n_src <= 0 and for a model without planes).  Deterministic; no
 * host synchronisation, no allocation.  GL_EINVAL: null arguments, sizes <= 0, a model without planes ("gl_model_set_lens_planes
 * has not been called"), n_planes that differs from the model's, a bad weight, a workspace that is too small; GL_EUNSUPPORTED: a
 * lens without a potential (the cases of gl_lens_potential).  No gradient. */
size_t gl_multiplane_fermat_workspace_bytes(const gl_model* m, int n_src);
int gl_multiplane_fermat(const gl_model* m, const float* params, int B, const float* x, const float* y, const float* src_x,
                         const float* src_y, int n_src, int n_points, const double* geom, const double* pot, int n_planes,
                         double* out, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Critical curves and caustics (beyond the reference): the image-plane locus D = det(I - H) = 0 (the Hessian as gl_lens_maps has
 * it) of every sample, contoured by marching squares on n_cells x n_cells cells over the window [x_lo, x_hi] x [y_lo, y_hi], and
 * its image in the source plane.  params [B,P] (DEVICE).  D is mapped at the vertices (one float each; a D that is not finite is
 * flagged, and so is a vertex that coincides bit for bit with the centre of a GL_SIS lens, whose Hessian is defined as 0 there);
 * every grid edge whose two finite endpoint values differ in sign (sign = D < 0) carries one crossing point, bisected ON
 * the edge until the bracket is 4 float32 spacings of the window's largest |coordinate| (at most 32 halvings), so the cells on both
 * sides of an edge see the same bits and segments join exactly.  Every cell yields 0, 1 or 2 segments; in the ambiguous case
 * (diagonal signs equal, neighbours different) the D < 0 corners are joined when the mean of the four vertex values is < 0.
 * Outputs (DEVICE), segments in row-major cell order:
 *   seg  [B][max_segments][2][2]  endpoints (x, y) of each segment, oriented with D < 0 on its left; NaN-padded;
 *   cau  [B][max_segments][2][2]  beta at the same endpoints; NaN-padded;
 *   kind [B][max_segments]        0 tangential (mean of 1 - kappa at the two endpoints > 0), 1 radial, -1 padding;
 *   n_seg [B] segments written; n_dropped [B] segments beyond max_segments (or whose endpoint fell off the list of
 *       2 * max_segments crossing edges: such a slot is padding); n_flagged [B] cells skipped because a vertex is flagged AND
 *       the finite vertices differ in sign (a flagged vertex among equal signs, the centre of an SIS / SIE / EPL, is skipped
 *       silently); open [B] != 0 when a crossing edge lies on the window boundary;
 *   area [B][4]  sum over the written segments of (x1 + x2) / 2 * (y2 - y1): tangential, radial (image plane), tangential,
 *       radial (source plane); the enclosed area when the curves are closed, positive for a loop that encloses D < 0, negative
 *       for one that encloses D > 0; float64 sums in a fixed order.
 * Guaranteed: every endpoint lies on D = 0 to float32 accuracy; between endpoints the curve is a chord of a cell.  Not
 * guaranteed: features narrower than a cell.  Deterministic (two calls give identical bits; a row does not depend on the other
 * rows).  No host synchronisation, no allocation: workspace of gl_critical_curves_workspace_bytes (0 for invalid sizes).
 * GL_EINVAL: sizes <= 0, n_cells > 8192, max_segments outside [1, 2^20], an empty window; GL_EUNSUPPORTED: GL_SERIES lenses (their
 * field exists on the model grid only) and GL_USER_MASS lenses (user-written bodies, the run-time compiled ScalingRelation
 * member loops among them: these kernels are not part of the run-time compiled point program). */
size_t gl_critical_curves_workspace_bytes(const gl_model* m, int B, int n_cells, int max_segments);
int gl_critical_curves(const gl_model* m, const float* params, int B, float x_lo, float x_hi, float y_lo, float y_hi, int n_cells,
                       int max_segments, float* seg, float* cau, int* kind, int* n_seg, int* n_dropped, int* n_flagged, int* open,
                       float* area, void* workspace, size_t workspace_bytes, void* hip_stream);
/* ... of the source plane with deflection scale `scale` (finite, > 0; 1 = gl_critical_curves): D = det(I - scale H), the caustic is
 * beta = theta - scale sum alpha, the curve kind comes from 1 - scale kappa. */
int gl_critical_curves_scaled(const gl_model* m, const float* params, int B, float x_lo, float x_hi, float y_lo, float y_hi,
                              int n_cells, int max_segments, float scale, float* seg, float* cau, int* kind, int* n_seg,
                              int* n_dropped, int* n_flagged, int* open, float* area, void* workspace, size_t workspace_bytes,
                              void* hip_stream);
/* Critical curves and caustics on lens planes (after gl_model_set_lens_planes; gl_critical_curves[_scaled] keep refusing such a
 * model): for every sample and every one of n_src source planes with the couplings targets [n_src][n_planes] (HOST; row s =
 * MultiPlane.target_scales(z_s), the rules of gl_multiplane_image_positions) the locus
 *   D = det A_t = A_xx A_yy - A_xy A_yx = 0,   A_t = d beta_t / d theta,   beta_t = theta - sum_i T_si a_i(theta)
 * of the full, non-symmetric Jacobian (the recursion and the dPIS convergence excess of gl_multiplane_maps), contoured, refined and
 * summed as gl_critical_curves does.  The caustic is beta_t at the refined points; a segment is tangential when the mean of
 * tr A_t / 2 at its endpoints is > 0 (on D = 0 the eigenvalues of A_t are 0 and tr A_t).  One dual ray trace per vertex serves
 * every source of the call.  A vertex is flagged for a source when D is not finite there: a GL_SIS lens centred bit for bit on the
 * ray's position ON ITS PLANE, a ray that reaches a plane not finite, a sum that is not finite -- on the planes in front of that
 * source alone (coupling != 0).  Outputs (DEVICE) [B][n_src][...] in the shapes of gl_critical_curves, every rule of its counters
 * per (sample, source).  The rows are copied on hip_stream into the call's workspace.  Deterministic; no host synchronisation, no
 * allocation: workspace of gl_multiplane_critical_curves_workspace_bytes (0 for invalid sizes and for a model without planes) = the
 * workspace of gl_critical_curves for B n_src samples + the coupling rows.  GL_EINVAL: the cases of gl_critical_curves, n_src <= 0,
 * a model without planes ("gl_model_set_lens_planes has not been called"), n_planes that differs from the model's, a bad coupling
 * row, more than 2^31 - 1 workgroups in a launch; GL_ENOMEM: a workspace that is too small.  No gradient. */
size_t gl_multiplane_critical_curves_workspace_bytes(const gl_model* m, int B, int n_src, int n_cells, int max_segments);
int gl_multiplane_critical_curves(const gl_model* m, const float* params, int B, const float* targets, int n_src, int n_planes,
                                  float x_lo, float x_hi, float y_lo, float y_hi, int n_cells, int max_segments, float* seg, float* cau,
                                  int* kind, int* n_seg, int* n_dropped, int* n_flagged, int* open, float* area, void* workspace,
                                  size_t workspace_bytes, void* hip_stream);

/* Pixelated source reconstruction (beyond the reference): semi-linear inversion (Warren & Dye 2003) with the Bayesian evidence
 * terms of Suyu et al. 2006, for every sample and every regularisation strength.  The source lives on a regular grid of
 * S = ny nx <= 1024 nodes, node (j, i) at (cx + (i - (nx-1)/2) pitch, cy + (j - (ny-1)/2) pitch) -- the pose of a GL_INTERPOL light
 * with phi = 0, scale = pitch, bilinear -- and is zero outside it.  Inputs (DEVICE):
 *   beta_x, beta_y [B][Hs Ws]  source-plane position of every supersampled pixel (gl_lens_maps), row-major on the model's
 *       supersampled frame; a value that is not finite (or is out of the float range test of a GL_INTERPOL light) gives that
 *       pixel a row of exact zeros;
 *   pix [n_used]  indices into the H x W image of the pixels that are fitted, ascending, each in [0, H W) (NOT checked: the
 *       call does not read device memory on the host);  obs, sigma [B][n_used]  data and its rms at those pixels;
 *   lens_light [B][H W] or null: subtracted from obs, added to model_image;
 *   pose [B][3] = pitch, cx, cy;  strength [B][n_strength] = lambda.
 * With L[q, (j,i)] = hat(v_q - j) hat(u_q - i), u = (beta_x - cx) / pitch + (nx-1)/2, v likewise, hat(t) = max(0, 1 - |t|), and
 * F = conversion_factor Pool PSF L (the operator gl_post_apply applies) restricted to the used pixels:
 *   A0 = F^T W F, b = F^T W y, W = diag(1 / sigma^2), y = obs - lens_light;  M = A0 + lambda R;  s = M^-1 b by Cholesky -- no
 *   rcond cut;  R by `regularization`: 0 identity, 1 gradient I (x) T_x + T_y (x) I, 2 curvature I (x) T_x^2 + T_y^2 (x) I with
 *   T_n = tridiag(-1, 2, -1) (the zero extension makes every form positive definite).
 * Outputs (DEVICE): source [B][n_strength][S]; model_image [B][n_strength][H W] = lens_light + F s on the used pixels, lens_light
 * alone elsewhere; scalars [B][n_strength][3] (float64) = chi2 = sum ((y - F s) / sigma)^2, s^T R s, log det M (the sum of the logs
 * of the Cholesky pivots); ok [B][n_strength] = 0 where a pivot is not finite or not positive -- the other outputs of that
 * (sample, strength) are then NaN.  A0 and b are built once per sample and reused for every strength.  Accumulation is float32 in
 * a fixed order (the three scalars: float64): two calls give identical bits, and a (sample, strength) does not depend on the
 * others.  No host synchronisation, no allocation: everything lives in `workspace` (gl_pixsrc_workspace_bytes; 0 for invalid
 * sizes), which is bounded by a chunk of samples and a slice of strengths, not by B or n_strength.
 * GL_EINVAL: null arguments, sizes <= 0, B or n_strength > 65535, n_used > H W, unknown regularization;
 * GL_EUNSUPPORTED: S > 1024.
 * gl_pixsrc_layout (host only: no launch, no allocation) reports how a call of these sizes is cut up: out = samples per chunk,
 * strengths per slice, basis planes per post-processing launch, and n_used rounded up to the tile of the normal matrix.
 * GL_EINVAL where gl_pixsrc_workspace_bytes answers 0. */
size_t gl_pixsrc_workspace_bytes(const gl_model* m, int B, int n_strength, int ny, int nx, int n_used);
int gl_pixsrc_layout(const gl_model* m, int B, int n_strength, int ny, int nx, int n_used, int32_t out[4]);
int gl_pixsrc_reconstruct(const gl_model* m, const float* beta_x, const float* beta_y, int B, const float* obs, const float* sigma,
                          const float* lens_light, const int* pix, int n_used, int ny, int nx, const float* pose, int regularization,
                          const float* strength, int n_strength, float* source, float* model_image, double* scalars, int* ok,
                          void* workspace, size_t workspace_bytes, void* hip_stream);

/* The evidence of gl_pixsrc_reconstruct with its gradient with respect to the rays and the lens-light image.  The arguments of
 * gl_pixsrc_reconstruct with strength [B] (one strength per sample, no scan); source [B][S], model_image [B][H W], scalars [B][3] and
 * ok [B] come from the same kernels and carry exactly the bits gl_pixsrc_reconstruct gives for the same inputs.  With
 * E = -1/2 chi2 - 1/2 lambda s^T R s - 1/2 log det M (the terms of the evidence that depend on the lens), Fw = D P L, rw = yw - Fw s:
 *   dE/dF = D (rw s^T - Fw M^-1),  G = P^T (dE/dF on the H x W image),
 *   grad_beta [2][B][Hs Ws] = dE/dbeta_x, dE/dbeta_y = (1/pitch) sum over the at most four nodes around the ray of G x the hat
 *       product with one factor differentiated (hat'(t) = -sign(t) for 0 < |t| < 1, else 0); exactly 0 for a ray with a row of
 *       zeros (not finite, out of range): the gradient of the evidence with the set of finite rays held fixed,
 *   grad_image [B][H W] = dE/d(lens light image) = rw / sigma on the used pixels, 0 elsewhere.
 * A sample whose ok is 0 has NaN in grad_beta and grad_image.  Kernels (csrc/gl_pixsrc.hip.h): Z = M^-1 Fw by forward and back
 * substitution with the factor the solve left in the workspace (float32, fixed order), the scatter of dE/dF columns to pooled
 * planes (every element written), the model's own transpose of PSF + pooling on a chunk of planes, and a contraction in which one
 * thread owns a supersampled pixel; samples and planes are chunked under the budgets of the forward call.  No atomics: two calls
 * give identical bits, a sample does not depend on the others.  No allocation, no host synchronisation.  Errors as
 * gl_pixsrc_reconstruct.  gl_pixsrc_grad_workspace_bytes: the workspace (0 for sizes the call refuses); gl_pixsrc_grad_layout:
 * out[3] = samples per chunk, planes per post-processing launch, n_pad (host only). */
size_t gl_pixsrc_grad_workspace_bytes(const gl_model* m, int B, int ny, int nx, int n_used);
int gl_pixsrc_grad_layout(const gl_model* m, int B, int ny, int nx, int n_used, int32_t out[3]);
int gl_pixsrc_evidence_grad(const gl_model* m, const float* beta_x, const float* beta_y, int B, const float* obs, const float* sigma,
                            const float* lens_light, const int* pix, int n_used, int ny, int nx, const float* pose, int regularization,
                            const float* strength, float* source, float* model_image, double* scalars, int* ok, float* grad_beta,
                            float* grad_image, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Point images in the pixel likelihood: PSF-rendered images of a lensed point source with linear amplitudes (beyond the reference;
 * csrc/gl_ptimg.hip.h).  x, y, amplitude [B][n_images] (DEVICE; 1 <= n_images <= 8): positions in arcsec and fluxes in image counts.
 * transform (HOST, 6 doubles) = x0, y0, m00, m01, m10, m11 maps a position to supersampled pixel coordinates, u along the columns and
 * v along the rows: (u, v) = M (x - x0, y - y0), the inverse of the camera's pix2angle on the supersampled grid (formed in float64, rounded once).
 * The unit image D(x, y) [H W] on final pixels: Keys' cubic weights (a = -1/2) of the 4 x 4 supersampled nodes around (u, v) on a
 * zero frame, nodes outside the frame dropped; the model's PSF applied as the render applies it (flipped, cross-correlated with
 * SAME padding; [[1]] without one); then the SUM over ss x ss sub-pixels, without the conversion factor.  D is C1 in (x, y), has
 * negative lobes (5e-3 of its peak behind a PSF with sigma = 1.6 nodes, up to 1/9 with none), and is 0 with a zero gradient for a position that is not finite or whose footprint
 * misses the frame.  sum(D) = sum(psf) when the footprint lies inside the frame.
 *   gl_ptimg_render:      image [B][H W] = sum_j amplitude_j D_j
 *   gl_ptimg_render_bwd:  its transpose: grad_image [B][H W] -> grad_amplitude_j = <grad_image, D_j>, grad_x, grad_y [B][n_images]
 *   gl_ptimg_fit:         the amplitudes that maximise the likelihood of observed = extended_image + sum_j a_j D_j:
 *       N_jk = sum w D_j D_k,  r_j = sum w D_j (observed - extended_image),  a = N^-1 r by Cholesky (float64; sums in float64),
 *       weight [H W] (or [B][H W], weight_batched) = 1 / err^2 on the used pixels and 0 elsewhere, observed likewise [H W] or
 *       [B][H W]; amplitude [B][n_images], model_image [B][H W], cotangent_image [B][H W] = weight (observed - model_image) (the
 *       gradient of -chi2 / 2 with respect to extended_image), chi2 [B] (float64), ok [B] = 0 where a pivot is not finite or not
 *       above 1e-6 of its diagonal entry (coincident images, an image on unused pixels alone) -- that sample's other outputs are
 *       then NaN; with want_grad, grad_x, grad_y [B][n_images] = d(-chi2 / 2)/d(x_j, y_j) at the fitted amplitudes (which
 *       maximise it: no term through them).
 * No atomics: two calls give identical bits; a sample does not depend on the others.  No allocation, no host synchronisation.
 * GL_EINVAL (before the model is read): null arguments, n_images outside 1..8, B outside 1..65535; a workspace smaller than
 * gl_ptimg_workspace_bytes (0 for sizes the calls refuse).  GL_EUNSUPPORTED: lens planes, a PSF of more than 12288 nodes with
 * its apron. */
size_t gl_ptimg_workspace_bytes(const gl_model* m, int B, int n_images);
int gl_ptimg_render(const gl_model* m, const float* x, const float* y, const float* amplitude, int B, int n_images,
                    const double* transform, float* image, void* workspace, size_t workspace_bytes, void* hip_stream);
int gl_ptimg_render_bwd(const gl_model* m, const float* x, const float* y, const float* amplitude, int B, int n_images,
                        const double* transform, const float* grad_image, float* grad_x, float* grad_y, float* grad_amplitude,
                        void* workspace, size_t workspace_bytes, void* hip_stream);
int gl_ptimg_fit(const gl_model* m, const float* x, const float* y, int B, int n_images, const double* transform,
                 const float* extended_image, const float* observed, int observed_batched, const float* weight, int weight_batched,
                 int want_grad, float* amplitude, float* model_image, float* cotangent_image, double* chi2, int* ok, float* grad_x,
                 float* grad_y, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Plugin-level point evaluation, the reference's MassProfile.deriv / LightProfile.light called on
 * arbitrary coordinates (tests/test_profiles.py calls exactly these):
 *   x, y [n_pts, B] when xy_batched, else [n_pts] shared by every sample (pixel-major, batch-minor
 *   like the reference, tf/simulator.py:45-51); params [B, n_params(kind)];
 *   out0/out1 [n_pts, B]: (alpha_x, alpha_y) for mass kinds; out0 = light for light kinds (out1 unused). */
int gl_profile_eval(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B,
                    int xy_batched, const float* params, float* out0, float* out1, void* hip_stream);

/* The optimiser update of the MAP / SVI loops (the reference hands the gradient to a Keras / optax Adam,
 * tf/inference.py:33-39; jax/inference.py:62-68) as ONE launch:
 *   g = grad_scale * grad;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   x -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)        (all [n], DEVICE, x / m / v updated in place)
 * t: the 1-based step count from the host; or t_dev (DEVICE, 16 bytes: a double counter holding the number of steps
 * already taken, followed by 8 zero-initialised bytes the library uses) -- the kernel then uses counter + 1 and
 * advances the counter itself, so the call can sit in a captured HIP graph and be replayed. */
int gl_adam_update(float* x, const float* grad, float* m, float* v, int64_t n, float grad_scale, float lr, float beta1,
                   float beta2, float eps, int64_t t, double* t_dev_or_null, void* hip_stream);

/* The Gaussian surrogate of the SVI step (tf/inference.py:64-91: MultivariateNormalTriL over FillScaleTriL(Exp,
 * diag_shift) / MultivariateNormalDiag over Exp; sharded like jax/inference.py:98-128), as the two launches that bracket
 * the forward+gradient call.  l_packed: the row-major lower triangle (d(d+1)/2, full_rank != 0) or the d log-scales.
 * gl_svi_sample: z [n,d] = mu + L eps, eps [n,d] standard normal draws.
 * gl_svi_grad:   buf [1 + d + len(l_packed)] = [ELBO = mean(log q - log p), dELBO/dmu, dELBO/dl_packed] from eps, logp [n]
 *                and grad_z [n,d] = d log p / d z  -- exactly the buffer the one RCCL all-reduce of the step carries. */
int gl_svi_sample(const float* mu, const float* l_packed, int d, int full_rank, const float* eps, int n, float diag_shift,
                  float* z, void* hip_stream);
int gl_svi_grad(const float* l_packed, int d, int full_rank, const float* eps, const float* logp, const float* grad_z, int n,
                float diag_shift, float* buf, void* hip_stream);

/* The leapfrog of the preconditioned HMC loop (tf/inference.py:95-182; momentum precision = the SVI covariance
 * Sigma = L L^T; any d up to 4096 -- cluster models run at d = 132).  All arrays [n,d] row-major DEVICE float32 unless
 * noted.
 * gl_hmc_kick_drift: p_out = p_in + kick * grad;  z_out = z_in + eps * (p_out Sigma)   (may run in place: p_out == p_in,
 *   z_out == z_in).
 * gl_hmc_accept: closes a transition.  p1 = p_new + kick * grad_new; log_acc = (logp_new - |p1 L|^2/2) - (logp - |p0 L|^2/2),
 *   non-finite -> rejected; chain i moves (z, grad, logp overwritten by the proposal) when log(uniforms[i]) < log_acc;
 *   accept_prob [n] = exp(min(log_acc, 0)).  scale_tril: L [d,d] lower triangular. */
int gl_hmc_kick_drift(const float* p_in, const float* grad, float kick, const float* z_in, const float* sigma, float eps, int n,
                      int d, float* p_out, float* z_out, void* hip_stream);
int gl_hmc_accept(float* z, float* grad, float* logp, const float* z_new, const float* grad_new, const float* logp_new,
                  const float* p0, const float* p_new, float kick, const float* scale_tril, const float* uniforms, int n, int d,
                  float* accept_prob, void* hip_stream);

/* LightProfile.light of a `use_lstsq=True` profile (the unit-amplitude basis images: sersic.py:30-34 `Ie = ones`,
 * `ret[tf.newaxis]`; shapelets.py:61-62,71-72): out [depth][n_pts][B], depth = 1 for the Sersic family and
 * (n_max+1)(n_max+2)/2 for Shapelets.  Other arguments as gl_profile_eval; params keeps the kind's full row width,
 * its amplitude columns are not read. */
int gl_profile_basis(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                     const float* params, float* out, void* hip_stream);

/* MassProfile.hessian / convergence / shear at plugin level (tf/profile.py:9-43 and the analytic overrides of
 * nfw.py:77-94, shear.py:18-26, sis.py:19-29, piemd.py:62-83,121-138): out [4][n_pts][B] = f_xx, f_xy, f_yx, f_yy.
 * Free-standing mass kinds only (catalogues and series: gl_lens_maps on a model). */
int gl_profile_hessian(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                       const float* params, float* out, void* hip_stream);

/* MassProfile.potential at plugin level, the twin of gl_profile_hessian: out [n_pts][B] = psi (gl_lens_potential's, one lens).
 * Free-standing built-in mass kinds only; GL_EUNSUPPORTED for GL_SCALED, GL_SERIES and GL_USER_MASS. */
int gl_profile_potential(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                         const float* params, float* out, void* hip_stream);

int gl_kind_num_params(const gl_component* comp); /* length of the reference's params list for this profile */

/* Measurement hooks (bench.py / rocprof cross-check).  gl_model_set_timing(m, slots): slots > 0 allocates a ring of
 * `slots` HIP-event pairs; every subsequent call records one pair on the CALLER'S stream around its dominant ("main")
 * kernel launch -- no host synchronisation, so a sustained loop can be timed launch by launch; slots == 0 turns the
 * hooks off.  gl_model_set_timing_stride(m, k): only every k-th main launch is bracketed (default 1; an event record costs
 * ~2.5 us of stream time, so a sustained loop is sampled rather than slowed).  gl_model_last_main_ms synchronises on the most recent pair and returns its elapsed milliseconds.
 * gl_model_timing_drain synchronises on every pair recorded since the last drain (at most `slots`, oldest first), writes
 * up to `cap` durations to ms[] and their number to *n, and restarts the ring.
 * gl_model_last_main_kernel: the (mangled) symbol of the kernel the most recent main launch dispatched -- the name
 * rocprofv3 lists and tools/isa_flops.py disassembles. */
int gl_model_set_timing(gl_model* m, int slots);
int gl_model_set_timing_stride(gl_model* m, int stride);
int gl_model_last_main_ms(gl_model* m, float* ms);
int gl_model_timing_drain(gl_model* m, float* ms, int cap, int* n);
int gl_model_last_main_kernel(const gl_model* m, char* buf, size_t cap);

/* The model's image post-processing on a caller-supplied stack (csrc/gl_post.hip.h): PSF convolution (SAME, true convolution),
 * average pooling by `supersample` and a scale, or the transpose (adjoint) of that linear map.
 *   transpose == 0: in [B][Hs][Ws] (the supersampled grid of gl_grid) -> out [B][H][W], H = Hs / supersample;
 *   transpose == 1: in [B][H][W] -> out [B][Hs][Ws].
 * `scale` multiplies every output (the simulate path passes the grid's conversion_factor, the basis stack of gl_lstsq_fwd 1).
 * These are the launches gl_simulate_fwd / gl_simulate_bwd / gl_loglike_fwd_bwd make after / before their main kernel, so the
 * call also serves to convolve a caller's own image stack with the model's PSF.  in and out must not overlap.  No workspace, no
 * allocation, no host synchronisation.  GL_EINVAL: a model without PSF and supersampling, null pointers, B <= 0, transpose not
 * 0 or 1; GL_EUNSUPPORTED: a PSF too large for the forward tap kernel's LDS tile.
 * gl_model_last_post_kernel: the (mangled) symbol of the kernel that served the most recent forward (transpose == 0) or
 * transposed (1) post-processing launch on this model, whichever entry point made it -- the twin of gl_model_last_main_kernel. */
int gl_post_apply(const gl_model* m, int B, const float* in, float* out, int transpose, float scale, void* hip_stream);
int gl_model_last_post_kernel(const gl_model* m, int transpose, char* buf, size_t cap);
/* Measurement aid: the work decomposition of a gradient call on B samples and where, inside a workspace of
 * gl_workspace_bytes(m, B), the per-(sample, chunk) partial rows [B][n_chunks][row_floats] live after the call (n_chunks is the
 * number of rows a sample owns: its pixel chunks, or more where the cheapest samples of a launch run as more, shorter
 * workgroups -- rows a sample does not use are zero).  Slots 2 and 3
 * of a row are pads the finalize kernel never reads; the shapelet kernel (csrc/gl_shp.hip.h) leaves there how many of the
 * workgroup's wave-tiles ran the shapelet chains and how many it saw -- what bench.py's instruction model weights the
 * conditional blocks with. */
int gl_model_launch_shape(const gl_model* m, int B, int* chunk_px, int* n_chunks, int* row_floats, size_t* partial_offset_bytes);
/* Measurement aid, host only (nothing is launched): where, inside a workspace of gl_workspace_bytes(m, B), a call on B samples
 * keeps the constrained parameter rows [B][P] (float; written by the z entries, gl_logprob_fwd_bwd), the derived rows [B][D]
 * (float; the front end's output: per-component constants, the EPL coefficient tables), the dispatch order [B] (int) and the
 * per-sample cost [B] (int; the EPL trip count the order sorts on) -- byte offsets from the start of the workspace and element
 * counts.  p_off / d_off: the first column of `component` inside a parameter row / a derived row (component == -1: not asked
 * for, both -1).  GL_EINVAL: null arguments, B outside [1, 65535], component outside [-1, number of components). */
typedef struct gl_workspace_layout {
  size_t params_offset, derived_offset, order_offset, cost_offset;
  size_t params_count, derived_count, order_count, cost_count;
  int P, D;
  int p_off, d_off;
} gl_workspace_layout;
int gl_model_workspace_layout(const gl_model* m, int B, int component, gl_workspace_layout* out);

/* ---- Open plugin boundary: user-written profile bodies (csrc/gl_user.hip) -------------------------------------------------------
 * The reference's extension point is a Python subclass with a TensorFlow body: MassProfile.deriv / LightProfile.light are
 * abstract (src/gigalens/profile.py:58-82).  Here the body is ONE function template in HIP C++ over a number type R,
 *     template <class R> __device__ void deriv(R x, R y, const R* p, R& fx, R& fy);     (mass profile: the deflection)
 *     template <class R> __device__ R    light(R x, R y, const R* p);                   (light profile: surface brightness)
 * with p = the profile's n_params parameters in their declared order.  hiprtc compiles it once for gfx950 with a forward-mode
 * dual number (arithmetic, comparisons, sqrt exp log pow sin cos tan atan atan2 sinh cosh tanh atanh abs fmin fmax resolve by
 * argument-dependent lookup; gl::value(r) gives the plain float of a number for branches).  Compile errors come back verbatim
 * through gl_last_error (GL_EINVAL).  gl_user_profile_check compiles only (no device needed).
 *   eval: x, y [n_pts] or [n_pts,B] (xy_batched), params [B,n_params], out0 (, out1 for mass profiles) [n_pts,B];
 *   jac_or_null [n_out][n_params + 2][n_pts,B]: d out / d (x, y, p_0 .. p_{n-1}) of the same pass (n_out = 2 mass, 1 light).
 * Plugin-level calls only: the pixel kernels of the likelihood path take built-in kinds (gl_model_create). */
/* ... and inside a model: components of kind GL_USER_MASS / GL_USER_LIGHT (iparam = parameter count <= 16, flags = index into
 * `bodies`) make gl_model_create_user compile the interpreter kernel of the likelihood path at run time with those bodies in it:
 * simulate / log-likelihood / fused log-prob and their gradients (forward-mode duals of the body) work as for built-in kinds.
 * The linear-amplitude solve serves them too (round 4: a user-written light with `reserved = 1` contributes one basis image).
 * The image-position likelihood and gl_lens_maps serve them as well (round 4): their kernels are compiled -- when first asked for
 * -- with the mass bodies on the nested duals of the point kernels (Hessians and their parameter derivatives by differentiating
 * `deriv`, as the reference does for every profile, tf/profile.py:9-43).  gl_user_points_check: that compile alone, for one mass
 * body, no device needed. */
int gl_model_create_user(const gl_component* comps, int n_lens, int n_lens_light, int n_src, const gl_grid* grid,
                         const char* const* bodies, int n_bodies, gl_model** out);
/* The compiled interpreter is cached per process, keyed on the program text (bodies, parameter counts, shapelet / family
 * switches): models created with the same bodies -- one LensSimulator per stage and batch size of a modelling sequence -- share
 * one hiprtc compile.  The kernel headers the compile includes are embedded in the library (no source checkout needed).
 * gl_user_model_compile_count: hiprtc compiles of model kernels this process has paid for so far (diagnostics, tests). */
long long gl_user_model_compile_count(void);
int gl_user_points_check(const char* body, int n_params);
typedef struct gl_user_profile gl_user_profile;
int gl_user_profile_check(const char* body, int is_light, int n_params);
int gl_user_profile_create(const char* body, int is_light, int n_params, gl_user_profile** out);
int gl_user_profile_eval(const gl_user_profile* u, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                         const float* params, float* out0, float* out1, float* jac_or_null, void* hip_stream);
void gl_user_profile_destroy(gl_user_profile* u);

const char* gl_last_error(void);
const char* gl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GIGALENS_HIP_H */
