// gl_api_plugin.hip -- the entry points that need no model: plugin-level evaluation of one profile, catalogue, series field or
// image table on arbitrary points (gl_point.hip.h), and the update kernels of the inference loops (gl_updates.hip.h).
#include <cmath>
#include <vector>

#include "gl_host_tables.h"
#include "gl_host.hip.h"
#include "gl_point.hip.h"
#include "gl_updates.hip.h"

using namespace glk;

namespace glk {

CompDesc point_comp(const gl_component* comp) {
  CompDesc cd{};
  cd.kind = comp->kind;
  cd.iparam = comp->iparam;
  cd.flags = comp->flags;
  cd.n_par = kind_num_params(comp->kind, comp->iparam);
  if (cd.kind == GL_EPL && cd.iparam <= 0) cd.iparam = 50;
  return cd;
}

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

}  // namespace glk

extern "C" {

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

int gl_profile_eval(const gl_component* comp, const float* x, const float* y, int64_t n_pts, int B, int xy_batched,
                    const float* params, float* out0, float* out1, void* hip_stream) {
  if (!comp || !x || !y || !params || !out0) return fail(GL_EINVAL, "null argument");
  if (n_pts <= 0 || B <= 0) return fail(GL_EINVAL, "n_pts and B must be positive");
  int npar = kind_num_params(comp->kind, comp->iparam);
  if (npar < 0) return fail(GL_EINVAL, "unknown profile kind %d", comp->kind);
  if (comp->kind == GL_SCALED) return fail(GL_EINVAL, "GL_SCALED needs its catalogue: use gl_scaled_eval");
  if (comp->kind == GL_SERIES) return fail(GL_EINVAL, "GL_SERIES needs its coefficient field: use gl_series_eval");
  if (comp->kind == GL_INTERPOL) return fail(GL_EINVAL, "GL_INTERPOL needs its image: use gl_interpol_eval");
  if (comp->kind == GL_INTERPOL_MASS) return fail(GL_EINVAL, "GL_INTERPOL_MASS needs its maps: use gl_interpol_mass_eval");
  const bool mass = comp->kind <= GL_DPIEP || comp->kind == GL_NFW_ELLIPSE || comp->kind == GL_TNFW || comp->kind == GL_MULTIPOLE;
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

}  // extern "C"
