// gl_point.hip.h -- plugin-level evaluation of one profile, one catalogue or one series field on arbitrary points
// (MassProfile.deriv / LightProfile.light).  Included by gl_api_plugin.hip alone, which launches them.
#pragma once
#include "gl_kernels.hip.h"

namespace glk {

// ---- plugin-level point evaluation (MassProfile.deriv / LightProfile.light on arbitrary points) ----
__global__ void __launch_bounds__(256) gl_point_kernel(CompDesc cd, const float* __restrict__ x,
                                                       const float* __restrict__ y, long long n_pts, int B,
                                                       int xy_batched, const float* __restrict__ params,
                                                       float* __restrict__ out0, float* __restrict__ out1,
                                                       const float* __restrict__ shp_tab, int shp_stride, InterpDev itab) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pts * B) return;
  const PointAt at(i, B, xy_batched, x, y);
  const float* p = params + (size_t)at.b * cd.n_par;
  float o0 = 0.f, o1 = 0.f;
  switch (cd.kind) {
    case K_EPL: epl_point<float>(p, cd.iparam, at.x, at.y, o0, o1); break;
    case K_SIE: { float d[SIE_ND + 1]; sie_prep<float>(p, d); sie_fwd(d, at.x, at.y, o0, o1); } break;
    case K_NFW: { float d[NFW_ND]; nfw_prep<float>(p, d); nfw_fwd(d, at.x, at.y, o0, o1); } break;
    case K_SHEAR: { float d[4]; shear_prep<float>(p, d); shear_fwd(d, at.x, at.y, o0, o1); } break;
    case K_SIS: { float d[4]; sis_prep<float>(p, d); sis_fwd(d, at.x, at.y, o0, o1); } break;
    case K_DPIS: case K_DPIE: case K_DPIEP: { float d[DPX_ND]; dpie_prep<float>(cd.kind, p, d); dpie_fwd<float>(cd.kind, d, at.x, at.y, o0, o1); } break;
    case K_NFW_ELLIPSE: { float d[NFE_ND]; nfw_ell_prep<float>(p, d); nfw_ell_fwd<float>(d, at.x, at.y, o0, o1); } break;
    case K_TNFW: { float d[TNF_ND]; tnfw_prep<float>(p, d); tnfw_fwd<float>(d, at.x, at.y, o0, o1); } break;
    case K_MULTIPOLE: { float d[MPL_ND]; multipole_prep<float>(p, cd.iparam, d); multipole_fwd<float>(d, cd.iparam, at.x, at.y, o0, o1); } break;
    case K_CORE_SERSIC: { float d[CSR_ND]; core_sersic_prep<float>(p, d); o0 = core_sersic_fwd<float>(d, at.x, at.y); } break;
    case K_INTERPOL: { float d[INT_ND]; interp_prep<float>(p, itab.h, itab.w, d); o0 = interp_fwd<float>(d, itab, cd.flags & 1u, at.x, at.y); } break;
    case K_SERSIC: { float d[SER_NDX]; sersic_prep<float>(p, false, d); o0 = sersic_fwd(d, at.x, at.y); } break;
    case K_SERSIC_ELLIPSE: { float d[SER_NDX]; sersic_prep<float>(p, true, d); o0 = sersic_fwd(d, at.x, at.y); } break;
    case K_SHAPELETS: {
      if (cd.iparam > SH_CAP) {  // runtime-order path; amplitudes straight from the parameter row (same triangle order)
        float d[SHP_AMP];
        d[SHP_CX] = p[1]; d[SHP_CY] = p[2]; d[SHP_IB] = 1.f / p[0]; d[SHP_NMAX] = (float)cd.iparam;
        o0 = shapelets_fwd_amp<float, SH_CAPB>(d, p + 3, shp_tab, shp_stride, cd.flags & 1u, at.x, at.y);
      } else {
        float d[SHP_SQ + SH_SQ * SH_SQ];
        shapelets_prep<float>(p, cd.iparam, d);
        o0 = shapelets_fwd<float, SH_CAP>(d, shp_tab, shp_stride, cd.flags & 1u, at.x, at.y);
      }
    } break;
  }
  out0[i] = o0;
  if (out1) out1[i] = o1;
}

// LightProfile.light of a use_lstsq profile at plugin level: the unit-amplitude basis images (sersic.py:30-34
// `Ie = ones`, `ret[tf.newaxis]`; shapelets.py:61-62,71-72), out[depth][n_pts][B]; amplitude columns are not read
__global__ void __launch_bounds__(256) gl_basis_point_kernel(CompDesc cd, const float* __restrict__ x,
                                                             const float* __restrict__ y, long long n_pts, int B,
                                                             int xy_batched, const float* __restrict__ params,
                                                             float* __restrict__ out,
                                                             const float* __restrict__ shp_tab, int shp_stride, InterpDev itab) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = n_pts * B;
  if (i >= total) return;
  const PointAt at(i, B, xy_batched, x, y);
  const float* p = params + (size_t)at.b * cd.n_par;
  if (cd.kind == K_SHAPELETS) {
    float d[SHP_AMP];
    d[SHP_CX] = p[1];
    d[SHP_CY] = p[2];
    d[SHP_IB] = 1.f / p[0];
    d[SHP_NMAX] = (float)cd.iparam;
    if (cd.iparam > SH_CAP)
      shapelets_basis<float, SH_CAPB>(d, shp_tab, shp_stride, cd.flags & 1u, at.x, at.y,
                                      [&](int k, float v) { out[(size_t)k * total + i] = v; });
    else
      shapelets_basis<float, SH_CAP>(d, shp_tab, shp_stride, cd.flags & 1u, at.x, at.y,
                                     [&](int k, float v) { out[(size_t)k * total + i] = v; });
    return;
  }
  float q[10];
  for (int k = 0; k < cd.n_par; ++k) q[k] = p[k];
  q[kind_linear_col(cd.kind, cd.iparam)] = 1.f;
  float v = 0.f;
  switch (cd.kind) {
    case K_CORE_SERSIC: { float d[CSR_ND]; core_sersic_prep<float>(q, d); v = core_sersic_fwd<float>(d, at.x, at.y); } break;
    case K_INTERPOL: { float d[INT_ND]; interp_prep<float>(q, itab.h, itab.w, d); v = interp_fwd_unit<float>(d, itab, cd.flags & 1u, at.x, at.y); } break;
    case K_SERSIC: { float d[SER_NDX]; sersic_prep<float>(q, false, d); v = sersic_fwd(d, at.x, at.y); } break;
    case K_SERSIC_ELLIPSE: { float d[SER_NDX]; sersic_prep<float>(q, true, d); v = sersic_fwd(d, at.x, at.y); } break;
  }
  out[i] = v;
}

// ScalingRelation.deriv on arbitrary points (scaling_relation.py:61-70)
__global__ void __launch_bounds__(256) gl_scaled_point_kernel(ScaledDesc sd, const float* __restrict__ table,
                                                              const float* __restrict__ x, const float* __restrict__ y,
                                                              long long n_pts, int B, int xy_batched,
                                                              const float* __restrict__ scales, int n_scales,
                                                              float* __restrict__ out0, float* __restrict__ out1) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pts * B) return;
  const PointAt at(i, B, xy_batched, x, y);
  const float* sc = scales + (size_t)at.b * n_scales;
  float sx = 0.f, sy = 0.f;
  for (int g = 0; g < sd.n_gal; ++g) {
    float ds[DP_NS], dd[DP_ND], ax, ay;
    scaled_static<float>(sd.base_kind, table + (size_t)7 * g, ds);
    scaled_dyn<float>(sd, table + (size_t)7 * g, sc, dd);
    if (sd.base_kind == K_DPIE) piemd_fwd<float>(ds, dd, at.x, at.y, ax, ay);
    else piep_fwd<float>(ds, dd, at.x, at.y, ax, ay);
    sx += ax;
    sy += ay;
  }
  out0[i] = sx;
  out1[i] = sy;
}

// Taylor coefficients of the population deflection at arbitrary points: coeffs[2][order+1][n_pts]
template <int N>
__global__ void __launch_bounds__(64) gl_series_precompute_kernel(ScaledDesc sd, const float* __restrict__ table,
                                                                 float s0, float s1, float s2, int order,
                                                                 const float* __restrict__ x, const float* __restrict__ y,
                                                                 long long n_pts, float* __restrict__ coeffs) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_pts) return;
  // float64 jets: near a member's foci (removable 0/0 of the Kassiola-Kovner form) the k-th coefficient loses
  // ~(1/distance)^k digits -- in fp32 orders >= 2 are noise at ~1 % of the pixels; the one-off precompute can afford
  // CDNA4's full-rate fp64, the stored field is fp32 like every other operand of the path
  const double scales[3] = {(double)s0, (double)s1, (double)s2};
  double cx[N + 1], cy[N + 1];
  series_point<N, double>(sd, table, scales, (double)x[i], (double)y[i], cx, cy);
  for (int n = 0; n <= order; ++n) {
    coeffs[(size_t)n * n_pts + i] = (float)cx[n];
    coeffs[(size_t)(order + 1 + n) * n_pts + i] = (float)cy[n];
  }
}

// Taylor coefficients of the population Hessian: coeffs[3][order+1][n_pts] = f_xx, f_xy, f_yy (one-off, fp64 jets)
template <int N>
__global__ void __launch_bounds__(64) gl_series_hessian_precompute_kernel(ScaledDesc sd, const float* __restrict__ table,
                                                                         float s0, float s1, float s2, int order,
                                                                         const float* __restrict__ x,
                                                                         const float* __restrict__ y, long long n_pts,
                                                                         float* __restrict__ coeffs) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_pts) return;
  const double scales[3] = {(double)s0, (double)s1, (double)s2};
  double hxx[N + 1], hxy[N + 1], hyy[N + 1];
  series_point_hessian<N, double>(sd, table, scales, (double)x[i], (double)y[i], hxx, hxy, hyy);
  for (int n = 0; n <= order; ++n) {
    coeffs[(size_t)n * n_pts + i] = (float)hxx[n];
    coeffs[(size_t)(order + 1 + n) * n_pts + i] = (float)hxy[n];
    coeffs[(size_t)(2 * (order + 1) + n) * n_pts + i] = (float)hyy[n];
  }
}

// theta_E[b] * sum_n coeffs[f][n][pt] (r_cut[b] - r0)^n for n_fields fields: out[n_fields][n_pts][B]
__global__ void __launch_bounds__(256) gl_series_fields_kernel(const float* __restrict__ coeffs, int n_fields, int order,
                                                               long long n_pts, int B,
                                                               const float* __restrict__ theta_E,
                                                               const float* __restrict__ r_cut, float r0,
                                                               float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pts * B) return;
  const long long pt = i / B;
  const int b = (int)(i - pt * B);
  const float dl = r_cut[b] - r0, te = theta_E[b];
  for (int f = 0; f < n_fields; ++f) {
    const float* c = coeffs + (size_t)f * (order + 1) * n_pts + pt;
    float v = c[(size_t)order * n_pts];
    for (int n = order - 1; n >= 0; --n) v = v * dl + c[(size_t)n * n_pts];
    out[(size_t)f * n_pts * B + i] = te * v;
  }
}

__global__ void __launch_bounds__(256) gl_series_eval_kernel(const float* __restrict__ coeffs, int order, long long n_pts,
                                                             int B, const float* __restrict__ theta_E,
                                                             const float* __restrict__ r_cut, float r0,
                                                             float* __restrict__ out0, float* __restrict__ out1) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pts * B) return;
  const long long pt = i / B;
  const int b = (int)(i - pt * B);
  const float dl = r_cut[b] - r0;
  float ax = coeffs[(size_t)order * n_pts + pt], ay = coeffs[(size_t)(2 * order + 1) * n_pts + pt];
  for (int n = order - 1; n >= 0; --n) {
    ax = ax * dl + coeffs[(size_t)n * n_pts + pt];
    ay = ay * dl + coeffs[(size_t)(order + 1 + n) * n_pts + pt];
  }
  out0[i] = theta_E[b] * ax;
  out1[i] = theta_E[b] * ay;
}

}  // namespace glk
