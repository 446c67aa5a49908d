// gl_hessian_vjp.hip.h -- the VJP of the summed Hessian of gl_lens_maps on arbitrary points, and the weak-lensing reduced-shear
// likelihood built on it (both beyond the reference, whose tape would do the former).
//
// Hessian VJP: given the cotangents (cot_xx, cot_xy, cot_yx, cot_yy) on f_xx, f_xy, f_yx, f_yy at every (point, sample),
//   grad[b][p_off + k] = sum_pt ( cot_xx d f_xx / d p_k + cot_xy d f_xy / d p_k + cot_yx d f_yx / d p_k + cot_yy d f_yy / d p_k ) ,
// f the Hessian as gl_lens_maps resolves it: the derivative of the deflection plus the dPIS convergence excess on f_xx and f_yy
// (lens_kappa_excess).  The mixed derivatives come from lens_point on Dual<Dual<float,1>,2> with ONE seeded parameter direction,
// as in gl_pos_p3_kernel: a lens is evaluated once per column.
//   H1  (sample, lens column, block of VJP_PTS points): one wave, a point per lane, the shuffle tree of vjp_wave_sum, one partial
//   H2  gl_lens_vjp_sum_kernel, unchanged
// A point whose four cotangents are all exactly 0, or one of which is not finite, is skipped before its lens is evaluated (the
// rule and the reason of gl_lens_vjp.hip.h: 0 x NaN must not reach the sum).
//
// Reduced shear of a catalogue of galaxies (x, y, e1, e2, sigma, scale c), with the conventions of LensSimulator.convergence / .shear:
//   kappa = c (f_xx + f_yy)/2 , gamma1 = c (f_xx - f_yy)/2 , gamma2 = c f_xy , g = (gamma1 + i gamma2)/(1 - kappa) ,
//   g^ = g where |g|^2 <= 1 , 1/g* = g/|g|^2 otherwise ,
//   chi2 = sum [(e1 - g^1)^2 + (e2 - g^2)^2]/sigma^2 ,  log_like = -1/2 (chi2 + 2 sum log(2 pi sigma^2)) .
//   S1  (sample, block of 64 galaxies): Hessian on Dual<float,2> as P1, g^, the block's partial of chi2 and of the norm; the
//       cotangents d log_like / d f_.. in the point layout of the lens maps when a gradient is wanted
//   S2  (sample): one wave adds the partials, lane-strided then the tree
// followed by H1 and H2 on the cotangents.  No atomics and no LDS of their own (the EPL template keeps its table there): every
// sum has a fixed order, two calls give identical bits and a sample reads nothing of another one.
// Included by gl_api_points.hip alone (not part of the run-time compile of user-written point kernels).
#pragma once
#include "gl_lens_vjp.hip.h"

namespace glk {

// grid: ((sample * lens_params + column) * n_blocks + block) workgroups; cot [4][n_pts][B]
__global__ void __launch_bounds__(VJP_WG) gl_hessian_vjp_kernel(PosArgs a, const float* __restrict__ x, const float* __restrict__ y,
                                                               long long n_pts, int xy_batched, const float* __restrict__ cot,
                                                               int lens_params, int n_blocks, float* __restrict__ partial) {
  const int blk = blockIdx.x % n_blocks, bc = blockIdx.x / n_blocks;
  const int col = bc % lens_params, b = bc / lens_params;
  using R1 = gld::Dual<float, 1>;
  using R = gld::Dual<R1, 2>;
  R p[POS_MAXP];
  R1 p1[POS_MAXP];
  const CompDesc cd = lens_seeded_column(a, b, col, p1, p);
  const long long st = n_pts * a.B, pt = (long long)blk * VJP_PTS + threadIdx.x;
  float acc = 0.f;
  if (pt < n_pts) {
    const long long i = pt * a.B + b;
    const float cxx = cot[i], cxy = cot[st + i], cyx = cot[2 * st + i], cyy = cot[3 * st + i];
    const bool zero = cxx == 0.f && cxy == 0.f && cyx == 0.f && cyy == 0.f;
    const bool finite = __builtin_isfinite(cxx) && __builtin_isfinite(cxy) && __builtin_isfinite(cyx) && __builtin_isfinite(cyy);
    if (!zero && finite) {
      const PointAt at(pt, b, i, xy_batched, x, y);
      R xd{R1(at.x)}, yd{R1(at.y)};
      xd.d[0] = R1(1.f);
      yd.d[1] = R1(1.f);
      R ax, ay;
      lens_point<R>(a, cd, p, xd, yd, ax, ay);
      const R1 ex = lens_kappa_excess<R1>(a, cd, p1, at.x, at.y);
      acc = cxx * (ax.d[0].d[0] + ex.d[0]) + cxy * ax.d[1].d[0] + cyx * ay.d[0].d[0] + cyy * (ay.d[1].d[0] + ex.d[0]);
    }
  }
  acc = vjp_wave_sum(acc);
  if (threadIdx.x == 0) partial[(size_t)bc * n_blocks + blk] = acc;
}

// the tables of a shear catalogue, [n_gal] each (kernel arguments of their own: PosArgs keeps its layout)
struct ShearArgs {
  const float* x;
  const float* y;
  const float* scale;  // or null: every scale 1
  const float* e1;
  const float* e2;
  const float* sigma;
  int n_gal, n_blocks;
  float* part;     // [B][n_blocks][2]  chi2, norm of every block
  float* model_g;  // [2][n_gal][B] or null
  float* cot;      // [4][n_gal][B] or null: no gradient wanted
};

// f_xx, f_xy, f_yy of gl_lens_maps_kernel at one point: the lens loop on Dual<float,2> with the dPIS excess.  Not inlined: the
// likelihood's own arithmetic and its nine table pointers stay out of the register budget of the largest lens template
__device__ __noinline__ float3 shear_hessian(const PosArgs& a, int b, float px, float py) {
  float fxx = 0.f, fxy = 0.f, fyy = 0.f;
  lens_jets(a, b, px, py, [&](const CompDesc&, const float*, const Jet2& ax, const Jet2& ay, float ex) {
    fxx += ax.d[0] + ex; fxy += ax.d[1]; fyy += ay.d[1] + ex;
  });
  return make_float3(fxx, fxy, fyy);
}

// grid: (sample * n_blocks + block) workgroups of one wave, a galaxy per lane
__global__ void __launch_bounds__(VJP_WG) gl_shear_fwd_kernel(PosArgs a, ShearArgs s) {
  const int blk = blockIdx.x % s.n_blocks, b = blockIdx.x / s.n_blocks;
  const int j = blk * VJP_PTS + threadIdx.x;
  float chi2 = 0.f, norm = 0.f;
  if (j < s.n_gal) {
    const float3 f = shear_hessian(a, b, s.x[j], s.y[j]);
    const float fxx = f.x, fxy = f.y, fyy = f.z;
    const float c = s.scale ? s.scale[j] : 1.f;
    const float kappa = c * (0.5f * (fxx + fyy)), g1 = c * (0.5f * (fxx - fyy)), g2 = c * fxy;
    const float omk = 1.f - kappa;
    const float r1 = g1 / omk, r2 = g2 / omk, n2 = r1 * r1 + r2 * r2;
    const bool weak = n2 <= 1.f;
    const float h1 = weak ? r1 : r1 / n2, h2 = weak ? r2 : r2 / n2;
    const float sg = s.sigma[j], w = 1.f / (sg * sg);
    const float d1 = s.e1[j] - h1, d2 = s.e2[j] - h2;
    chi2 = (d1 * d1 + d2 * d2) * w;
    norm = 2.f * logf(6.283185307179586f * sg * sg);
    const long long i = (long long)j * a.B + b, st = (long long)s.n_gal * a.B;
    if (s.model_g) { s.model_g[i] = h1; s.model_g[st + i] = h2; }
    if (s.cot) {
      // a = d ll / d g^ = (e - g^)/sigma^2 ; through the active branch to (kappa, gamma1, gamma2):
      //   |g| <= 1:  g^ = gamma/(1 - kappa)            d ll/d gamma = a/(1 - kappa) ,                      d ll/d kappa =  (a . g^)/(1 - kappa)
      //   |g| >  1:  g^ = gamma (1 - kappa)/|gamma|^2  d ll/d gamma = (a - 2 (a . u) u)(1 - kappa)/|gamma|^2 , d ll/d kappa = -(a . g^)/(1 - kappa)
      // with u = gamma/|gamma|
      const float a1 = d1 * w, a2 = d2 * w, adg = (a1 * h1 + a2 * h2) / omk;
      float dk, dg1, dg2;
      if (weak) {
        dk = adg;
        dg1 = a1 / omk;
        dg2 = a2 / omk;
      } else {
        const float gg = g1 * g1 + g2 * g2, t = 2.f * (a1 * g1 + a2 * g2) / gg, f = omk / gg;
        dk = -adg;
        dg1 = (a1 - t * g1) * f;
        dg2 = (a2 - t * g2) * f;
      }
      s.cot[i] = c * (0.5f * (dk + dg1));
      s.cot[st + i] = c * dg2;
      s.cot[2 * st + i] = 0.f;
      s.cot[3 * st + i] = c * (0.5f * (dk - dg1));
    }
  }
  chi2 = vjp_wave_sum(chi2);
  norm = vjp_wave_sum(norm);
  if (threadIdx.x == 0) {
    float* o = s.part + ((size_t)b * s.n_blocks + blk) * 2;
    o[0] = chi2;
    o[1] = norm;
  }
}

// grid: B workgroups of one wave
__global__ void __launch_bounds__(VJP_WG) gl_shear_sum_kernel(const float* __restrict__ part, int n_blocks, float* __restrict__ ll,
                                                             float* __restrict__ chi2) {
  const float* row = part + (size_t)blockIdx.x * n_blocks * 2;
  float c = 0.f, n = 0.f;
  for (int j = threadIdx.x; j < n_blocks; j += VJP_WG) { c += row[2 * j]; n += row[2 * j + 1]; }
  c = vjp_wave_sum(c);
  n = vjp_wave_sum(n);
  if (threadIdx.x == 0) {
    ll[blockIdx.x] = -0.5f * (c + n);
    chi2[blockIdx.x] = c;
  }
}

}  // namespace glk
