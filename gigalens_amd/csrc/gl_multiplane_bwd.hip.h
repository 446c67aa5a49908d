// gl_multiplane_bwd.hip.h -- the VJP of gl_mp_render_kernel (gl_multiplane.hip.h): the gradient of a multi-plane image with
// respect to every parameter, in the accumulator layout of the single-plane gradient kernels, so that gl_finalize_kernel applies the
// chain rule to the raw parameters (and to z) unchanged.
//
// Launch geometry is the main kernels': one 256-thread workgroup per (chunk of the launch plan, sample), the sample's derived rows
// staged in LDS, one row of partials per workgroup in [B][n_chunks][A].  A thread takes one supersampled pixel at a time:
//   1  forward   a_i for every plane (mp_trace's recursion on the derived rows: theta_j = theta - sum_{i<j} C_ij a_i), the lens
//                lights at theta and source s at beta_s = theta - sum_i T_is a_i; a pixel whose value is NaN was written as 0 by the
//                render and passes no cotangent: g = gimg[pix] x out_scale, or 0
//   2  lights    lens-light VJPs at theta; source VJPs at beta_s, whose position cotangent feeds  abar_i -= T_is betabar_s
//   3  planes    mp.order backwards.  When a lens of plane j is reached abar_j is complete (only the sources and the planes behind j
//                feed it).  Its VJP at theta_j with cotangent abar_j gives its accumulators; every centred profile accumulates
//                acc[CX] -= d(g . alpha)/d dx in the sky frame, so the position cotangent is thetabar = -(acc[CX], acc[CY]) of this
//                one call (a Shear has no centre: thetabar = Gamma abar), and  abar_i -= C_ij thetabar  for i < j.  thetabar of
//                plane 0 is dropped: theta is the fixed grid.  (The dPIS convergence excess enters the Jacobian maps only.)
// The per-plane sums a_i and abar_i are sixteen registers touched by unrolled loops with constant indices alone (MpRegSums: the plane
// of a lens selects by comparison) -- nothing of them goes to scratch.  Every component's accumulators are reduced as soon as its
// VJP has run (wave_acc: DPP sums over a lane group, the group's own LDS column), so at most one component's accumulators are live
// beside the sums; the columns are summed in a fixed order at the end.  No float atomics: two calls give the same bits.
// The ray is recomputed from the derived rows (`*_fwd(d, ...)`; an EPL through its coefficient table), where the render runs `*_prep`
// per pixel from the raw rows (lens_point, mp_light): the same formulas, not the same roundings.  The image and the statistics are the
// render's own, but the NaN mask is re-derived here, so a pixel that sits within rounding of a NaN (a ray exactly on a singular
// centre) can receive a cotangent the render zeroed, or the reverse.
// A lens whose cotangent abar_j is exactly zero at a pixel contributes exact zeros and its VJP is masked like a dead pixel's: a plane
// that deflects no source (behind every source, feeding no later plane that does) is ignored by the render, so a position theta_j
// that is not finite there must not reach the accumulators as 0 x NaN.
// XF: models with NFW_ELLIPSE / TNFW lenses or a CoreSersic light -- their VJPs (TNFW's float64 core) would set the register count of
// the kernel every other model runs, so they are compiled into an instantiation of their own.
#pragma once
#include "gl_multiplane.hip.h"

namespace glk {

struct MpBwd {
  const CompDesc* comps;
  int n_lens, n_ll, n_src;
  const float* derived;  // [B][D]
  int D, A, Apad, ncols;
  const float* gx;  // [N] supersampled pixel positions
  const float* gy;
  const int* pix;   // [N] index of a listed pixel in the supersampled frame, or null: the whole frame
  int N, chunk;
  const float* gimg;  // [B][Hs Ws] cotangent of the supersampled image
  long long img_stride;
  float out_scale;
  float* partial;  // [B][n_chunks][A]
};

// deflection of one lens from its derived row (what lens_point computes from the raw row)
template <bool XF>
__device__ __forceinline__ void mp_lens_fwd(int kind, int iparam, const float* d, float x, float y, float& ax, float& ay) {
  ax = 0.f;
  ay = 0.f;
  switch (kind) {
    case K_EPL: epl_fwd<float>(d, x, y, ax, ay); break;
    case K_SIE: sie_fwd<float>(d, x, y, ax, ay); break;
    case K_NFW: nfw_fwd<float>(d, x, y, ax, ay); break;
    case K_SHEAR: shear_fwd<float>(d, x, y, ax, ay); break;
    case K_SIS: sis_fwd<float>(d, x, y, ax, ay); break;
    case K_DPIE: piemd_fwd<float>(d, d + DP_NS, x, y, ax, ay); break;
    case K_DPIS:
    case K_DPIEP: piep_fwd<float>(d, d + DP_NS, x, y, ax, ay); break;
    case K_NFW_ELLIPSE: if constexpr (XF) nfw_ell_fwd<float>(d, x, y, ax, ay); break;
    case K_TNFW: if constexpr (XF) tnfw_fwd<float>(d, x, y, ax, ay); break;
    case K_MULTIPOLE: if constexpr (XF) multipole_fwd<float>(d, iparam, x, y, ax, ay); break;
  }
}

template <bool XF> __device__ __forceinline__ float mp_light_fwd(int kind, const float* d, float x, float y) {
  if (kind == K_CORE_SERSIC) {
    if constexpr (XF) return core_sersic_fwd<float>(d, x, y);
    return 0.f;
  }
  return sersic_fwd<float>(d, x, y);
}

template <int G> __device__ __forceinline__ void mp_zero(float (&acc)[G]) {
#pragma unroll
  for (int k = 0; k < G; ++k) acc[k] = 0.f;
}
// a pixel without cotangent (NaN in the forward image, or past the end of the chunk) contributes exact zeros, whatever its VJP formed
template <int G> __device__ __forceinline__ void mp_mask(float (&acc)[G], bool live) {
#pragma unroll
  for (int k = 0; k < G; ++k) acc[k] = live ? acc[k] : 0.f;
}

// VJP of one light at (x, y) with cotangent g: accumulators reduced into the LDS columns; the position cotangent is ADDED to (gpx, gpy)
template <bool XF>
__device__ __forceinline__ void mp_light_vjp(const CompDesc& cd, const float* d, float x, float y, float g, bool live, const AccCol& ac,
                                             float& gpx, float& gpy) {
  float px = 0.f, py = 0.f;
  if (cd.kind == K_CORE_SERSIC) {
    if constexpr (XF) {
      float acc[CSR_NACC];
      mp_zero(acc);
      (void)core_sersic_vjp<float>(d, x, y, g, acc, px, py);
      mp_mask(acc, live);
      wave_acc<CSR_NACC>(acc, ac, cd.a_off);
    }
  } else {
    float acc[SER_NACC];
    mp_zero(acc);
    (void)sersic_vjp<float>(d, x, y, g, acc, px, py);
    mp_mask(acc, live);
    wave_acc<SER_NACC>(acc, ac, cd.a_off);
  }
  gpx += live ? px : 0.f;
  gpy += live ? py : 0.f;
}

// VJP of one lens at (x, y) with cotangent (gx, gy) of its deflection: accumulators reduced into the LDS columns; returns the
// cotangent of (x, y) in (tbx, tby)
template <bool XF>
__device__ __forceinline__ void mp_lens_vjp(const CompDesc& cd, const float* d, float x, float y, float gx, float gy, bool live,
                                            const AccCol& ac, float& tbx, float& tby) {
  tbx = 0.f;
  tby = 0.f;
#define GL_MP_CENTRED(NACC, CX, CY, CALL)  \
  {                                        \
    float acc[NACC];                       \
    mp_zero(acc);                          \
    CALL;                                  \
    mp_mask(acc, live);                    \
    tbx = -acc[CX];                        \
    tby = -acc[CY];                        \
    wave_acc<NACC>(acc, ac, cd.a_off);     \
  }
  switch (cd.kind) {
    case K_EPL: GL_MP_CENTRED(EPL_NACC, EPLA_CX, EPLA_CY, epl_vjp<float>(d, x, y, gx, gy, acc)) break;
    case K_SIE: GL_MP_CENTRED(SIE_NACC, SIEA_CX, SIEA_CY, sie_vjp<float>(d, x, y, gx, gy, acc)) break;
    case K_NFW: GL_MP_CENTRED(NFW_NACC, NFWA_CX, NFWA_CY, nfw_vjp<float>(d, x, y, gx, gy, acc)) break;
    case K_SIS: GL_MP_CENTRED(SIS_NACC, 0, 1, sis_vjp<float>(d, x, y, gx, gy, acc)) break;
    case K_DPIE: GL_MP_CENTRED(DP_NACC, DPA_CX, DPA_CY, (piemd_vjp<float, true>(d, d + DP_NS, d + DPX_DE, x, y, gx, gy, acc))) break;
    case K_DPIS:
    case K_DPIEP: GL_MP_CENTRED(DP_NACC, DPA_CX, DPA_CY, (piep_vjp<float, true>(d, d + DP_NS, x, y, gx, gy, acc))) break;
    case K_NFW_ELLIPSE:
      if constexpr (XF) GL_MP_CENTRED(NFE_NACC, NFEA_CX, NFEA_CY, nfw_ell_vjp<float>(d, x, y, gx, gy, acc))
      break;
    case K_TNFW:
      if constexpr (XF) GL_MP_CENTRED(TNF_NACC, TNFA_CX, TNFA_CY, tnfw_vjp<float>(d, x, y, gx, gy, acc))
      break;
    case K_MULTIPOLE:
      if constexpr (XF) {
        float ux = 0.f, uy = 0.f;  // (the point's cotangent: GL_MP_CENTRED takes it from the centre sums)
        GL_MP_CENTRED(MPL_NACC, MPLA_CX, MPLA_CY, multipole_vjp<float>(d, cd.iparam, x, y, gx, gy, acc, ux, uy))
      }
      break;
    case K_SHEAR: {  // evaluated at the un-shifted coordinates: alpha = Gamma (x, y), Gamma symmetric
      float acc[SHR_NACC];
      mp_zero(acc);
      shear_vjp<float>(d, x, y, gx, gy, acc);
      mp_mask(acc, live);
      const float g1 = d[SHR_G1], g2 = d[SHR_G2];
      tbx = live ? gx * g1 + gy * g2 : 0.f;
      tby = live ? gx * g2 - gy * g1 : 0.f;
      wave_acc<SHR_NACC>(acc, ac, cd.a_off);
    } break;
  }
#undef GL_MP_CENTRED
}

template <bool XF>
__global__ void __launch_bounds__(MP_WG) gl_mp_bwd_kernel(MpArgs mp, MpBwd r) {
  extern __shared__ float smem[];
  float* s_d = smem;
  float* s_acc = smem + ((r.D + 3) & ~3);
  const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
  {
    const float* src = r.derived + (size_t)b * r.D;
    for (int i = tid; i < r.D; i += MP_WG) s_d[i] = src[i];
    for (int i = tid; i < r.ncols * r.Apad; i += MP_WG) s_acc[i] = 0.f;
  }
  __syncthreads();
  const AccCol ac = acc_col(s_acc, r.Apad, r.ncols, tid);
  const CompDesc* __restrict__ comps = r.comps;
  const float* __restrict__ src_scale = mp.scale + MP_MAXK * MP_MAXK;  // [MP_MAXK][n_src]
  const float* __restrict__ grow = r.gimg + (size_t)b * r.img_stride;
  const int p0 = chunk * r.chunk, p1 = min(p0 + r.chunk, r.N);

  for (int base = p0; base < p1; base += MP_WG) {  // (every thread of the workgroup runs every trip: the reductions are wave-wide)
    const int j = base + tid;
    const bool valid = j < p1;
    const int jj = valid ? j : p1 - 1;
    const float tx = r.gx[jj], ty = r.gy[jj];
    // ---- 1: the forward ray and the pixel's value ----
    MpRegSums a;
    for (int t = 0; t < r.n_lens; ++t) {
      const int l = mp.order[t], pl = mp.plane[l];
      float x = tx, y = ty, ax, ay;
      a.to_plane(pl, mp.scale, x, y);
      mp_lens_fwd<XF>(comps[l].kind, comps[l].iparam, s_d + comps[l].d_off, x, y, ax, ay);
      a.add(pl, ax, ay);
    }
    float v = 0.f;
    for (int i = 0; i < r.n_ll; ++i) {
      const CompDesc cd = comps[r.n_lens + i];
      v += mp_light_fwd<XF>(cd.kind, s_d + cd.d_off, tx, ty);
    }
    for (int s = 0; s < r.n_src; ++s) {
      const CompDesc cd = comps[r.n_lens + r.n_ll + s];
      float bx = tx, by = ty;
#pragma unroll
      for (int k = 0; k < MP_MAXK; ++k) {
        const float c = src_scale[k * r.n_src + s];
        if (c != 0.f) { bx -= c * a.x[k]; by -= c * a.y[k]; }
      }
      v += mp_light_fwd<XF>(cd.kind, s_d + cd.d_off, bx, by);
    }
    const bool live = valid && !isnan_(v);
    const float g = live ? grow[r.pix ? r.pix[jj] : jj] * r.out_scale : 0.f;
    // ---- 2: light VJPs; the sources hand their position cotangent to the planes in front of them ----
    float unused_x = 0.f, unused_y = 0.f;
    for (int i = 0; i < r.n_ll; ++i) {
      const CompDesc cd = comps[r.n_lens + i];
      mp_light_vjp<XF>(cd, s_d + cd.d_off, tx, ty, g, live, ac, unused_x, unused_y);
    }
    MpRegSums abar;
    for (int s = 0; s < r.n_src; ++s) {
      const CompDesc cd = comps[r.n_lens + r.n_ll + s];
      float bx = tx, by = ty;
#pragma unroll
      for (int k = 0; k < MP_MAXK; ++k) {
        const float c = src_scale[k * r.n_src + s];
        if (c != 0.f) { bx -= c * a.x[k]; by -= c * a.y[k]; }
      }
      float gbx = 0.f, gby = 0.f;
      mp_light_vjp<XF>(cd, s_d + cd.d_off, bx, by, g, live, ac, gbx, gby);
#pragma unroll
      for (int k = 0; k < MP_MAXK; ++k) {
        const float c = src_scale[k * r.n_src + s];
        if (c != 0.f) { abar.x[k] -= c * gbx; abar.y[k] -= c * gby; }
      }
    }
    // ---- 3: the planes, backwards ----
    for (int t = r.n_lens - 1; t >= 0; --t) {
      const int l = mp.order[t], pl = mp.plane[l];
      const CompDesc cd = comps[l];
      float x = tx, y = ty, gx = 0.f, gy = 0.f;
      a.to_plane(pl, mp.scale, x, y);
#pragma unroll
      for (int i = 0; i < MP_MAXK; ++i)
        if (i == pl) { gx = abar.x[i]; gy = abar.y[i]; }
      float tbx, tby;
      mp_lens_vjp<XF>(cd, s_d + cd.d_off, x, y, gx, gy, live && (gx != 0.f || gy != 0.f), ac, tbx, tby);
#pragma unroll
      for (int i = 0; i < MP_MAXK - 1; ++i)
        if (i < pl) {
          const float c = mp.scale[i * MP_MAXK + pl];
          abar.x[i] -= c * tbx;
          abar.y[i] -= c * tby;
        }
    }
  }
  __syncthreads();
  float* out = r.partial + ((size_t)b * gridDim.x + chunk) * r.A;
  for (int k = tid; k < r.A; k += MP_WG) {
    float v = 0.f;
    for (int c = 0; c < r.ncols; ++c) v += s_acc[c * r.Apad + k];
    out[k] = v;
  }
}

}  // namespace glk
