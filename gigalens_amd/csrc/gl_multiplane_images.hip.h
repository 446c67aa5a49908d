// gl_multiplane_images.hip.h -- the lens-equation solver (gl_images.hip.h) on lens planes (gl_multiplane.hip.h): the images theta of
// sources that each sit on a plane of their own behind some of the lens planes, beta_t(theta) = beta_s with
//   beta_t = theta - sum_i T_i a_i(theta),    A_t = d beta_t / d theta   (not symmetric once two planes are offset)
// for every sample of lens parameters (gl_multiplane_image_positions; LensSimulator.image_positions(source_redshifts=...)).
//
// The plane sums a_i(theta) of the recursion do not depend on the target: only the last line does.  So ONE map of the a_i per sample
// serves every source of the call, whatever its redshift -- as one reference-plane map serves every deflection scale in the
// single-plane solver.  Three kernels, all on the caller's stream, no host synchronisation, no allocation:
//   map    (sample, vertex):  the recursion on float (mp_trace<float> on MpRegSums, no catalogue loop); the K plane sums of the vertex go
//                             to pmap[b][k][v] as float2 -- plane-major, so a wave reads consecutive vertices of one plane contiguously.
//                             Plane k of a vertex is NaN when a lens of that plane is singular at the ray's position ON THAT PLANE
//                             (lens_singular_at with theta_k), when the ray does not reach the plane finite (a flagged plane in front
//                             of it), or when the sum is not finite.
//   scan   (sample, source):  gl_img_scan_kernel's walk (img_scan_body) with the vertex value theta - sum_i T_si a_i from the source's own
//                             coupling row; only planes with T_si != 0 enter, so a plane at or behind a source never flags it.  The
//                             value is a function of the vertex alone, formed without contraction: the tie rule of img_tri_hit holds.
//   newton (sample, source):  gl_img_newton_kernel's iteration, merge, sort and counters (img_newton_core); the evaluation is mp_trace on
//                             Dual<float, 2> with MpLdsSums, combined with the source's couplings into beta and f = I - A_t (the dPIS
//                             convergence excess enters inside mp_trace, as in gl_mp_maps_kernel); mu = 1 / det A_t.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_images.hip.h"
#include "gl_multiplane.hip.h"

namespace glk {

struct MpImgArgs {
  const float* tgt;  // [S][K] couplings T_s of every source's plane (0 from the first lens plane at or behind the source on)
  int K;             // lens planes of the model
  float2* pmap;      // [B][K][(n+1)^2] plane sums a_k at the vertices (row-major as ImgArgs::map); NaN = flagged
};

// mp_trace's skip of the solver: a lens that is singular where the ray meets its plane, and a ray that is not finite there (a flagged
// plane in front of it; no lens template is ever evaluated at such a position)
struct MpImgSkip {
  __device__ __forceinline__ bool operator()(const CompDesc& cd, const float* p, float x, float y) const {
    return lens_singular_at(cd, p, x, y) || !(isfinite(x) && isfinite(y));
  }
};

__global__ void __launch_bounds__(256) gl_mpimg_map_kernel(PosArgs a, MpArgs mp, ImgArgs g, MpImgArgs q) {
  const int V1 = g.n + 1;
  const long long V = (long long)V1 * V1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= V * a.B) return;
  const int b = (int)(i / V), v = (int)(i - (long long)b * V);
  const int r = v / V1, c = v - r * V1;
  const float x = img_vx(g, c), y = img_vy(g, r);
  MpRegSums sums;
  mp_trace<float, false>(a, mp, b, x, y, sums, MpImgSkip());
  float2* o = q.pmap + (size_t)b * (size_t)q.K * (size_t)V + v;
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k)
    if (k < q.K) {
      float ax = sums.x[k], ay = sums.y[k];
      if (!(isfinite(ax) && isfinite(ay))) ax = ay = __builtin_nanf("");
      o[(size_t)k * (size_t)V] = float2{ax, ay};
    }
}

// the plane sums of one sample on the plane of a source with couplings t, as the scan reads them: vertex -> beta_t.  A function of the
// vertex alone, without contraction (img_vertex_beta of the single-plane scan)
struct MpImgVertex {
  const ImgArgs& g;
  const float2* pm;  // [K][V] of the sample
  long long V;
  MpTarget t;
  __device__ __forceinline__ float2 operator()(int v) const {
#pragma clang fp contract(off)
    const int V1 = g.n + 1, r = v / V1, col = v - r * V1;
    float bx = img_vx(g, col), by = img_vy(g, r);
#pragma unroll
    for (int k = 0; k < MP_MAXK; ++k) {
      const float c = t.c[k];
      if (c != 0.f) {  // (a plane at or behind the source: not part of its ray, even where it is flagged)
        const float2 ak = pm[(size_t)k * (size_t)V + v];
        bx = bx - c * ak.x;
        by = by - c * ak.y;
      }
    }
    return float2{bx, by};
  }
};

// the coupling row of source s, zero-padded to MP_MAXK
__device__ __forceinline__ MpTarget mpimg_target(const MpImgArgs& q, int s) {
  MpTarget t;
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k) t.c[k] = k < q.K ? q.tgt[(size_t)s * q.K + k] : 0.f;
  return t;
}

__global__ void __launch_bounds__(IMG_SCAN_WG) gl_mpimg_scan_kernel(ImgArgs g, MpImgArgs q) {
  const int bs = blockIdx.x, b = bs / g.S;
  const long long V1 = g.n + 1, V = V1 * V1;
  img_scan_body(g, bs, MpImgVertex{g, q.pmap + (size_t)b * (size_t)q.K * (size_t)V, V, mpimg_target(q, bs - b * g.S)});
}

// The evaluation of the Newton kernel at one point of sample b: beta_t and f = I - A_t (f_xx, f_xy, f_yx, f_yy) on the plane of the
// couplings t.  The 6 MP_MAXK running sums of each lane live in the lane's own column of LDS (MpLdsSums; the workgroup is one wave of
// MP_MAPS_WG lanes), so the two places img_newton_core evaluates at share one column and the Newton state stays in registers.
// Inlined at both: as ONE function call (img_lens_eval_im's device) the callee saves 52 callee-saved vector registers to the private
// segment and restores them on every call -- 104 scratch instructions, 212 B a lane, one wave per SIMD -- where the two inlined
// copies fit 241 registers without a private segment ("Lens-equation solver on lens planes").
struct MpImgEval {
  const PosArgs& a;
  const MpArgs& mp;
  MpTarget t;
  int b;
  __device__ __forceinline__ void operator()(float px, float py, float& bx, float& by, float* h) const {
    __shared__ float lds[6 * MP_MAXK][MP_MAPS_WG];
    using R = gld::Dual<float, 2>;
    R xd(px), yd(py);
    xd.d[0] = 1.f;
    yd.d[1] = 1.f;
    MpLdsSums sums(&lds[0][threadIdx.x]);
    mp_trace<R, false>(a, mp, b, xd, yd, sums, MpImgSkip());
    bx = px;
    by = py;
    h[0] = h[1] = h[2] = h[3] = 0.f;
#pragma unroll
    for (int k = 0; k < MP_MAXK; ++k) {
      const float c = t.c[k];
      if (c != 0.f) {  // (a plane at or behind the source: not part of its ray, even where its own sum is not finite)
        bx -= c * sums.at(k, 0); by -= c * sums.at(k, 3);
        h[0] += c * sums.at(k, 1); h[1] += c * sums.at(k, 2); h[2] += c * sums.at(k, 4); h[3] += c * sums.at(k, 5);
      }
    }
  }
};

__global__ void __launch_bounds__(MP_MAPS_WG) gl_mpimg_newton_kernel(PosArgs a, MpArgs mp, ImgArgs g, MpImgArgs q) {
  const int bs = blockIdx.x, b = bs / g.S;
  img_newton_core(g, MpImgEval{a, mp, mpimg_target(q, bs - b * g.S), b});
}

}  // namespace glk
