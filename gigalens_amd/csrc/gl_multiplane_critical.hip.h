// gl_multiplane_critical.hip.h -- critical curves and caustics (gl_critical.hip.h) on lens planes (gl_multiplane.hip.h): the locus
//   D = det A_t = A_xx A_yy - A_xy A_yx = 0,    A_t = d beta_t / d theta,    beta_t = theta - sum_i T_i a_i(theta)
// of the NON-symmetric Jacobian on the plane of a source with couplings T_s, for every sample of lens parameters and every source of
// the call (gl_multiplane_critical_curves; LensSimulator.critical_curves / einstein_radius(source_redshifts=...)).  The caustic is
// beta_t at the refined points.  On D = 0 the eigenvalues of A_t are 0 and tr A_t, so the stored "1 - kappa" is tr A_t / 2 and
// gl_crit_cells_kernel's rule (mean of the two endpoints > 0: tangential) holds as it stands.
//
// The plane sums a_i and their Jacobians do not depend on the target: only the last line does.  Rows (b, s) = b S + s take the place
// of the samples of gl_critical.hip.h; its scan and cells kernels index their sample by blockIdx.x alone and read nothing but the
// map of D and the edge records, so they are launched unchanged with B S blocks on a CritArgs laid out [B S][...].  Two new kernels,
// on the caller's stream, no host synchronisation, no allocation:
//   map    (sample, vertex):            ONE dual trace per vertex (mp_trace on Dual<float, 2> with MpLdsSums and MpImgSkip, the dPIS excess
//                                       inside it) serves every source: for each of the S coupling rows the sums are combined and one
//                                       float D goes to dmap[b S + s][v].  A D that is not finite -- a lens singular where the ray
//                                       meets its plane, a ray that does not arrive finite, an infinite sum -- is stored as NaN and
//                                       flags its cells (D counts as not finite wherever beta_t is not: mpcrit_combine).  Only
//                                       planes with T_si != 0 enter: a flagged plane at or behind a source does not flag it.
//   refine (sample, source, list slot): gl_crit_refine_kernel's bisection (bracket rule, CRIT_MAX_BISECT, one record per edge: the
//                                       bracket's midpoint with beta_t and tr A_t / 2 there) on the evaluation of the map kernel
//                                       (mpcrit_trace + mpcrit_combine), so the sign at a vertex and the signs inside the bisection
//                                       come from the same device function.  B S ceil(max_edges / 64) one-wave workgroups.  The
//                                       evaluations inside the loop and the one after it share ONE site: the loop's last trip is
//                                       the evaluation at the final midpoint (the points visited are those of gl_crit_refine_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include "gl_critical.hip.h"
#include "gl_multiplane_images.hip.h"

namespace glk {

struct MpCritArgs {
  const float* tgt;  // [S][K] couplings T_s of every source's plane (0 from the first lens plane at or behind the source on)
  int K, S;          // lens planes of the model; sources of the call
};

// the plane recursion of sample b from (px, py) on Dual<float, 2>: on return the lane's LDS column holds every a_i and d a_i / d theta
__device__ __forceinline__ MpLdsSums mpcrit_trace(const PosArgs& a, const MpArgs& mp, int b, float px, float py) {
  __shared__ float lds[6 * MP_MAXK][MP_MAPS_WG];
  using R = gld::Dual<float, 2>;
  R xd(px), yd(py);
  xd.d[0] = 1.f;
  yd.d[1] = 1.f;
  MpLdsSums sums(&lds[0][threadIdx.x]);
  mp_trace<R, false>(a, mp, b, xd, yd, sums, MpImgSkip());
  return sums;
}

// D = det A_t, beta_t and tr A_t / 2 on the plane with couplings t from the sums of mpcrit_trace at (px, py)
__device__ __forceinline__ float mpcrit_combine(const MpLdsSums& sums, const MpTarget& t, float px, float py, float& bx, float& by,
                                                float& omk) {
  bx = px;
  by = py;
  float h[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k) {
    const float c = t.c[k];
    if (c != 0.f) {  // (a plane at or behind the source: not part of its ray, even where its own sum is not finite)
      bx -= c * sums.at(k, 0); by -= c * sums.at(k, 3);
      h[0] += c * sums.at(k, 1); h[1] += c * sums.at(k, 2); h[2] += c * sums.at(k, 4); h[3] += c * sums.at(k, 5);
    }
  }
  omk = 1.f - 0.5f * (h[0] + h[3]);
  // a skipped lens (MpImgSkip) leaves NaN in the VALUE of its plane sum alone -- its derivative entries stay 0 --, so a ray that
  // meets a singular centre or does not arrive finite shows in beta, not in the determinant: D is not finite where beta is not
  const float d = (1.f - h[0]) * (1.f - h[3]) - h[1] * h[2];
  return isfinite(bx) && isfinite(by) ? d : __builtin_nanf("");
}

// the coupling row of source s, zero-padded to MP_MAXK
__device__ __forceinline__ MpTarget mpcrit_target(const MpCritArgs& q, int s) {
  MpTarget t;
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k) t.c[k] = k < q.K ? q.tgt[(size_t)s * q.K + k] : 0.f;
  return t;
}

__global__ void __launch_bounds__(MP_MAPS_WG) gl_mpcrit_map_kernel(PosArgs a, MpArgs mp, CritArgs g, MpCritArgs q) {
  const int V1 = g.n + 1;
  const long long V = (long long)V1 * V1;
  const long long i = (long long)blockIdx.x * MP_MAPS_WG + threadIdx.x;
  if (i >= V * a.B) return;
  const int b = (int)(i / V), v = (int)(i - (long long)b * V);
  const int r = v / V1, c = v - r * V1;
  const float px = crit_vx(g, c), py = crit_vy(g, r);
  const MpLdsSums sums = mpcrit_trace(a, mp, b, px, py);
  for (int s = 0; s < q.S; ++s) {
    float bx, by, omk;
    float d = mpcrit_combine(sums, mpcrit_target(q, s), px, py, bx, by, omk);
    if (!isfinite(d)) d = __builtin_nanf("");
    g.dmap[((size_t)b * (size_t)q.S + (size_t)s) * (size_t)V + (size_t)v] = d;
  }
}

__global__ void __launch_bounds__(MP_MAPS_WG) gl_mpcrit_refine_kernel(PosArgs a, MpArgs mp, CritArgs g, MpCritArgs q) {
  const int per_row = (g.max_edges + 63) / 64;
  const int row = blockIdx.x / per_row, k = (blockIdx.x - row * per_row) * 64 + threadIdx.x;
  const int b = row / q.S, s = row - b * q.S;
  if (k >= g.n_edges[row]) return;
  const int n = g.n, V1 = n + 1;
  const int e = g.edge_id[(size_t)row * g.max_edges + k];
  int r, c;
  bool hz;
  crit_edge_vertices(n, e, r, c, hz);
  const float x0 = crit_vx(g, c), y0 = crit_vy(g, r);
  const float len = hz ? g.hx : g.hy;
  const bool neg0 = g.dmap[(size_t)row * (size_t)V1 * (size_t)V1 + (size_t)(r * V1 + c)] < 0.f;  // the sign at t = 0; t = 1 has the other
  const MpTarget tg = mpcrit_target(q, s);
  float t_lo = 0.f, t_hi = 1.f, x, y, bx, by, omk;
  for (int it = 0;; ++it) {
    const bool halve = it < CRIT_MAX_BISECT && (t_hi - t_lo) * len > g.bracket;  // false: this trip evaluates the record
    const float t = 0.5f * (t_lo + t_hi);
    x = hz ? x0 + t * len : x0;
    y = hz ? y0 : y0 + t * len;
    const float d = mpcrit_combine(mpcrit_trace(a, mp, b, x, y), tg, x, y, bx, by, omk);
    if (!halve) break;
    if ((d < 0.f) == neg0) t_lo = t;
    else t_hi = t;
  }
  g.edge_pt[(size_t)row * g.max_edges + k] = float4{x, y, bx, by};
  g.edge_omk[(size_t)row * g.max_edges + k] = omk;
}

}  // namespace glk
