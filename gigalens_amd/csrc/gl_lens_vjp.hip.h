// gl_lens_vjp.hip.h -- the VJP of the ray-shoot beta = theta - sum alpha (LensSimulator.beta, tf/simulator.py:72-78) on arbitrary
// points: given a cotangent (cot_x, cot_y) on beta at every (point, sample), the gradient on the lens parameters
//   grad[b][p_off + k] = - sum_pt ( cot_x d alpha_x / d p_k + cot_y d alpha_y / d p_k ) .
// The derivative comes from the generic lens_point<R> of gl_positions.hip.h on forward-mode duals that carry ONE parameter
// direction (Dual<float,1>, as gl_pos_p3_kernel does with its nested ones): a lens is evaluated once per column, which keeps
// every profile -- the EPL series loop above all -- far inside the register file.  Two launches:
//   V1  (sample, lens column, block of VJP_PTS points): one wave, a point per lane; the 64 lanes are added by a shuffle tree and
//       lane 0 writes the block's partial
//   V2  (sample, column): one wave adds the partials of its column, lane-strided then the same tree; columns of no lens get 0
// No atomics: the order of every sum is fixed by the launch shape, so two calls give identical bits, and a sample reads nothing of
// another one.  A point whose two cotangents are both exactly 0, or one of which is not finite, is skipped before its deflection is
// formed: an SIE at e = 0 or a ray at a centre has NaN derivatives, and 0 x NaN must not reach the sum.
// Included by gl_api_points.hip alone (not part of the run-time compile of user-written point kernels).
#pragma once
#include "gl_positions.hip.h"

namespace glk {

constexpr int VJP_WG = 64;        // one wave per workgroup
constexpr int VJP_PTS = VJP_WG;   // points per workgroup: one per lane

// sum over the 64 lanes of a wave in a fixed tree order; the total is lane 0's
__device__ inline float vjp_wave_sum(float v) {
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// grid: ((sample * lens_params + column) * n_blocks + block) workgroups
__global__ void __launch_bounds__(VJP_WG) gl_lens_vjp_kernel(PosArgs a, const float* __restrict__ x, const float* __restrict__ y,
                                                            long long n_pts, int xy_batched, const float* __restrict__ cot,
                                                            int lens_params, int n_blocks, float* __restrict__ partial) {
  const int blk = blockIdx.x % n_blocks, bc = blockIdx.x / n_blocks;
  const int col = bc % lens_params, b = bc / lens_params;
  using R = gld::Dual<float, 1>;
  R p[POS_MAXP];
  const CompDesc cd = lens_seeded_column(a, b, col, p);
  const long long st = n_pts * a.B, pt = (long long)blk * VJP_PTS + threadIdx.x;
  float acc = 0.f;
  if (pt < n_pts) {
    const long long i = pt * a.B + b;
    const float cx = cot[i], cy = cot[st + i];
    if (!((cx == 0.f && cy == 0.f) || !__builtin_isfinite(cx) || !__builtin_isfinite(cy))) {
      const PointAt at(pt, b, i, xy_batched, x, y);
      R ax, ay;
      lens_point<R>(a, cd, p, R(at.x), R(at.y), ax, ay);
      acc = -(cx * ax.d[0] + cy * ay.d[0]);
    }
  }
  acc = vjp_wave_sum(acc);
  if (threadIdx.x == 0) partial[(size_t)bc * n_blocks + blk] = acc;
}

// grid: B * P workgroups, one per element of grad_params [B][P]
__global__ void __launch_bounds__(VJP_WG) gl_lens_vjp_sum_kernel(const float* __restrict__ partial, int P, int lens_params, int n_blocks,
                                                                float* __restrict__ grad) {
  const int b = blockIdx.x / P, p = blockIdx.x - b * P;
  float v = 0.f;
  if (p < lens_params) {
    const float* row = partial + ((size_t)b * lens_params + p) * n_blocks;
    for (int j = threadIdx.x; j < n_blocks; j += VJP_WG) v += row[j];
  }
  v = vjp_wave_sum(v);
  if (threadIdx.x == 0) grad[blockIdx.x] = v;
}

}  // namespace glk
