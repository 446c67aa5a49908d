// gl_pixsrc.hip.h -- pixelated source reconstruction (semi-linear inversion, Warren & Dye 2003) with the Bayesian evidence of
// Suyu et al. 2006 for every sample of lens parameters (gl_pixsrc_reconstruct; LensSimulator.reconstruct_source).  The reference
// has no such call.  The ray-shot source-plane positions beta [B][Hs Ws] come from gl_lens_maps; everything below is linear algebra
// on the source grid of S = ny nx nodes (node (j, i) at (cx + (i - (nx-1)/2) pitch, cy + (j - (ny-1)/2) pitch), the pose of an
// Interpolated light with phi = 0, scale = pitch, order 1):
//   L[q, (j,i)] = hat(v_q - j) hat(u_q - i),  u = (beta_x - cx) / pitch + (nx-1)/2, v likewise, hat(t) = max(0, 1 - |t|); a beta that
//                 is not finite or fails the range test of gl_interp.h gives a row of exact zeros
//   F = scale Pool PSF L restricted to the n_used used pixels;  Fw = diag(1/sigma) F;  yw = (obs - lens light) / sigma
//   A0 = Fw^T Fw,  b = Fw^T yw,  M = A0 + lambda R,  s = M^-1 b by Cholesky (no rcond cut);  log det M from the pivots
// Launches per chunk of samples, all on the caller's stream, no host synchronisation, no allocation:
//   planes   (plane, subpixel):  column (b, s) of L as a supersampled basis plane.  Every element of a plane is WRITTEN (one hat
//                                product, mostly zero) -- no atomics, nothing to clear.  The model's own PSF + pooling launch
//                                (post_fwd, the kernels gl_post_apply runs) then turns a chunk of planes into columns of F: the
//                                operator is bit for bit the one simulate() applies, and every sum has a fixed order.  (The other
//                                way, one output pixel's row accumulated in LDS with atomics over its PSF footprint, adds floats in
//                                the order the lanes arrive: two calls would differ in the last bits.)
//   gather   (plane, used pixel): Fw[b][s][n] = plane[pix[n]] / sigma[b][n], rows padded with zeros to a multiple of PIX_TK
//   rhs_prep (b, used pixel):     yw
//   normal   (b, tile):           the lower-triangle 32 x 32 tiles of A0 = Fw Fw^T, LDS-tiled FMA; per k-tile of 32 a local sum,
//                                 added to the running one (two-level, fixed order); mirrored on the way out
//   rhs      (b, s):              b = Fw yw, one wave per row, lanes stride the pixels, fixed butterfly
//   solve    (b, strength):       one workgroup: M = A0 + lambda R (stencil) in the workspace, blocked right-looking Cholesky in
//                                 place (32-column panels: diagonal block in LDS, panel by forward substitution per row, trailing
//                                 update in 32 x 32 tiles staged through LDS), log det M = sum log(pivot) in float64, the ok flag,
//                                 forward and back substitution blocked the same way, then one step of iterative refinement
//                                 on the float64 residual b - M s
//   combine  (b, strength):       (F s)[n] = sigma sum_s Fw[s][n] s_s, the model image, chi2 = sum (yw - Fw s)^2 and s^T R s by the
//                                 stencil, all summed in float64 in a fixed order
#pragma once
#include <hip/hip_runtime.h>

namespace glk {

constexpr int PIX_MAX_S = 1024;  // source nodes served
constexpr int PIX_TK = 32;       // tile edge of the normal-matrix and Cholesky kernels; rows of Fw are padded to a multiple of it
constexpr int PIX_WG = 256;
constexpr int PIX_REG_IDENTITY = 0, PIX_REG_GRADIENT = 1, PIX_REG_CURVATURE = 2;

struct PixArgs {
  int B, L;            // samples of this chunk, strengths of this slice
  int ny, nx, S;       // source grid
  int HsWs, HW;        // supersampled and pooled pixels of one plane
  int n_used, n_pad;   // used pixels; n_used rounded up to a multiple of PIX_TK
  int reg;             // PIX_REG_*
  int L_total;         // row length of strength / of the outputs' strength axis
  const float* beta_x;  // [B][HsWs]
  const float* beta_y;
  const float* pose;   // [B][3] pitch, cx, cy
  const int* pix;      // [n_used] index of a used pixel in the pooled image
  const float* sigma;  // [B][n_used]
  const float* obs;    // [B][n_used]
  const float* lens_light;  // [B][HW] or null
  const float* strength;    // [B][L_total], offset to this slice's first column
  float* Fw;           // [B][S][n_pad]
  float* yw;           // [B][n_pad]
  float* A0;           // [B][S][S]
  float* bvec;         // [B][S]
  float* M;            // [B][L][S][S]
  float* source;       // [B][L_total][S], offset to this slice's first column
  float* model;        // [B][L_total][HW]
  double* scal;        // [B][L_total][3] chi2, s^T R s, log det M
  int* ok;             // [B][L_total]
};

__device__ inline float pix_hat(float t) { return fmaxf(0.f, 1.f - fabsf(t)); }

// planes p0 .. p0 + gridDim.y - 1 of the chunk's flat (sample, node) list -> out[plane][q] = out_scale * L[q, node]
__global__ void __launch_bounds__(PIX_WG) gl_pix_planes_kernel(PixArgs a, int p0, float out_scale, float* __restrict__ out) {
  const int q = blockIdx.x * PIX_WG + threadIdx.x;
  if (q >= a.HsWs) return;
  const int p = p0 + blockIdx.y, b = p / a.S, s = p - b * a.S;
  const int j = s / a.nx, i = s - j * a.nx;
  const float pitch = a.pose[3 * b], cx = a.pose[3 * b + 1], cy = a.pose[3 * b + 2];
  const float u = (a.beta_x[(size_t)b * a.HsWs + q] - cx) / pitch + 0.5f * (float)(a.nx - 1);
  const float v = (a.beta_y[(size_t)b * a.HsWs + q] - cy) / pitch + 0.5f * (float)(a.ny - 1);
  // the range test of gl_interp.h (false for NaN and infinities): such a ray has a row of exact zeros
  const bool in = u >= -2.f && u <= (float)(a.nx + 1) && v >= -2.f && v <= (float)(a.ny + 1);
  const float w = in ? pix_hat(v - (float)j) * pix_hat(u - (float)i) : 0.f;
  out[(size_t)blockIdx.y * a.HsWs + q] = w * out_scale;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_gather_kernel(PixArgs a, int p0, const float* __restrict__ planes) {
  const int n = blockIdx.x * PIX_WG + threadIdx.x;
  if (n >= a.n_pad) return;
  const int p = p0 + blockIdx.y, b = p / a.S;
  float v = 0.f;
  if (n < a.n_used) v = planes[(size_t)blockIdx.y * a.HW + a.pix[n]] / a.sigma[(size_t)b * a.n_used + n];
  a.Fw[(size_t)p * a.n_pad + n] = v;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_rhs_prep_kernel(PixArgs a) {
  const int n = blockIdx.x * PIX_WG + threadIdx.x, b = blockIdx.y;
  if (n >= a.n_pad) return;
  float v = 0.f;
  if (n < a.n_used) {
    const float ll = a.lens_light ? a.lens_light[(size_t)b * a.HW + a.pix[n]] : 0.f;
    v = (a.obs[(size_t)b * a.n_used + n] - ll) / a.sigma[(size_t)b * a.n_used + n];
  }
  a.yw[(size_t)b * a.n_pad + n] = v;
}

// tile t of the lower triangle, row-major: (ti, tj) with tj <= ti
__device__ inline void pix_tri_tile(int t, int& ti, int& tj) {
  ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  tj = t - ti * (ti + 1) / 2;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_normal_kernel(PixArgs a) {
  __shared__ float Fi[PIX_TK][PIX_TK + 1], Fj[PIX_TK][PIX_TK + 1];
  int ti, tj;
  pix_tri_tile(blockIdx.x, ti, tj);
  const int b = blockIdx.y, i0 = ti * PIX_TK, j0 = tj * PIX_TK;
  const float* F = a.Fw + (size_t)b * a.S * a.n_pad;
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
  const int lr = threadIdx.x >> 5, lk = threadIdx.x & 31;
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int k0 = 0; k0 < a.n_pad; k0 += PIX_TK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = lr + 8 * q;
      Fi[r][lk] = i0 + r < a.S ? F[(size_t)(i0 + r) * a.n_pad + k0 + lk] : 0.f;
      Fj[r][lk] = j0 + r < a.S ? F[(size_t)(j0 + r) * a.n_pad + k0 + lk] : 0.f;
    }
    __syncthreads();
    float t[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < PIX_TK; ++k) {
      const float a0 = Fi[tr][k], a1 = Fi[tr + 16][k], b0 = Fj[tc][k], b1 = Fj[tc + 16][k];
      t[0][0] = fmaf(a0, b0, t[0][0]);
      t[0][1] = fmaf(a0, b1, t[0][1]);
      t[1][0] = fmaf(a1, b0, t[1][0]);
      t[1][1] = fmaf(a1, b1, t[1][1]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[r][c] += t[r][c];
    __syncthreads();
  }
  float* A = a.A0 + (size_t)b * a.S * a.S;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int i = i0 + tr + 16 * r, j = j0 + tc + 16 * c;
      if (i < a.S && j <= i) {
        A[(size_t)i * a.S + j] = acc[r][c];
        A[(size_t)j * a.S + i] = acc[r][c];
      }
    }
}

__device__ inline float pix_wave_sum(float v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ inline double pix_wave_sum(double v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_rhs_kernel(PixArgs a) {
  const int s = blockIdx.x * (PIX_WG / 64) + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
  if (s >= a.S) return;
  const float* f = a.Fw + ((size_t)b * a.S + s) * a.n_pad;
  const float* y = a.yw + (size_t)b * a.n_pad;
  float acc = 0.f;
  for (int n = lane; n < a.n_pad; n += 64) acc = fmaf(f[n], y[n], acc);
  acc = pix_wave_sum(acc);
  if (lane == 0) a.bvec[(size_t)b * a.S + s] = acc;
}

// entries of the one-dimensional factors of R: T_n = tridiag(-1, 2, -1) (gradient) or T_n^2 (curvature), zero-extended source
__device__ inline float pix_r1(int reg, int n, int p, int q) {
  const int d = p > q ? p - q : q - p;
  if (reg == PIX_REG_GRADIENT) return d == 0 ? 2.f : (d == 1 ? -1.f : 0.f);
  if (d == 0) return 4.f + (p > 0 ? 1.f : 0.f) + (p < n - 1 ? 1.f : 0.f);
  return d == 1 ? -4.f : (d == 2 ? 1.f : 0.f);
}

// (R s) at node (j, i), in float64 sums of float32 products' operands
__device__ inline double pix_rs(int reg, int ny, int nx, const float* s, int j, int i) {
  if (reg == PIX_REG_IDENTITY) return (double)s[j * nx + i];
  double acc = 0.0;
  for (int d = -2; d <= 2; ++d) {
    if (i + d >= 0 && i + d < nx) acc += (double)pix_r1(reg, nx, i, i + d) * (double)s[j * nx + i + d];
    if (j + d >= 0 && j + d < ny) acc += (double)pix_r1(reg, ny, j, j + d) * (double)s[(j + d) * nx + i];
  }
  return acc;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_solve_kernel(PixArgs a) {
  __shared__ float D[PIX_TK][PIX_TK + 1], Pa[PIX_TK][PIX_TK + 1], Pb[PIX_TK][PIX_TK + 1];
  __shared__ float dg[PIX_TK];
  __shared__ float z[PIX_MAX_S], s0[PIX_MAX_S];
  const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, S = a.S, nx = a.nx;
  const float lam = a.strength[(size_t)b * a.L_total + l];
  const float* A0 = a.A0 + (size_t)b * S * S;
  float* M = a.M + ((size_t)b * a.L + l) * (size_t)S * S;
  // M = A0 + lambda R, lower triangle (the stencil of R reaches two nodes back along either axis)
  for (int p = tid; p < S * S; p += PIX_WG) {
    const int r = p / S, c = p - r * S;
    if (c <= r) M[p] = A0[p];
  }
  __syncthreads();
  for (int p = tid; p < S; p += PIX_WG) {
    const int j = p / nx, i = p - j * nx;
    float* row = M + (size_t)p * S;
    if (a.reg == PIX_REG_IDENTITY) {
      row[p] += lam;
    } else {
      row[p] += lam * (pix_r1(a.reg, nx, i, i) + pix_r1(a.reg, a.ny, j, j));
      for (int d = 1; d <= 2; ++d) {
        if (i - d >= 0) row[p - d] += lam * pix_r1(a.reg, nx, i, i - d);
        if (j - d >= 0) row[p - d * nx] += lam * pix_r1(a.reg, a.ny, j, j - d);
      }
    }
  }
  __syncthreads();
  // (a thread owns row p, and no two of its additions meet: an x neighbour p - d' and a y neighbour p - d nx coincide only for
  // d' = d nx, i.e. nx = 1 or nx = 2 with d' = 2, and there i - d' >= 0 never holds)
  bool ok = true;
  double logdet = 0.0;
  const int tr = tid >> 3, tc4 = (tid & 7) * 4;
  for (int k0 = 0; k0 < S && ok; k0 += PIX_TK) {
    const int nb = min(PIX_TK, S - k0);
    for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
      const int r = e >> 5, c = e & 31;
      D[r][c] = (r < nb && c <= r) ? M[(size_t)(k0 + r) * S + k0 + c] : (r == c ? 1.f : 0.f);
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const float p = D[j][j];  // uniform
      if (!(p > 0.f && p < __builtin_inff())) { ok = false; break; }
      const float lj = sqrtf(p);
      if (tid == 0) { logdet += log((double)p); dg[j] = lj; }
      if (tid > j && tid < nb) D[tid][j] /= lj;
      __syncthreads();
      for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
        const int r = e >> 5, c = e & 31;
        if (c > j && c <= r && r < nb) D[r][c] = fmaf(-D[r][j], D[c][j], D[r][c]);
      }
      __syncthreads();
    }
    if (!ok) break;
    if (tid < nb) D[tid][tid] = dg[tid];
    __syncthreads();
    for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
      const int r = e >> 5, c = e & 31;
      if (r < nb && c <= r) M[(size_t)(k0 + r) * S + k0 + c] = D[r][c];
    }
    const int r0 = k0 + PIX_TK;  // rows below the block (then nb == PIX_TK)
    // panel: row i of L[:, k0 .. k0+31] = A[i, k0 ..] D^-T, one thread a row
    for (int i = r0 + tid; i < S; i += PIX_WG) {
      float* row = M + (size_t)i * S + k0;
      float x[PIX_TK];
#pragma unroll
      for (int c = 0; c < PIX_TK; ++c) x[c] = row[c];
#pragma unroll
      for (int c = 0; c < PIX_TK; ++c) {
        float t = x[c];
#pragma unroll
        for (int k = 0; k < c; ++k) t = fmaf(-x[k], D[c][k], t);
        x[c] = t / D[c][c];
      }
#pragma unroll
      for (int c = 0; c < PIX_TK; ++c) row[c] = x[c];
    }
    __syncthreads();
    // trailing update A[i][j] -= sum_k L[i][k] L[j][k], 32 x 32 tiles of the lower triangle, a thread 4 consecutive columns of a row
    for (int ib = r0; ib < S; ib += PIX_TK) {
      for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
        const int r = e >> 5, c = e & 31;
        Pa[r][c] = ib + r < S ? M[(size_t)(ib + r) * S + k0 + c] : 0.f;
      }
      for (int jb = r0; jb <= ib; jb += PIX_TK) {
        for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
          const int r = e >> 5, c = e & 31;
          Pb[r][c] = jb + r < S ? M[(size_t)(jb + r) * S + k0 + c] : 0.f;
        }
        __syncthreads();
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < PIX_TK; ++k) {
          const float av = Pa[tr][k];
#pragma unroll
          for (int q = 0; q < 4; ++q) t[q] = fmaf(av, Pb[tc4 + q][k], t[q]);
        }
        const int i = ib + tr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jj = jb + tc4 + q;
          if (i < S && jj <= i) M[(size_t)i * S + jj] -= t[q];
        }
        __syncthreads();
      }
    }
  }
  const size_t o = (size_t)b * a.L_total + l;
  if (tid == 0) a.ok[o] = ok ? 1 : 0;
  float* src = a.source + o * S;
  if (!ok) {  // uniform
    const float nan = __builtin_nanf("");
    for (int p = tid; p < S; p += PIX_WG) src[p] = nan;
    if (tid == 0) a.scal[3 * o + 2] = (double)nan;
    return;
  }
  if (tid == 0) a.scal[3 * o + 2] = logdet;
  // L w = b, then L^T s = w, in blocks of 32: the diagonal block by the first 32 lanes of wave 0, the rest one thread an entry.
  // Twice: the second pass solves for the residual b - M s0 of the first, formed in float64 from A0 (symmetric: a thread reads a
  // column, coalesced) and the stencil -- one step of iterative refinement, which takes the float32 factorisation's error
  // (cond(M) x its rounding) out of the solution and leaves the rounding of A0 and b themselves.
  for (int p = tid; p < S; p += PIX_WG) z[p] = a.bvec[(size_t)b * S + p];
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < S; k0 += PIX_TK) {
      const int nb = min(PIX_TK, S - k0);
      for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
        const int r = e >> 5, c = e & 31;
        D[r][c] = (r < nb && c <= r) ? M[(size_t)(k0 + r) * S + k0 + c] : (r == c ? 1.f : 0.f);
      }
      __syncthreads();
      if (tid < 64) {
        const int r = tid & 31;
        float zr = r < nb ? z[k0 + r] : 0.f;
        for (int c = 0; c < nb; ++c) {
          const float zc = __shfl(zr, c, 64) / D[c][c];
          if (r == c) zr = zc;
          else if (r > c) zr = fmaf(-D[r][c], zc, zr);
        }
        if (tid < nb) z[k0 + r] = zr;
      }
      __syncthreads();
      for (int i = k0 + PIX_TK + tid; i < S; i += PIX_WG) {
        const float* row = M + (size_t)i * S + k0;
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < PIX_TK; ++k) t = fmaf(row[k], z[k0 + k], t);
        z[i] -= t;
      }
      __syncthreads();
    }
    for (int k0 = ((S - 1) / PIX_TK) * PIX_TK; k0 >= 0; k0 -= PIX_TK) {
      const int nb = min(PIX_TK, S - k0);
      for (int e = tid; e < PIX_TK * PIX_TK; e += PIX_WG) {
        const int r = e >> 5, c = e & 31;
        D[r][c] = (r < nb && c <= r) ? M[(size_t)(k0 + r) * S + k0 + c] : (r == c ? 1.f : 0.f);
      }
      __syncthreads();
      if (tid < 64) {
        const int c = tid & 31;
        float zc = c < nb ? z[k0 + c] : 0.f;
        for (int r = nb - 1; r >= 0; --r) {
          const float sr = __shfl(zc, r, 64) / D[r][r];
          if (c == r) zc = sr;
          else if (c < r) zc = fmaf(-D[r][c], sr, zc);
        }
        if (tid < nb) z[k0 + c] = zc;
      }
      __syncthreads();
      for (int j = tid; j < k0; j += PIX_WG) {
        float t = 0.f;
        for (int r = 0; r < nb; ++r) t = fmaf(M[(size_t)(k0 + r) * S + j], z[k0 + r], t);
        z[j] -= t;
      }
      __syncthreads();
    }
    if (pass == 0) {
      for (int p = tid; p < S; p += PIX_WG) s0[p] = z[p];
      __syncthreads();
      for (int p = tid; p < S; p += PIX_WG) {
        double acc = (double)a.bvec[(size_t)b * S + p];
        for (int j = 0; j < S; ++j) acc = fma(-(double)A0[(size_t)j * S + p], (double)s0[j], acc);
        acc -= (double)lam * pix_rs(a.reg, a.ny, nx, s0, p / nx, p % nx);
        z[p] = (float)acc;
      }
      __syncthreads();
    }
  }
  for (int p = tid; p < S; p += PIX_WG) src[p] = s0[p] + z[p];
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_combine_kernel(PixArgs a) {
  __shared__ float s[PIX_MAX_S];
  __shared__ double red[2][PIX_WG / 64];
  const int b = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, S = a.S;
  const size_t o = (size_t)b * a.L_total + l;
  float* model = a.model + o * a.HW;
  const float nan = __builtin_nanf("");
  if (!a.ok[o]) {  // uniform
    for (int k = tid; k < a.HW; k += PIX_WG) model[k] = nan;
    if (tid == 0) { a.scal[3 * o] = (double)nan; a.scal[3 * o + 1] = (double)nan; }
    return;
  }
  for (int p = tid; p < S; p += PIX_WG) s[p] = a.source[o * S + p];
  for (int k = tid; k < a.HW; k += PIX_WG) model[k] = a.lens_light ? a.lens_light[(size_t)b * a.HW + k] : 0.f;
  __syncthreads();  // (also orders the fill of `model` before the used pixels are added below: same workgroup)
  const float* F = a.Fw + (size_t)b * S * a.n_pad;
  double chi2 = 0.0, reg = 0.0;
  for (int n = tid; n < a.n_used; n += PIX_WG) {
    double acc = 0.0;  // float64: chi2 is a small difference of two long sums
    for (int p = 0; p < S; ++p) acc = fma((double)F[(size_t)p * a.n_pad + n], (double)s[p], acc);
    const double r = (double)a.yw[(size_t)b * a.n_pad + n] - acc;
    chi2 += r * r;
    model[a.pix[n]] += (float)(acc * (double)a.sigma[(size_t)b * a.n_used + n]);
  }
  for (int p = tid; p < S; p += PIX_WG) reg += (double)s[p] * pix_rs(a.reg, a.ny, a.nx, s, p / a.nx, p % a.nx);
  chi2 = pix_wave_sum(chi2);
  reg = pix_wave_sum(reg);
  if ((tid & 63) == 0) { red[0][tid >> 6] = chi2; red[1][tid >> 6] = reg; }
  __syncthreads();
  if (tid == 0) {
    double c = 0.0, r = 0.0;
    for (int w = 0; w < PIX_WG / 64; ++w) { c += red[0][w]; r += red[1][w]; }
    a.scal[3 * o] = c;
    a.scal[3 * o + 1] = r;
  }
}

// ---- gradient of the evidence with respect to the rays (gl_pixsrc_evidence_grad) ---------------------------------------------
// With Fw = D P L, rw = yw - Fw s and E = -1/2 |rw|^2 - 1/2 lambda s^T R s - 1/2 log det M (s stationary for the first two terms,
// d log det M = 2 tr(M^-1 Fw^T dFw)):   dE/dF = D (rw s^T - Fw M^-1)  [n_used x S],   G = P^T (dE/dF scattered to the H x W image)
// [Hs Ws x S]  (P^T: the model's own post_bwd), and with u = (beta_x - cx) / pitch + (nx-1)/2, v likewise,
//   dE/dbeta_x[q] = (1/pitch) sum_(j,i) G[q,(j,i)] hat(v_q - j) hat'(u_q - i),   dE/dbeta_y[q] = (1/pitch) sum G hat'(v_q - j) hat(u_q - i),
// hat'(t) = -sign(t) for 0 < |t| < 1, else 0: at most the four nodes around (u_q, v_q) contribute, and a ray with a row of exact
// zeros in L (not finite, out of range) has a cotangent of exactly zero.  After the forward launches of a chunk of samples:
//   resid    (b, used pixel):     rw = yw - Fw s, the sum in float64 as combine has it
//   inv      (pooled pixel):      the inverse of `pix`: index of the used pixel, -1 elsewhere (once per call)
//   gimage   (b, pooled pixel):   grad_image = rw / sigma on the used pixels, 0 elsewhere
//   zsolve   (b, column of Fw):   Z = M^-1 Fw from the factor solve left in the workspace: one thread a right-hand side, forward and
//                                 back substitution in float32 in ascending / descending node order (columns past n_used are zero)
//   scatter  (plane, pooled px):  column (b, s) of dE/dF as a pooled plane: every element WRITTEN, no atomics, nothing to clear
//   post_bwd                      the model's own transpose of PSF + pooling over a chunk of planes
//   contract (b, subpixel):       one thread owns a supersampled pixel and adds the nodes of this chunk that are among its four,
//                                 in ascending node order; chunks arrive in launch order on one stream, so the order is fixed
struct PixGradArgs {
  const float* Z;     // [B][S][n_pad]  M^-1 Fw
  const float* rw;    // [B][n_pad]
  const int* inv;     // [HW] used-pixel index of a pooled pixel, or -1
  float* gbx;         // [B][HsWs] of this chunk
  float* gby;
  float* gimg;        // [B][HW] of this chunk
};

__global__ void __launch_bounds__(PIX_WG) gl_pix_resid_kernel(PixArgs a, float* __restrict__ rw) {
  const int n = blockIdx.x * PIX_WG + threadIdx.x, b = blockIdx.y;
  if (n >= a.n_pad) return;
  float r = 0.f;
  if (n < a.n_used) {
    const float* F = a.Fw + (size_t)b * a.S * a.n_pad;
    const float* s = a.source + (size_t)b * a.L_total * a.S;
    double acc = 0.0;
    for (int p = 0; p < a.S; ++p) acc = fma((double)F[(size_t)p * a.n_pad + n], (double)s[p], acc);
    r = (float)((double)a.yw[(size_t)b * a.n_pad + n] - acc);
  }
  rw[(size_t)b * a.n_pad + n] = r;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_inv_fill_kernel(int HW, int* __restrict__ inv) {
  const int k = blockIdx.x * PIX_WG + threadIdx.x;
  if (k < HW) inv[k] = -1;
}
__global__ void __launch_bounds__(PIX_WG) gl_pix_inv_set_kernel(const int* __restrict__ pix, int n_used, int HW, int* __restrict__ inv) {
  const int n = blockIdx.x * PIX_WG + threadIdx.x;
  if (n < n_used && pix[n] >= 0 && pix[n] < HW) inv[pix[n]] = n;
}

__global__ void __launch_bounds__(PIX_WG) gl_pix_gimage_kernel(PixArgs a, PixGradArgs g) {
  const int k = blockIdx.x * PIX_WG + threadIdx.x, b = blockIdx.y;
  if (k >= a.HW) return;
  const int n = g.inv[k];
  float v = 0.f;
  if (!a.ok[(size_t)b * a.L_total]) v = __builtin_nanf("");
  else if (n >= 0) v = g.rw[(size_t)b * a.n_pad + n] / a.sigma[(size_t)b * a.n_used + n];
  g.gimg[(size_t)b * a.HW + k] = v;
}

// Z [S][n_pad] of sample b: column n of Fw through L w = f, L^T z = w with the lower-triangle factor in a.M (one strength per sample).
// One wave per workgroup (the columns of a sample spread over many CUs); a row's dot product runs in four interleaved partial sums,
// added as (t0 + t1) + (t2 + t3): a fixed order that keeps four loads in flight instead of one.
constexpr int PIX_ZS_WG = 64;
__global__ void __launch_bounds__(PIX_ZS_WG) gl_pix_zsolve_kernel(PixArgs a, float* Zall) {
  const int n = blockIdx.x * PIX_ZS_WG + threadIdx.x, b = blockIdx.y, S = a.S;
  if (n >= a.n_pad || !a.ok[(size_t)b * a.L_total]) return;
  const float* Lf = a.M + (size_t)b * S * S;
  const float* F = a.Fw + (size_t)b * S * a.n_pad + n;
  float* Z = Zall + (size_t)b * S * a.n_pad + n;
  const size_t st = (size_t)a.n_pad;
  for (int i = 0; i < S; ++i) {
    const float* row = Lf + (size_t)i * S;
    float t0 = F[(size_t)i * st], t1 = 0.f, t2 = 0.f, t3 = 0.f;
    int k = 0;
    for (; k + 4 <= i; k += 4) {
      t0 = fmaf(-row[k], Z[(size_t)k * st], t0);
      t1 = fmaf(-row[k + 1], Z[(size_t)(k + 1) * st], t1);
      t2 = fmaf(-row[k + 2], Z[(size_t)(k + 2) * st], t2);
      t3 = fmaf(-row[k + 3], Z[(size_t)(k + 3) * st], t3);
    }
    for (; k < i; ++k) t0 = fmaf(-row[k], Z[(size_t)k * st], t0);
    Z[(size_t)i * st] = ((t0 + t1) + (t2 + t3)) / row[i];
  }
  for (int i = S - 1; i >= 0; --i) {
    float t0 = Z[(size_t)i * st], t1 = 0.f, t2 = 0.f, t3 = 0.f;
    int k = S - 1;
    for (; k - 4 >= i; k -= 4) {
      t0 = fmaf(-Lf[(size_t)k * S + i], Z[(size_t)k * st], t0);
      t1 = fmaf(-Lf[(size_t)(k - 1) * S + i], Z[(size_t)(k - 1) * st], t1);
      t2 = fmaf(-Lf[(size_t)(k - 2) * S + i], Z[(size_t)(k - 2) * st], t2);
      t3 = fmaf(-Lf[(size_t)(k - 3) * S + i], Z[(size_t)(k - 3) * st], t3);
    }
    for (; k > i; --k) t0 = fmaf(-Lf[(size_t)k * S + i], Z[(size_t)k * st], t0);
    Z[(size_t)i * st] = ((t0 + t1) + (t2 + t3)) / Lf[(size_t)i * S + i];
  }
}

// planes p0 .. p0 + gridDim.y - 1 of the chunk's flat (sample, node) list -> out[plane][k] = out_scale dE/dF[n(k), node] (0 off the used pixels)
__global__ void __launch_bounds__(PIX_WG) gl_pix_scatter_kernel(PixArgs a, PixGradArgs g, int p0, float out_scale, float* __restrict__ out) {
  const int k = blockIdx.x * PIX_WG + threadIdx.x;
  if (k >= a.HW) return;
  const int p = p0 + blockIdx.y, b = p / a.S, s = p - b * a.S;
  const int n = g.inv[k];
  float v = 0.f;
  if (n >= 0 && a.ok[(size_t)b * a.L_total]) {
    const float src = a.source[(size_t)b * a.L_total * a.S + s];
    v = out_scale * (g.rw[(size_t)b * a.n_pad + n] * src - g.Z[((size_t)b * a.S + s) * a.n_pad + n]) / a.sigma[(size_t)b * a.n_used + n];
  }
  out[(size_t)blockIdx.y * a.HW + k] = v;
}

__device__ inline float pix_dhat(float t) { return (t > 0.f && t < 1.f) ? -1.f : ((t < 0.f && t > -1.f) ? 1.f : 0.f); }

// samples b_lo .. b_lo + gridDim.y - 1 of the chunk, planes p0 .. p0 + np - 1 in G [np][HsWs]
__global__ void __launch_bounds__(PIX_WG) gl_pix_contract_kernel(PixArgs a, PixGradArgs g, int b_lo, int p0, int np, const float* __restrict__ G) {
  const int q = blockIdx.x * PIX_WG + threadIdx.x;
  if (q >= a.HsWs) return;
  const int b = b_lo + blockIdx.y;
  const size_t o = (size_t)b * a.HsWs + q;
  const bool first = b * a.S >= p0, last = (b + 1) * a.S <= p0 + np;  // this launch holds the sample's first / last plane
  float gx = first ? 0.f : g.gbx[o], gy = first ? 0.f : g.gby[o];
  const float pitch = a.pose[3 * b], cx = a.pose[3 * b + 1], cy = a.pose[3 * b + 2];
  const float u = (a.beta_x[o] - cx) / pitch + 0.5f * (float)(a.nx - 1);
  const float v = (a.beta_y[o] - cy) / pitch + 0.5f * (float)(a.ny - 1);
  const bool in = u >= -2.f && u <= (float)(a.nx + 1) && v >= -2.f && v <= (float)(a.ny + 1);
  if (in) {
    const int j0 = (int)floorf(v), i0 = (int)floorf(u);
    for (int dj = 0; dj < 2; ++dj)
      for (int di = 0; di < 2; ++di) {
        const int j = j0 + dj, i = i0 + di;
        if (j < 0 || j >= a.ny || i < 0 || i >= a.nx) continue;
        const int p = b * a.S + j * a.nx + i;
        if (p < p0 || p >= p0 + np) continue;
        const float w = G[(size_t)(p - p0) * a.HsWs + q];
        const float tu = u - (float)i, tv = v - (float)j;
        gx += w * pix_hat(tv) * pix_dhat(tu) / pitch;
        gy += w * pix_dhat(tv) * pix_hat(tu) / pitch;
      }
  }
  if (last && !a.ok[(size_t)b * a.L_total]) gx = gy = __builtin_nanf("");
  g.gbx[o] = gx;
  g.gby[o] = gy;
}

}  // namespace glk
