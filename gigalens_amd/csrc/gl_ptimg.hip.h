// gl_ptimg.hip.h -- point images in the pixel likelihood: PSF-rendered images of a lensed point source (quasar, supernova) with
// linear amplitudes (gl_ptimg_render, gl_ptimg_render_bwd, gl_ptimg_fit; LensSimulator.point_images, fit_point_images,
// point_image_log_like_and_grad).  The reference renders extended light only.
//
// The unit point image D(x, y) [H][W] of a position (x, y) in arcsec.  With (u, v) its position in supersampled pixel coordinates
// (u along the columns, v along the rows; u = m00 (x - x0) + m01 (y - y0), v = m10 (x - x0) + m11 (y - y0), the inverse of the
// camera's pix2angle on the supersampled grid):
//   splat     a zero supersampled frame gets wv[j] wu[i] at node (floor(v) - 1 + j, floor(u) - 1 + i), i, j = 0..3, with Keys' cubic
//             weights (a = -1/2, those of gl_interp.h order 3) at t = u - floor(u), v - floor(v); nodes outside the frame are dropped
//   convolve  the chain of simulate(): flip the PSF, cross-correlate with SAME padding ((k - 1) / 2 zeros before, k / 2 after)
//   pool      the SUM over ss x ss sub-pixels, no det T: the amplitude of an image is its flux in image counts
// The kernels compute the same function in gather form and never form the frame: sub-pixel (i, j) of the convolved frame is
//   sum_mn k(m - qv) k(n - qu) P[m][n],  qv = kh / 2 + i - v,  qu = kw / 2 + j - u          (k: Keys' kernel, P: the PSF as given)
// the cubic interpolation of the zero-extended PSF at (qv, qu).  Every sub-pixel of one image shares the fractional parts
// ceil(v) - v and ceil(u) - u, so the four weights of an axis are formed once per image; tap a of the row axis is the splat node
// ceil(v) + 1 - a whatever the sub-pixel, so "dropped outside the frame" is a mask on the four weights.  The PSF table carries a
// two-node zero apron (the layout idea of InterpTab) and tap indices are clamped into it, never tested.
//
// The weights are written in factored form, w0 = -t s^2 / 2, w1 = s (1 + t (1 - 3 t / 2)), w2 = w1(s), w3 = w0(s) with s = 1 - t
// (the same polynomials as glp::interp_weights, whose Horner form loses all relative accuracy next to their zeros at t -> 1):
// where one tap alone meets the PSF -- the rim of the footprint, or no PSF at all -- the pixel IS that weight.
//
// A position that is not finite, or further outside the frame than the PSF and four nodes, fails a range test made in float before
// anything becomes an integer: its box is empty, D = 0 and every derivative is 0.
//
// Kernels, all deterministic (no atomics; every sum has a fixed order; a sample does not depend on the others):
//   columns  (image, sample)  D and, GRAD, dD/du and dD/dv on the image's bounding box of final pixels (at most
//                             ceil((k + 3) / ss) + 1 a side) into the workspace, with the box origin and size
//   solve    (sample)         N_jk = sum_U w D_j D_k over box intersections, r_j = sum_U w D_j (obs - E): one wave per sum, lanes
//                             stride the pixels of box j, float64 accumulation, xor butterfly; Cholesky of the J x J system in
//                             float64 on one lane; ok = 0 where a pivot is not finite or not above PTI_PIVOT_TOL x its diagonal
//   residual (sample)         every final pixel gathers the boxes that cover it (image order): model = E + sum a_j D_j, the
//                             cotangent w (obs - model), chi2 in float64; GRAD: the adjoint below on that cotangent
//   render   (pixels, sample) sum a_j D_j
//   adjoint  (sample)         one wave per image: sum_box g D_j, a_j sum_box g dD_j/du, dv -> the (x, y) gradient by the chain rule
#pragma once
#include <hip/hip_runtime.h>

namespace glk {

constexpr int PTI_MAX_J = 8;     // images per sample
constexpr int PTI_WG = 256;
constexpr int PTI_COL_WG = 128;  // the columns kernel: a box is a few dozen pixels
constexpr int PTI_MAX_TAB = 12288;  // floats of the PSF table with its apron in LDS (48 KiB)
constexpr double PTI_PIVOT_TOL = 1e-6;  // a pivot this small against its diagonal entry is float32 rounding of the columns

struct PtImgArgs {
  int B, J;
  int H, W, ss;      // final frame and supersampling
  int kh, kw;        // PSF sides
  int stride;        // floats of one column plane in the workspace: the largest box
  double x0, y0, m00, m01, m10, m11;  // (u, v) = M (x - x0, y - y0), formed in float64 and rounded once
  const float* tab;  // [(kh + 4)][(kw + 4)]
  const float* x;    // [B][J]
  const float* y;
  const float* amp;  // [B][J]
  int* box;          // [B][J][4]: first row, first column, rows, columns (0 rows: empty)
  float* cols;       // [B][J][3][stride]: D, dD/du, dD/dv on the box, row-major with the box's own width
};

struct PtFitArgs {
  const float* ext;     // [B][H W] extended image
  const float* obs;     // [H W] or [B][H W]
  const float* weight;  // [H W] or [B][H W]: 1 / err^2 on the used pixels, 0 elsewhere
  int obs_stride, weight_stride;  // 0 or H W
  float* amp;           // [B][J]
  float* model;         // [B][H W]
  float* cot;           // [B][H W] weight (obs - model)
  double* chi2;         // [B]
  int* ok;              // [B]
  float *gx, *gy;       // [B][J], GRAD
};

__device__ inline double pti_wave_sum(double v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// Keys' weights of the taps floor(q) - 1 .. floor(q) + 2 at t = q - floor(q) in [0, 1], and their derivatives in q
__device__ inline void pti_weights(float t, float* w, float* d) {
  const float s = 1.f - t;
  w[0] = -0.5f * t * s * s;
  w[1] = s * fmaf(t, fmaf(-1.5f, t, 1.f), 1.f);
  w[2] = t * fmaf(s, fmaf(-1.5f, s, 1.f), 1.f);
  w[3] = -0.5f * s * t * t;
  d[0] = -0.5f * s * fmaf(-3.f, t, 1.f);
  d[1] = fmaf(4.5f, t, -5.f) * t;
  d[2] = -fmaf(4.5f, s, -5.f) * s;
  d[3] = -0.5f * t * fmaf(-3.f, t, 2.f);
}

__device__ inline int pti_clamp(int k, int lo, int hi) { return k < lo ? lo : (k > hi ? hi : k); }

template <bool GRAD>
__global__ void __launch_bounds__(PTI_COL_WG) gl_ptimg_columns_kernel(PtImgArgs a) {
  extern __shared__ float tab[];
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int tw = a.kw + 4, th = a.kh + 4;
  for (int k = tid; k < th * tw; k += PTI_COL_WG) tab[k] = a.tab[k];
  __syncthreads();
  const size_t bj = (size_t)b * a.J + j;
  const double dx = (double)a.x[bj] - a.x0, dy = (double)a.y[bj] - a.y0;
  const float u = (float)(a.m00 * dx + a.m01 * dy), v = (float)(a.m10 * dx + a.m11 * dy);
  const int Hs = a.H * a.ss, Ws = a.W * a.ss;
  // the range test, in float, before any conversion to int: false for NaN and for infinities
  const bool in = u >= -(float)(a.kw + 4) && u <= (float)(Ws + a.kw + 4) && v >= -(float)(a.kh + 4) && v <= (float)(Hs + a.kh + 4);
  const float us = in ? u : 0.f, vs = in ? v : 0.f;
  const float cuf = ceilf(us), cvf = ceilf(vs);
  const int cu = (int)cuf, cv = (int)cvf;
  float wu[4], du[4], wv[4], dv[4];
  pti_weights(cuf - us, wu, du);
  pti_weights(cvf - vs, wv, dv);
#pragma unroll
  for (int t = 0; t < 4; ++t) {  // tap t of an axis is the splat node ceil + 1 - t: dropped outside the frame
    const int r = cv + 1 - t, c = cu + 1 - t;
    if (r < 0 || r >= Hs) wv[t] = dv[t] = 0.f;
    if (c < 0 || c >= Ws) wu[t] = du[t] = 0.f;
  }
  // sub-pixels that can differ from zero: PSF node g = k / 2 + i - ceil in [-2, k], clipped to the frame; then their final pixels
  const int cr = a.kh / 2, cc = a.kw / 2;
  const int i_lo = max(cv - cr - 2, 0), i_hi = min(cv - cr + a.kh, Hs - 1);
  const int j_lo = max(cu - cc - 2, 0), j_hi = min(cu - cc + a.kw, Ws - 1);
  const bool live = in && i_lo <= i_hi && j_lo <= j_hi;
  const int oy = live ? i_lo / a.ss : 0, ox = live ? j_lo / a.ss : 0;
  const int ny = live ? i_hi / a.ss - oy + 1 : 0, nx = live ? j_hi / a.ss - ox + 1 : 0;
  if (tid == 0) {
    int* bx = a.box + 4 * bj;
    bx[0] = oy; bx[1] = ox; bx[2] = ny; bx[3] = nx;
  }
  float* out = a.cols + bj * 3 * (size_t)a.stride;
  for (int p = tid; p < ny * nx; p += PTI_COL_WG) {
    const int py = p / nx, px = p - py * nx;
    float S = 0.f, Su = 0.f, Sv = 0.f;
    for (int si = 0; si < a.ss; ++si) {
      const int g = cr + (oy + py) * a.ss + si - cv;  // floor(qv)
      int row[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) row[t] = (pti_clamp(g - 1 + t, -2, a.kh + 1) + 2) * tw;
      for (int sj = 0; sj < a.ss; ++sj) {
        const int h = cc + (ox + px) * a.ss + sj - cu;  // floor(qu)
        int col[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) col[t] = pti_clamp(h - 1 + t, -2, a.kw + 1) + 2;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float* r = tab + row[t];
          const float a0 = r[col[0]], a1 = r[col[1]], a2 = r[col[2]], a3 = r[col[3]];
          // (explicit fused multiply-adds: both instantiations form the image with the same operations)
          const float rs = fmaf(wu[3], a3, fmaf(wu[2], a2, fmaf(wu[1], a1, wu[0] * a0)));
          S = fmaf(wv[t], rs, S);
          if (GRAD) {
            Su = fmaf(wv[t], fmaf(du[3], a3, fmaf(du[2], a2, fmaf(du[1], a1, du[0] * a0))), Su);
            Sv = fmaf(dv[t], rs, Sv);
          }
        }
      }
    }
    out[p] = S;
    if (GRAD) {  // d qu / du = d qv / dv = -1
      out[a.stride + p] = -Su;
      out[2 * a.stride + p] = -Sv;
    }
  }
}

// box headers of one sample into LDS (the caller synchronises)
__device__ inline void pti_load_boxes(const PtImgArgs& a, int b, int (*box)[4]) {
  if ((int)threadIdx.x < 4 * a.J) box[threadIdx.x >> 2][threadIdx.x & 3] = a.box[(size_t)b * a.J * 4 + threadIdx.x];
}

// D_k (plane 0) at final pixel (gy, gx), 0 outside box k
__device__ inline float pti_at(const PtImgArgs& a, int b, int k, const int (*box)[4], int gy, int gx, int plane = 0) {
  const int ky = gy - box[k][0], kx = gx - box[k][1];
  if (ky < 0 || ky >= box[k][2] || kx < 0 || kx >= box[k][3]) return 0.f;
  return a.cols[(((size_t)b * a.J + k) * 3 + plane) * a.stride + ky * box[k][3] + kx];
}

__global__ void __launch_bounds__(PTI_WG) gl_ptimg_solve_kernel(PtImgArgs a, PtFitArgs f) {
  __shared__ int box[PTI_MAX_J][4];
  __shared__ double Nm[PTI_MAX_J][PTI_MAX_J], rv[PTI_MAX_J];
  __shared__ double L[PTI_MAX_J][PTI_MAX_J], z[PTI_MAX_J];  // the factor and the solution: one lane's, kept out of scratch
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, J = a.J, HW = a.H * a.W;
  pti_load_boxes(a, b, box);
  __syncthreads();
  const float* wgt = f.weight + (size_t)b * f.weight_stride;
  const float* obs = f.obs + (size_t)b * f.obs_stride;
  const float* ext = f.ext + (size_t)b * HW;
  const int n_pair = J * (J + 1) / 2;
  for (int s = wave; s < n_pair + J; s += PTI_WG / 64) {  // (wave-uniform: the butterfly below runs on whole waves)
    int j = 0, k = -1;
    if (s < n_pair) {
      while ((j + 1) * (j + 2) / 2 <= s) ++j;
      k = s - j * (j + 1) / 2;
    } else {
      j = s - n_pair;
    }
    const int nxj = box[j][3], nj = box[j][2] * nxj;
    const float* Dj = a.cols + ((size_t)b * J + j) * 3 * a.stride;
    double acc = 0.0;
    for (int p = lane; p < nj; p += 64) {
      const int py = p / nxj, gy = box[j][0] + py, gx = box[j][1] + p - py * nxj, q = gy * a.W + gx;
      const double wd = (double)wgt[q] * (double)Dj[p];
      if (wd != 0.0) acc += wd * (k >= 0 ? (double)pti_at(a, b, k, box, gy, gx) : (double)obs[q] - (double)ext[q]);
    }
    acc = pti_wave_sum(acc);
    if (lane == 0) {
      if (k >= 0) Nm[j][k] = Nm[k][j] = acc;
      else rv[j] = acc;
    }
  }
  __syncthreads();
  if (tid == 0) {
    bool ok = true;
    for (int c = 0; c < J && ok; ++c) {
      double d = Nm[c][c];
      for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
      // (false for a NaN and for an infinite diagonal)
      ok = d > PTI_PIVOT_TOL * Nm[c][c] && d < __builtin_huge_val();
      if (!ok) break;
      L[c][c] = sqrt(d);
      for (int r = c + 1; r < J; ++r) {
        double t = Nm[r][c];
        for (int k = 0; k < c; ++k) t -= L[r][k] * L[c][k];
        L[r][c] = t / L[c][c];
      }
    }
    if (ok) {
      for (int r = 0; r < J; ++r) {
        double t = rv[r];
        for (int k = 0; k < r; ++k) t -= L[r][k] * z[k];
        z[r] = t / L[r][r];
      }
      for (int r = J - 1; r >= 0; --r) {
        double t = z[r];
        for (int k = r + 1; k < J; ++k) t -= L[k][r] * z[k];
        z[r] = t / L[r][r];
        ok = ok && z[r] - z[r] == 0.0;  // a right-hand side that is not finite
      }
    }
    for (int r = 0; r < J; ++r) f.amp[(size_t)b * J + r] = ok ? (float)z[r] : __builtin_nanf("");
    f.ok[b] = ok ? 1 : 0;
  }
}

// One wave per image: g_amp = sum_box g D_j, (g_u, g_v) = a_j sum_box g (dD_j/du, dD_j/dv), (g_x, g_y) = M^T (g_u, g_v).  `g` is the
// cotangent image of the sample; amp its amplitudes; g_amp may be null.  A sample that is not `ok` gets NaN.
__device__ inline void pti_adjoint(const PtImgArgs& a, int b, const int (*box)[4], const float* g, const float* amp, bool ok,
                                   float* g_amp, float* g_x, float* g_y) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = wave; j < a.J; j += PTI_WG / 64) {
    const int nxj = box[j][3], nj = box[j][2] * nxj;
    const float* Dj = a.cols + ((size_t)b * a.J + j) * 3 * a.stride;
    double sa = 0.0, su = 0.0, sv = 0.0;
    for (int p = lane; p < nj; p += 64) {
      const int py = p / nxj;
      const float c = g[(box[j][0] + py) * a.W + box[j][1] + p - py * nxj];
      if (c != 0.f) {
        sa += (double)c * (double)Dj[p];
        su += (double)c * (double)Dj[a.stride + p];
        sv += (double)c * (double)Dj[2 * a.stride + p];
      }
    }
    sa = pti_wave_sum(sa);
    su = pti_wave_sum(su);
    sv = pti_wave_sum(sv);
    if (lane == 0) {
      const size_t bj = (size_t)b * a.J + j;
      const double aj = (double)amp[bj];
      const float nan = __builtin_nanf("");
      if (g_amp) g_amp[bj] = ok ? (float)sa : nan;
      g_x[bj] = ok ? (float)(aj * (a.m00 * su + a.m10 * sv)) : nan;
      g_y[bj] = ok ? (float)(aj * (a.m01 * su + a.m11 * sv)) : nan;
    }
  }
}

template <bool GRAD>
__global__ void __launch_bounds__(PTI_WG) gl_ptimg_residual_kernel(PtImgArgs a, PtFitArgs f) {
  __shared__ int box[PTI_MAX_J][4];
  __shared__ float amp[PTI_MAX_J];
  __shared__ double part[PTI_WG / 64];
  const int b = blockIdx.x, tid = threadIdx.x, J = a.J, HW = a.H * a.W;
  pti_load_boxes(a, b, box);
  if (tid < J) amp[tid] = f.amp[(size_t)b * J + tid];
  __syncthreads();
  const bool ok = f.ok[b] != 0;
  const float* wgt = f.weight + (size_t)b * f.weight_stride;
  const float* obs = f.obs + (size_t)b * f.obs_stride;
  const float* ext = f.ext + (size_t)b * HW;
  float* model = f.model + (size_t)b * HW;
  float* cot = f.cot + (size_t)b * HW;
  const float nan = __builtin_nanf("");
  double chi = 0.0;
  for (int q = tid; q < HW; q += PTI_WG) {
    const int gy = q / a.W, gx = q - gy * a.W;
    float pt = 0.f;
    for (int j = 0; j < J; ++j) pt = fmaf(amp[j], pti_at(a, b, j, box, gy, gx), pt);
    const float m = ext[q] + pt, w = wgt[q];
    const float res = w != 0.f ? obs[q] - m : 0.f, c = w * res;
    model[q] = ok ? m : nan;
    cot[q] = ok ? c : nan;
    chi += (double)c * (double)res;
  }
  chi = pti_wave_sum(chi);
  if ((tid & 63) == 0) part[tid >> 6] = chi;
  __threadfence_block();  // GRAD: the cotangent image this workgroup wrote is read back below
  __syncthreads();
  if (tid == 0) {
    double t = part[0];
    for (int k = 1; k < PTI_WG / 64; ++k) t += part[k];
    f.chi2[b] = ok ? t : (double)nan;
  }
  if (GRAD) pti_adjoint(a, b, box, cot, f.amp, ok, nullptr, f.gx, f.gy);
}

__global__ void __launch_bounds__(PTI_WG) gl_ptimg_render_kernel(PtImgArgs a, float* __restrict__ image) {
  __shared__ int box[PTI_MAX_J][4];
  __shared__ float amp[PTI_MAX_J];
  const int b = blockIdx.y, tid = threadIdx.x, HW = a.H * a.W;
  pti_load_boxes(a, b, box);
  if (tid < a.J) amp[tid] = a.amp[(size_t)b * a.J + tid];
  __syncthreads();
  const int q = blockIdx.x * PTI_WG + tid;
  if (q >= HW) return;
  const int gy = q / a.W, gx = q - gy * a.W;
  float pt = 0.f;
  for (int j = 0; j < a.J; ++j) {
    const float d = pti_at(a, b, j, box, gy, gx);
    if (d != 0.f) pt = fmaf(amp[j], d, pt);  // (an amplitude that is not finite stays inside its own box)
  }
  image[(size_t)b * HW + q] = pt;
}

__global__ void __launch_bounds__(PTI_WG) gl_ptimg_adjoint_kernel(PtImgArgs a, const float* __restrict__ grad_image, float* g_amp,
                                                                  float* g_x, float* g_y) {
  __shared__ int box[PTI_MAX_J][4];
  const int b = blockIdx.x;
  pti_load_boxes(a, b, box);
  __syncthreads();
  pti_adjoint(a, b, box, grad_image + (size_t)b * a.H * a.W, a.amp, true, g_amp, g_x, g_y);
}

}  // namespace glk
