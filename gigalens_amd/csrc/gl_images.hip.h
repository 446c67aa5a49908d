// gl_images.hip.h -- the lens-equation solver: the images theta of a source position beta_s, beta(theta) = beta_s, for every
// sample of lens parameters (gl_image_positions; LensSimulator.image_positions).  The reference maps only image plane -> source
// plane; this inverts it on a search window with the same point evaluation of beta and the Hessian as the image-position
// likelihood (lens_point<R> of gl_positions.hip.h: built-in kinds, GL_SCALED catalogues, user-written lenses through the
// run-time compiled point program).  Three kernels, all on the caller's stream, no host synchronisation, no allocation:
//   map     (sample, vertex):  beta at the (n+1)^2 vertices of a regular n x n grid of cells over the window, lens_point<float>;
//                              a vertex whose beta is not finite (a singular lens centre) is stored as NaN: it flags its triangles
//   scan    (sample, source):  one workgroup of IMG_SCAN_WG threads walks the 2 n^2 triangles (two per cell) in a fixed order;
//                              a triangle whose image in the source plane contains beta_s is a candidate, with the preimage of
//                              beta_s under the triangle's affine map as its seed; hits are compacted per wave (ballot + mbcnt)
//                              into a wave-private LDS list and the lists are concatenated in wave order, i.e. in triangle order
//   newton (sample, source):   one wave; lane k refines candidate k by Newton on Dual<float, 2> (beta and Hessian as P1 of the
//                              positions likelihood), theta <- theta + (I - H)^-1 (beta_s - beta(theta)), keeps the signed
//                              mu = 1 / det(I - H) at the converged point, then lane 0 merges duplicates and sorts the images
// Output per (sample, source): n images sorted by x, then y (NaN-padded to max_images), and n_dropped = candidates that did not
// converge or converged outside the window + triangle hits beyond the candidate list + images beyond max_images.  A candidate
// whose seed misses beta_s by more than a cell side (its triangle straddles a singular lens centre) and does not converge is
// no image and is not counted.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_positions.hip.h"

namespace glk {

constexpr int IMG_SCAN_WG = 256;  // four waves; a 256^2 search grid is 131 072 triangles = 512 per lane
constexpr int IMG_MAXC = 64;      // candidates per (sample, source): one Newton lane each
constexpr float IMG_MERGE = 0.05f;  // converged candidates closer than this fraction of a cell side are one image

struct ImgArgs {
  const float* src_x;  // [B][S]
  const float* src_y;
  const float* src_scale;  // [S] deflection scale of every source (its own plane: beta_s = theta - c_s sum alpha), or null: all 1
  int S, n;            // sources per sample, cells per side
  float x_lo, x_hi, y_lo, y_hi;
  float hx, hy;        // cell sides
  int max_images, max_iter;
  float tol;
  float2* map;   // [B][(n+1)^2] beta at the vertices, row-major (y rows, x columns); NaN = flagged
  float2* cand;  // [B][S][IMG_MAXC] Newton seeds in triangle order
  int* n_cand;   // [B][S] seeds stored
  int* n_over;   // [B][S] triangle hits beyond the list
  float* out;      // [B][S][max_images][3]  x, y, mu
  int* n_images;   // [B][S]
  int* n_dropped;  // [B][S]
};

// The SIS deflection is DEFINED as 0 at its own centre (sis_fwd, as the reference has it), so a grid vertex that coincides bit for bit
// with the centre would see alpha = 0, H = 0 (beta = theta, D = 1) where the lens is singular (D -> -inf).  The map kernels of the
// solver and of the critical curves flag such a vertex instead (no other built-in kind defines a value at a singular centre).
__device__ inline bool lens_singular_at(const CompDesc& cd, const float* p, float x, float y) {
  return cd.kind == glp::K_SIS && x == p[1] && y == p[2];
}

__device__ inline float img_vx(const ImgArgs& g, int c) { return g.x_lo + (float)c * g.hx; }
__device__ inline float img_vy(const ImgArgs& g, int r) { return g.y_lo + (float)r * g.hy; }

// IM: the build for models that hold an interpolated lens (gl_positions.hip.h lens_point); the kernels of every other model are
// compiled without it and compute bit for bit what they did before that lens existed
template <bool IM> __device__ __forceinline__ void img_map_body(const PosArgs& a, const ImgArgs& g) {
  const int V1 = g.n + 1;
  const long long V = (long long)V1 * V1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= V * a.B) return;
  const int b = (int)(i / V), v = (int)(i - (long long)b * V);
  const int r = v / V1, c = v - r * V1;
  const float x = img_vx(g, c), y = img_vy(g, r);
  float bx = x, by = y;
  lens_deflections<IM>(a, b, x, y, [&](const CompDesc& cd, const float* p, float ax, float ay) {
    bx -= lens_singular_at(cd, p, x, y) ? __builtin_nanf("") : ax;
    by -= ay;
  });
  if (!(isfinite(bx) && isfinite(by))) bx = by = __builtin_nanf("");
  g.map[i] = float2{bx, by};
}
__global__ void __launch_bounds__(256) gl_img_map_kernel(PosArgs a, ImgArgs g) { img_map_body<false>(a, g); }
__global__ void __launch_bounds__(256) gl_img_map_im_kernel(PosArgs a, ImgArgs g) { img_map_body<true>(a, g); }

// edge function of the edge (p, q) at s, always evaluated with p = the vertex of lower index: the two triangles that share an
// edge then see bitwise the same value (up to an exact negation), which makes the tie rule below exact
__device__ inline float img_edge(float2 p, float2 q, float sx, float sy) {
#pragma clang fp contract(off)
  return (q.x - p.x) * (sy - p.y) - (q.y - p.y) * (sx - p.x);
}

// the stored map (beta of the reference plane at vertex v) on the plane of a source with scale c: theta + c (beta - theta).  A function
// of the vertex alone, without contraction: every triangle that touches the vertex sees bitwise the same value, so the tie rule of
// img_tri_hit still counts a source on a shared edge once
__device__ inline float2 img_vertex_beta(const ImgArgs& g, const float2* mp, int v, float c) {
#pragma clang fp contract(off)
  const float2 b1 = mp[v];
  if (c == 1.f) return b1;
  const int V1 = g.n + 1, r = v / V1, col = v - r * V1;
  const float x = img_vx(g, col), y = img_vy(g, r);
  return float2{x + c * (b1.x - x), y + c * (b1.y - y)};
}

// the stored map of one sample on the plane of a source with scale c, as the scan reads it: vertex -> beta
struct ImgVertexScaled {
  const ImgArgs& g;
  const float2* mp;
  float c;
  __device__ __forceinline__ float2 operator()(int v) const { return img_vertex_beta(g, mp, v, c); }
};

// Is beta_s inside the image of triangle t?  Cell (ci, cj) holds triangles k = 0: (v00, v10, v11) and k = 1: (v00, v11, v01).
// A point is inside when every oriented edge function is > 0; on an edge (== 0) it belongs to the triangle that owns that edge,
// and of two triangles sharing an edge with the same orientation exactly one owns it: the owner is the one whose oriented
// direction d along the edge has d.y > 0, or d.y == 0 and d.x > 0.  Triangles with a flagged vertex or zero area are skipped.
// VB: vertex -> beta on the plane of the source (ImgVertexScaled; gl_multiplane_images.hip.h: the plane sums with the source's couplings)
template <class VB>
__device__ inline bool img_tri_hit(const ImgArgs& g, const VB& vertex_beta, int t, float sx, float sy, float& seed_x, float& seed_y) {
  const int n = g.n, V1 = n + 1;
  const int cell = t >> 1, k = t & 1;
  const int cj = cell / n, ci = cell - cj * n;
  const int v00 = cj * V1 + ci;
  int vi[3] = {v00, k ? v00 + V1 + 1 : v00 + 1, k ? v00 + V1 : v00 + V1 + 1};
  float2 bv[3];
  for (int e = 0; e < 3; ++e) bv[e] = vertex_beta(vi[e]);
  float w[3], dx[3], dy[3];
  for (int e = 0; e < 3; ++e) {  // edge e runs from vertex e to vertex e+1
    const int p = e, q = e == 2 ? 0 : e + 1;
    const bool fwd = vi[p] < vi[q];
    const float2 lo = fwd ? bv[p] : bv[q], hi = fwd ? bv[q] : bv[p];
    const float f = fwd ? 1.f : -1.f;
    w[e] = f * img_edge(lo, hi, sx, sy);
    dx[e] = f * (hi.x - lo.x);
    dy[e] = f * (hi.y - lo.y);
  }
  const float W = w[0] + w[1] + w[2];  // twice the signed area (exactly its sign when all three share a sign)
  if (!(W != 0.f) || !isfinite(W)) return false;
  const float o = W > 0.f ? 1.f : -1.f;
  for (int e = 0; e < 3; ++e) {
    const float we = o * w[e], de_x = o * dx[e], de_y = o * dy[e];
    const bool owned = de_y > 0.f || (de_y == 0.f && de_x > 0.f);
    if (!(we > 0.f || (we == 0.f && owned))) return false;
  }
  // barycentric weights of the preimage: vertex e is opposite edge e+1
  const float l0 = w[1] / W, l1 = w[2] / W, l2 = w[0] / W;
  const float x0 = img_vx(g, ci), x1 = img_vx(g, ci + 1), y0 = img_vy(g, cj), y1 = img_vy(g, cj + 1);
  // vertex positions: k = 0 -> (x0,y0), (x1,y0), (x1,y1);  k = 1 -> (x0,y0), (x1,y1), (x0,y1)
  seed_x = l0 * x0 + l1 * x1 + l2 * (k ? x0 : x1);
  seed_y = l0 * y0 + l1 * (k ? y1 : y0) + l2 * y1;
  return true;
}

// the scan of (sample, source) pair bs = blockIdx.x over the triangles of the grid, their vertices read through vertex_beta
template <class VB> __device__ __forceinline__ void img_scan_body(const ImgArgs& g, int bs, const VB& vertex_beta) {
  constexpr int NW = IMG_SCAN_WG / 64;
  __shared__ float2 list[NW][IMG_MAXC];
  __shared__ int cnt[NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float sx = g.src_x[bs], sy = g.src_y[bs];
  // wave w walks the w-th quarter of the triangles, 64 consecutive triangles (32 cells of one row) per round
  const int T = 2 * g.n * g.n, per = (T + NW - 1) / NW;
  const int t0 = wave * per, t1 = min(T, t0 + per);
  int count = 0;
  for (int base = t0; base < t1; base += 64) {
    const int t = base + lane;
    float seed_x = 0.f, seed_y = 0.f;
    const bool hit = t < t1 && img_tri_hit(g, vertex_beta, t, sx, sy, seed_x, seed_y);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    const int rank = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (hit && rank < IMG_MAXC) list[wave][rank] = float2{seed_x, seed_y};
    count += __builtin_popcountll(m);
  }
  if (lane == 0) cnt[wave] = count;
  __syncthreads();
  if (wave != 0) return;
  int off = 0, total = 0;
  for (int w = 0; w < NW; ++w) {
    const int c = min(cnt[w], IMG_MAXC);
    for (int k = lane; k < c && off + k < IMG_MAXC; k += 64) g.cand[(size_t)bs * IMG_MAXC + off + k] = list[w][k];
    off = min(off + c, IMG_MAXC);
    total += cnt[w];
  }
  if (lane == 0) {
    g.n_cand[bs] = off;
    g.n_over[bs] = total - off;
  }
}
__global__ void __launch_bounds__(IMG_SCAN_WG) gl_img_scan_kernel(ImgArgs g) {
  const int bs = blockIdx.x, b = bs / g.S;
  const float c = g.src_scale ? g.src_scale[bs - b * g.S] : 1.f;
  const long long V1 = g.n + 1;
  img_scan_body(g, bs, ImgVertexScaled{g, g.map + (size_t)b * (size_t)(V1 * V1), c});
}

// beta and Hessian (f_xx, f_xy, f_yx, f_yy; the dPIS convergence excess included) at one point
// (c: the deflection scale of the source's plane; 1 leaves every value as the sum formed it)
template <bool IM = true>
__device__ inline void img_lens_eval(const PosArgs& a, int b, float px, float py, float& bx, float& by, float* h, float c = 1.f) {
  bx = px;
  by = py;
  h[0] = h[1] = h[2] = h[3] = 0.f;
  lens_jets<IM>(a, b, px, py, [&](const CompDesc&, const float*, const Jet2& ax, const Jet2& ay, float ex) {
    bx -= ax.v;
    by -= ay.v;
    h[0] += ax.d[0] + ex; h[1] += ax.d[1]; h[2] += ay.d[0]; h[3] += ay.d[1] + ex;
  });
  lens_rescale(c, px, py, bx, by, h);
}

// ... with the interpolated lens in the switch, always a function call (the device of crit_eval_cat in gl_critical.hip.h): inline,
// twice, beside the Newton state it does not fit the 256 VGPRs
static __device__ __attribute__((noinline)) void img_lens_eval_im(const PosArgs& a, int b, float px, float py, float& bx, float& by, float* h, float c) {
  img_lens_eval<true>(a, b, px, py, bx, by, h, c);
}
template <bool IM> __device__ __forceinline__ void img_lens_eval_of(const PosArgs& a, int b, float px, float py, float& bx, float& by, float* h, float c) {
  if constexpr (IM) img_lens_eval_im(a, b, px, py, bx, by, h, c);
  else img_lens_eval<false>(a, b, px, py, bx, by, h, c);
}
// the evaluation of the single-plane solver at one point of sample b, on the plane of scale c
template <bool IM> struct ImgEvalScaled {
  const PosArgs& a;
  int b;
  float c;
  __device__ __forceinline__ void operator()(float px, float py, float& bx, float& by, float* h) const {
    img_lens_eval_of<IM>(a, b, px, py, bx, by, h, c);
  }
};

// Newton, merge, sort and counters of (sample, source) pair bs = blockIdx.x; eval(px, py, bx, by, h): beta and f = I - A at one point
// on the plane of the source (ImgEvalScaled; gl_multiplane_images.hip.h: the plane recursion with the source's couplings)
template <class Eval> __device__ __forceinline__ void img_newton_core(const ImgArgs& g, const Eval& eval) {
  __shared__ float rx[IMG_MAXC], ry[IMG_MAXC], rmu[IMG_MAXC];
  __shared__ int rok[IMG_MAXC], order[IMG_MAXC];
  __shared__ int n_keep_s, n_bad_s;
  const int bs = blockIdx.x, lane = threadIdx.x;
  const int nc = g.n_cand[bs];
  const float sx = g.src_x[bs], sy = g.src_y[bs], tol2 = g.tol * g.tol;
  const float max_step = sqrtf(g.hx * g.hx + g.hy * g.hy);  // a step is at most one cell diagonal (folds: near-singular I - H)
  bool ok = false;
  float x = 0.f, y = 0.f, mu = 0.f;
  if (lane < nc) {
    const float2 s0 = g.cand[(size_t)bs * IMG_MAXC + lane];
    x = s0.x;
    y = s0.y;
    float bx, by, h[4];
    eval(x, y, bx, by, h);
    float r_x = sx - bx, r_y = sy - by, r2 = r_x * r_x + r_y * r_y;
    // the affine preimage misses beta_s by more than a cell side: the triangle straddles a singular or discontinuous point of
    // the deflection (the centre of an SIS / SIE / EPL with gamma >= 2), not a smooth neighbourhood of an image; if such a
    // candidate does not converge it is discarded without being counted
    const float hmax = fmaxf(g.hx, g.hy);
    const bool straddles = !(r2 <= hmax * hmax);
    // steps until converged; then one more (the point where |r| first drops below tol can be up to tol / |1 - kappa - gamma| off
    // the root, a polishing step brings it to the float32 noise floor) that is kept when its residual is not larger
    for (int it = 0; it <= g.max_iter; ++it) {
      const bool conv = r2 <= tol2;
      if (!conv && it == g.max_iter) break;
      const float a00 = 1.f - h[0], a01 = -h[1], a10 = -h[2], a11 = 1.f - h[3];
      const float det = a00 * a11 - a01 * a10;
      float dx = (a11 * r_x - a01 * r_y) / det, dy = (a00 * r_y - a10 * r_x) / det;
      const float len = sqrtf(dx * dx + dy * dy);
      if (!(len <= max_step)) {  // (also NaN)
        if (!isfinite(len)) { ok = conv; break; }
        dx *= max_step / len;
        dy *= max_step / len;
      }
      const float nx = x + dx, ny = y + dy;
      float nbx, nby, nh[4];
      eval(nx, ny, nbx, nby, nh);
      const float nr_x = sx - nbx, nr_y = sy - nby, nr2 = nr_x * nr_x + nr_y * nr_y;
      if (conv) {  // the polishing step
        if (nr2 <= r2) { x = nx; y = ny; for (int k = 0; k < 4; ++k) h[k] = nh[k]; }
        ok = true;
        break;
      }
      x = nx; y = ny; r_x = nr_x; r_y = nr_y; r2 = nr2;
      for (int k = 0; k < 4; ++k) h[k] = nh[k];
    }
    mu = 1.f / ((1.f - h[0]) * (1.f - h[3]) - h[1] * h[2]);
    ok = ok && isfinite(x) && isfinite(y) && x >= g.x_lo && x <= g.x_hi && y >= g.y_lo && y <= g.y_hi;
    rx[lane] = x;
    ry[lane] = y;
    rmu[lane] = mu;
    rok[lane] = ok ? 1 : (straddles ? 2 : 0);
  }
  __syncthreads();
  if (lane == 0) {
    // merge: a converged candidate within IMG_MERGE cells of an image already kept (earlier in triangle order) is that image
    const float mx = IMG_MERGE * g.hx, my = IMG_MERGE * g.hy, m2 = mx * mx + my * my;
    int n_keep = 0, n_bad = 0;
    for (int i = 0; i < nc; ++i) {
      if (rok[i] != 1) { n_bad += rok[i] == 0; continue; }
      bool dup = false;
      for (int j = 0; j < n_keep && !dup; ++j) {
        const float dx = rx[i] - rx[order[j]], dy = ry[i] - ry[order[j]];
        dup = dx * dx + dy * dy < m2;
      }
      if (!dup) order[n_keep++] = i;
    }
    // sort by x, then y (insertion sort: at most IMG_MAXC entries)
    for (int i = 1; i < n_keep; ++i) {
      const int v = order[i];
      int j = i - 1;
      while (j >= 0 && (rx[order[j]] > rx[v] || (rx[order[j]] == rx[v] && ry[order[j]] > ry[v]))) { order[j + 1] = order[j]; --j; }
      order[j + 1] = v;
    }
    n_keep_s = n_keep;
    n_bad_s = n_bad;
  }
  __syncthreads();
  const int n_keep = n_keep_s, n_out = min(n_keep, g.max_images);
  if (lane == 0) {
    g.n_images[bs] = n_out;
    g.n_dropped[bs] = n_bad_s + g.n_over[bs] + (n_keep - n_out);
  }
  const float nan = __builtin_nanf("");
  for (int m = lane; m < g.max_images; m += 64) {
    float* o = g.out + ((size_t)bs * g.max_images + m) * 3;
    const int src = m < n_out ? order[m] : -1;
    o[0] = src >= 0 ? rx[src] : nan;
    o[1] = src >= 0 ? ry[src] : nan;
    o[2] = src >= 0 ? rmu[src] : nan;
  }
}
template <bool IM> __device__ __forceinline__ void img_newton_body(const PosArgs& a, const ImgArgs& g) {
  const int bs = blockIdx.x, b = bs / g.S;
  const float c = g.src_scale ? g.src_scale[bs - b * g.S] : 1.f;
  img_newton_core(g, ImgEvalScaled<IM>{a, b, c});
}
__global__ void __launch_bounds__(64) gl_img_newton_kernel(PosArgs a, ImgArgs g) { img_newton_body<false>(a, g); }
__global__ void __launch_bounds__(64) gl_img_newton_im_kernel(PosArgs a, ImgArgs g) { img_newton_body<true>(a, g); }

}  // namespace glk
