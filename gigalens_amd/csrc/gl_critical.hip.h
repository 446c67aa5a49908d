// gl_critical.hip.h -- critical curves, caustics and the area they enclose, for every sample of lens parameters
// (gl_critical_curves; LensSimulator.critical_curves / einstein_radius).  The reference has no such call.  The critical curves are
// the image-plane locus D = det(I - H) = (1 - f_xx)(1 - f_yy) - f_xy f_yx = 0, contoured by marching squares on a regular
// n x n grid of cells over a window with the point evaluation of beta and the Hessian the lens-equation solver uses
// (crit_eval below, on lens_jets of gl_positions.hip.h as img_lens_eval of gl_images.hip.h is, and built in two forms, see
// crit_eval_impl; built-in kinds and GL_SCALED catalogues).  Four launches, all
// on the caller's stream, no host synchronisation, no allocation:
//   map    (sample, vertex):   D at the (n+1)^2 vertices, ONE float per vertex, vertex fastest: the parameter row of a wave is
//                              one broadcast load and the plane of a sample is contiguous for the kernels below; a D that is
//                              not finite (a singular lens centre) is stored as NaN and flags its cells
//   scan   (sample):           one workgroup of CRIT_WG threads walks the 2 n (n+1) grid edges in index order (the (n+1) n
//                              horizontal ones row by row, then the n (n+1) vertical ones); an edge whose two finite endpoint
//                              values differ in sign (sign = D < 0) is crossing; the ids of the crossing edges are compacted per
//                              wave (ballot + mbcnt) and the waves' runs concatenated in wave order, i.e. the list is sorted by
//                              edge id.  Two passes over the plane (count, then write) instead of a wave-private LDS list, so
//                              the list length is not bounded by LDS.  A crossing edge on the window boundary sets `open`.
//   refine (sample, list slot): the root finder has its own launch over the compacted list, so every lane of a wave holds a
//                              crossing edge (a few hundred of the 1.3e5 edges cross: refining inside the scan would leave one
//                              lane in 64 spinning).  Bisection on the edge parameter t in [0, 1]: the signs at t = 0, 1 are the
//                              stored vertex signs, D at the midpoint comes from crit_eval.  It stops when the bracket
//                              (t_hi - t_lo) * (edge length) is at most CRIT_BRACKET_ULP float32 spacings of the window's largest
//                              |coordinate|, or after CRIT_MAX_BISECT halvings; the record is the bracket's midpoint (x, y), its
//                              beta and 1 - kappa there.  One record per EDGE: the two cells sharing it read the same bits.
//                              The grid is B x ceil(max_edges / 64) one-wave workgroups, sized by the capacity because the
//                              host does not know the list lengths (no synchronisation): a workgroup beyond its sample's
//                              list reads n_edges and exits (65 536 workgroups at the defaults, about 10 per sample refine).
//   cells  (sample):           one workgroup walks the n^2 cells row-major (wave w the w-th quarter, 64 consecutive cells per
//                              round).  Marching squares on the four vertex signs gives 0, 1 or 2 segments, endpoints looked up
//                              in the edge list by binary search on the edge id.  Segments are oriented with D < 0 on their left.
//                              The ambiguous cases (diagonal signs equal, neighbours different) join the D < 0 corners when the
//                              mean of the four vertex values is < 0 and separate them otherwise.  A segment is tangential
//                              (kind 0) when the mean of 1 - kappa at its two endpoints is > 0 (on D = 0 one eigenvalue
//                              1 - kappa -+ |gamma| vanishes; 1 - kappa = +|gamma| is the tangential one), else radial (1).
//                              Segments are compacted in cell order (per wave, then in wave order; count pass + write pass).
//                              A cell with a NaN vertex is skipped; it counts in n_flagged only when its finite vertices differ
//                              in sign (the centre of an SIS / SIE / EPL lies inside D < 0 and is no crossing).
// Per-sample sums, in a fixed order (lane partials in cell order, a fixed butterfly over the lanes, then the waves in order),
// in float64: the enclosed area  sum (x1 + x2) / 2 * (y2 - y1)  (Green, coordinates relative to the window centre) of the
// tangential and of the radial segments, and the same of their caustic (source-plane) images.  With D < 0 on the left a loop
// that encloses D < 0 counts positive, one that encloses D > 0 (a radial curve inside the tangential one) negative.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_images.hip.h"

namespace glk {

constexpr int CRIT_WG = 256;            // four waves per sample in scan and cells
constexpr int CRIT_MAX_BISECT = 32;     // cap on the halvings of one edge
constexpr float CRIT_BRACKET_ULP = 4.f;  // bracket width at which the bisection stops, in float32 spacings of max |window coordinate|

struct CritArgs {
  int n, max_segments, max_edges;  // cells per side; segment and crossing-edge capacity per sample
  float x_lo, x_hi, y_lo, y_hi;
  float hx, hy;       // cell sides
  float bracket;      // CRIT_BRACKET_ULP * eps * max |window coordinate|
  float scale;        // deflection scale c of the source plane the curves are drawn for: D = det(I - c H), beta = theta - c sum alpha
  float* dmap;        // [B][(n+1)^2] D at the vertices, row-major (y rows, x columns); NaN = flagged
  int* edge_id;       // [B][max_edges] crossing edges, ascending
  float4* edge_pt;    // [B][max_edges] x, y, beta_x, beta_y of the refined crossing
  float* edge_omk;    // [B][max_edges] 1 - kappa there
  int* n_edges;       // [B] entries of the list
  int* n_edge_over;   // [B] crossing edges beyond the list
  float* seg;         // [B][max_segments][2][2]
  float* cau;         // [B][max_segments][2][2]
  int* kind;          // [B][max_segments]
  int* n_seg;         // [B]
  int* n_dropped;     // [B]
  int* n_flagged;     // [B]
  int* open;          // [B]
  float* area;        // [B][4] tangential, radial (image plane), tangential, radial (source plane)
};

__device__ inline float crit_vx(const CritArgs& g, int c) { return g.x_lo + (float)c * g.hx; }
__device__ inline float crit_vy(const CritArgs& g, int r) { return g.y_lo + (float)r * g.hy; }

// D = det(I - H), beta and 1 - kappa of sample b at one point (H with the dPIS convergence excess).  CAT = false is the build for
// models without a GL_SCALED catalogue or a GL_INTERPOL_MASS lens: without their cases in the switch of lens_point the evaluation fits the 256 VGPRs
// inline; with it (CAT = true) it is a function call, which keeps the kernels free of register spills.
template <bool CAT>
__device__ inline float crit_eval_impl(const PosArgs& a, int b, float px, float py, float c, float& bx, float& by, float& omk) {
  bx = px;
  by = py;
  float h[4] = {0.f, 0.f, 0.f, 0.f};
  lens_jets<CAT>(
      a, b, px, py,
      [&](const CompDesc& cd, const float* pf, const Jet2& ax, const Jet2& ay, float ex) {
        bx -= ax.v;
        by -= ay.v;
        // exactly on an SIS centre D is not finite (the vertex is flagged), as beta is in gl_img_map_kernel
        h[0] += lens_singular_at(cd, pf, px, py) ? __builtin_nanf("") : ax.d[0] + ex;
        h[1] += ax.d[1]; h[2] += ay.d[0]; h[3] += ay.d[1] + ex;
      },
      [](const CompDesc& cd) { return !CAT && cd.kind == glp::K_SCALED; });  // (the host picks CAT = true for such a model)
  lens_rescale(c, px, py, bx, by, h);
  omk = 1.f - 0.5f * (h[0] + h[3]);
  return (1.f - h[0]) * (1.f - h[3]) - h[1] * h[2];
}

static __device__ __attribute__((noinline)) float crit_eval_cat(const PosArgs& a, int b, float px, float py, float c, float& bx, float& by, float& omk) {
  return crit_eval_impl<true>(a, b, px, py, c, bx, by, omk);
}
template <bool CAT>
__device__ inline float crit_eval(const PosArgs& a, int b, float px, float py, float c, float& bx, float& by, float& omk) {
  if constexpr (CAT) return crit_eval_cat(a, b, px, py, c, bx, by, omk);
  else return crit_eval_impl<false>(a, b, px, py, c, bx, by, omk);
}

template <bool CAT> __global__ void __launch_bounds__(256) gl_crit_map_kernel(PosArgs a, CritArgs g) {
  const int V1 = g.n + 1;
  const long long V = (long long)V1 * V1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= V * a.B) return;
  const int b = (int)(i / V), v = (int)(i - (long long)b * V);
  const int r = v / V1, c = v - r * V1;
  float bx, by, omk;
  float d = crit_eval<CAT>(a, b, crit_vx(g, c), crit_vy(g, r), g.scale, bx, by, omk);
  if (!isfinite(d)) d = __builtin_nanf("");
  g.dmap[i] = d;
}

// the two vertices of grid edge e: horizontal edges e < (n+1) n run from (r, c) to (r, c+1), vertical ones from (r, c) to (r+1, c)
__device__ inline void crit_edge_vertices(int n, int e, int& r, int& c, bool& horizontal) {
  const int H = (n + 1) * n;
  horizontal = e < H;
  if (horizontal) { r = e / n; c = e - r * n; }
  else { const int k = e - H; r = k / (n + 1); c = k - r * (n + 1); }
}

__device__ inline int crit_wave_rank(bool flag, unsigned long long& mask) {
  mask = __builtin_amdgcn_ballot_w64(flag);
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__global__ void __launch_bounds__(CRIT_WG) gl_crit_scan_kernel(CritArgs g) {
  constexpr int NW = CRIT_WG / 64;
  __shared__ int cnt[NW], bnd[NW];
  const int b = blockIdx.x, n = g.n, V1 = n + 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* dm = g.dmap + (size_t)b * (size_t)V1 * (size_t)V1;
  const int E = 2 * n * V1, per = (E + NW - 1) / NW;
  const int e0 = min(E, wave * per), e1 = min(E, e0 + per);
  int base_out = 0;
  for (int pass = 0; pass < 2; ++pass) {
    int count = 0, boundary = 0;
    for (int eb = e0; eb < e1; eb += 64) {
      const int e = eb + lane;
      bool cross = false, edge_of_window = false;
      if (e < e1) {
        int r, c;
        bool hz;
        crit_edge_vertices(n, e, r, c, hz);
        const float d0 = dm[r * V1 + c], d1 = dm[hz ? r * V1 + c + 1 : (r + 1) * V1 + c];
        cross = isfinite(d0) && isfinite(d1) && ((d0 < 0.f) != (d1 < 0.f));
        edge_of_window = hz ? (r == 0 || r == n) : (c == 0 || c == n);
      }
      unsigned long long m;
      const int rank = base_out + count + crit_wave_rank(cross, m);
      if (pass == 1 && cross && rank < g.max_edges) g.edge_id[(size_t)b * g.max_edges + rank] = e;
      count += __builtin_popcountll(m);
      boundary |= __builtin_amdgcn_ballot_w64(cross && edge_of_window) != 0ull;
    }
    if (pass == 1) break;
    if (lane == 0) { cnt[wave] = count; bnd[wave] = boundary; }
    __syncthreads();
    int total = 0, any = 0;
    for (int w = 0; w < NW; ++w) {
      if (w < wave) base_out += cnt[w];
      total += cnt[w];
      any |= bnd[w];
    }
    if (threadIdx.x == 0) {
      g.n_edges[b] = min(total, g.max_edges);
      g.n_edge_over[b] = total - min(total, g.max_edges);
      g.open[b] = any;
    }
  }
}

template <bool CAT> __global__ void __launch_bounds__(64) gl_crit_refine_kernel(PosArgs a, CritArgs g) {
  const int per_sample = (g.max_edges + 63) / 64;
  const int b = blockIdx.x / per_sample, k = (blockIdx.x - b * per_sample) * 64 + threadIdx.x;
  if (k >= g.n_edges[b]) return;
  const int n = g.n, V1 = n + 1;
  const int e = g.edge_id[(size_t)b * g.max_edges + k];
  int r, c;
  bool hz;
  crit_edge_vertices(n, e, r, c, hz);
  const float x0 = crit_vx(g, c), y0 = crit_vy(g, r);
  const float len = hz ? g.hx : g.hy;
  const bool neg0 = g.dmap[(size_t)b * (size_t)V1 * (size_t)V1 + (size_t)(r * V1 + c)] < 0.f;  // the sign at t = 0; t = 1 has the other
  float t_lo = 0.f, t_hi = 1.f, bx, by, omk;
  for (int it = 0; it < CRIT_MAX_BISECT && (t_hi - t_lo) * len > g.bracket; ++it) {
    const float t = 0.5f * (t_lo + t_hi);
    const float d = crit_eval<CAT>(a, b, hz ? x0 + t * len : x0, hz ? y0 : y0 + t * len, g.scale, bx, by, omk);
    if ((d < 0.f) == neg0) t_lo = t;
    else t_hi = t;
  }
  const float t = 0.5f * (t_lo + t_hi);
  const float x = hz ? x0 + t * len : x0, y = hz ? y0 : y0 + t * len;
  crit_eval<CAT>(a, b, x, y, g.scale, bx, by, omk);
  g.edge_pt[(size_t)b * g.max_edges + k] = float4{x, y, bx, by};
  g.edge_omk[(size_t)b * g.max_edges + k] = omk;
}

// Marching squares.  Corner bits (set when D < 0): 1 = (r, c), 2 = (r, c+1), 4 = (r+1, c+1), 8 = (r+1, c).  Cell edges:
// 0 = bottom (r, c)-(r, c+1), 1 = right (r, c+1)-(r+1, c+1), 2 = top (r+1, c)-(r+1, c+1), 3 = left (r, c)-(r+1, c).  A table
// entry from | to << 2 is one segment walked from edge `from` to edge `to` with the D < 0 corners on its left (x to the right,
// y upwards); 0xFF = none.  Rows 16 and 17 are cases 5 and 10 in the form that joins the two D < 0 corners (mean of the four
// values < 0); rows 5 and 10 separate them.
__device__ inline int crit_cell_segments(int code, bool join, int* from, int* to) {
  constexpr unsigned char NONE = 0xFF;
  constexpr unsigned char T[18][2] = {
      {NONE, NONE},           // 0
      {0 | 3 << 2, NONE},     // 1: bottom -> left
      {1 | 0 << 2, NONE},     // 2: right -> bottom
      {1 | 3 << 2, NONE},     // 3: right -> left
      {2 | 1 << 2, NONE},     // 4: top -> right
      {0 | 3 << 2, 2 | 1 << 2},  // 5 separated: cases 1 and 4
      {2 | 0 << 2, NONE},     // 6: top -> bottom
      {2 | 3 << 2, NONE},     // 7: top -> left
      {3 | 2 << 2, NONE},     // 8: left -> top
      {0 | 2 << 2, NONE},     // 9: bottom -> top
      {1 | 0 << 2, 3 | 2 << 2},  // 10 separated: cases 2 and 8
      {1 | 2 << 2, NONE},     // 11: right -> top
      {3 | 1 << 2, NONE},     // 12: left -> right
      {0 | 1 << 2, NONE},     // 13: bottom -> right
      {3 | 0 << 2, NONE},     // 14: left -> bottom
      {NONE, NONE},           // 15
      {0 | 1 << 2, 2 | 3 << 2},  // 5 joined: cases 13 and 7
      {3 | 0 << 2, 1 | 2 << 2},  // 10 joined: cases 14 and 11
  };
  const int row = join && code == 5 ? 16 : (join && code == 10 ? 17 : code);
  int ns = 0;
  for (int s = 0; s < 2; ++s)
    if (T[row][s] != NONE) { from[ns] = T[row][s] & 3; to[ns] = T[row][s] >> 2; ++ns; }
  return ns;
}

// vertex values of cell (r, c) -> number of segments (0 when a vertex is NaN; `flagged` then says whether the finite ones differ in sign)
__device__ inline int crit_classify(const float* dm, int V1, int r, int c, int* from, int* to, bool& flagged) {
  const float d[4] = {dm[r * V1 + c], dm[r * V1 + c + 1], dm[(r + 1) * V1 + c + 1], dm[(r + 1) * V1 + c]};
  int code = 0, n_fin = 0, n_neg = 0;
  for (int k = 0; k < 4; ++k) {
    const bool fin = isfinite(d[k]), neg = fin && d[k] < 0.f;
    code |= neg ? 1 << k : 0;
    n_fin += fin;
    n_neg += neg;
  }
  flagged = n_fin < 4 && n_neg > 0 && n_neg < n_fin;
  if (n_fin < 4) return 0;
  const bool join = 0.25f * (d[0] + d[1] + d[2] + d[3]) < 0.f;
  return crit_cell_segments(code, join, from, to);
}

// slot of edge e in the sample's ascending list, or -1
__device__ inline int crit_find_edge(const int* ids, int ne, int e) {
  int lo = 0, hi = ne;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < e) lo = mid + 1;
    else hi = mid;
  }
  return lo < ne && ids[lo] == e ? lo : -1;
}

__device__ inline double crit_wave_sum(double v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ inline int crit_wave_sum(int v) {
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

__global__ void __launch_bounds__(CRIT_WG) gl_crit_cells_kernel(CritArgs g) {
  constexpr int NW = CRIT_WG / 64;
  __shared__ int cnt[NW], flg[NW], drp[NW];
  __shared__ double acc[NW][4];
  const int b = blockIdx.x, n = g.n, V1 = n + 1, Hn = V1 * n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* dm = g.dmap + (size_t)b * (size_t)V1 * (size_t)V1;
  const int* ids = g.edge_id + (size_t)b * g.max_edges;
  const float4* pts = g.edge_pt + (size_t)b * g.max_edges;
  const float* omks = g.edge_omk + (size_t)b * g.max_edges;
  const int ne = g.n_edges[b];
  const int C = n * n, per = (C + NW - 1) / NW;
  const int c0 = min(C, wave * per), c1 = min(C, c0 + per);
  // pass 1: segments and flagged cells of this wave's cells
  {
    int count = 0, flagged_cells = 0;
    for (int cb = c0; cb < c1; cb += 64) {
      const int cell = cb + lane;
      int from[2], to[2], ns = 0;
      bool flagged = false;
      if (cell < c1) ns = crit_classify(dm, V1, cell / n, cell % n, from, to, flagged);
      count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(ns >= 1)) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(ns == 2));
      flagged_cells += __builtin_popcountll(__builtin_amdgcn_ballot_w64(flagged));
    }
    if (lane == 0) { cnt[wave] = count; flg[wave] = flagged_cells; }
  }
  __syncthreads();
  int base = 0, total = 0, n_flagged = 0;
  for (int w = 0; w < NW; ++w) {
    if (w < wave) base += cnt[w];
    total += cnt[w];
    n_flagged += flg[w];
  }
  // pass 2: the same walk, now writing every segment at its rank in cell order
  const float cx = 0.5f * (g.x_lo + g.x_hi);  // x of the window centre: the sums stay small
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int dropped = 0, count = 0;
  for (int cb = c0; cb < c1; cb += 64) {
    const int cell = cb + lane;
    const int r = cell / n, c = cell - r * n;
    int from[2], to[2], ns = 0;
    bool flagged = false;
    if (cell < c1) ns = crit_classify(dm, V1, r, c, from, to, flagged);
    unsigned long long m1, m2;
    const int rank = base + count + crit_wave_rank(ns >= 1, m1) + crit_wave_rank(ns == 2, m2);
    count += __builtin_popcountll(m1) + __builtin_popcountll(m2);
    for (int k = 0; k < ns; ++k) {
      const int slot = rank + k;
      if (slot >= g.max_segments) { ++dropped; continue; }
      const int cell_edge[4] = {r * n + c, Hn + r * V1 + c + 1, (r + 1) * n + c, Hn + r * V1 + c};
      const int i1 = crit_find_edge(ids, ne, cell_edge[from[k]]), i2 = crit_find_edge(ids, ne, cell_edge[to[k]]);
      float* so = g.seg + ((size_t)b * g.max_segments + slot) * 4;
      float* co = g.cau + ((size_t)b * g.max_segments + slot) * 4;
      if (i1 < 0 || i2 < 0) {  // an endpoint beyond the edge list: the slot is padding and the segment counts as dropped
        const float nan = __builtin_nanf("");
        for (int q = 0; q < 4; ++q) so[q] = co[q] = nan;
        g.kind[(size_t)b * g.max_segments + slot] = -1;
        ++dropped;
        continue;
      }
      const float4 p1 = pts[i1], p2 = pts[i2];
      const int kind = omks[i1] + omks[i2] > 0.f ? 0 : 1;
      so[0] = p1.x; so[1] = p1.y; so[2] = p2.x; so[3] = p2.y;
      co[0] = p1.z; co[1] = p1.w; co[2] = p2.z; co[3] = p2.w;
      g.kind[(size_t)b * g.max_segments + slot] = kind;
      s[kind] += 0.5 * ((double)(p1.x - cx) + (double)(p2.x - cx)) * ((double)p2.y - (double)p1.y);
      s[2 + kind] += 0.5 * ((double)(p1.z - cx) + (double)(p2.z - cx)) * ((double)p2.w - (double)p1.w);
    }
  }
  for (int q = 0; q < 4; ++q) s[q] = crit_wave_sum(s[q]);
  dropped = crit_wave_sum(dropped);
  if (lane == 0) {
    for (int q = 0; q < 4; ++q) acc[wave][q] = s[q];
    drp[wave] = dropped;
  }
  __syncthreads();
  const int n_out = min(total, g.max_segments);
  if (threadIdx.x == 0) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    int nd = 0;
    for (int w = 0; w < NW; ++w) {
      for (int q = 0; q < 4; ++q) t[q] += acc[w][q];
      nd += drp[w];
    }
    for (int q = 0; q < 4; ++q) g.area[(size_t)b * 4 + q] = (float)t[q];
    g.n_seg[b] = n_out;
    g.n_dropped[b] = nd;
    g.n_flagged[b] = n_flagged;
  }
  const float nan = __builtin_nanf("");
  for (int k = n_out + (int)threadIdx.x; k < g.max_segments; k += CRIT_WG) {
    float* so = g.seg + ((size_t)b * g.max_segments + k) * 4;
    float* co = g.cau + ((size_t)b * g.max_segments + k) * 4;
    for (int q = 0; q < 4; ++q) so[q] = co[q] = nan;
    g.kind[(size_t)b * g.max_segments + k] = -1;
  }
}

}  // namespace glk
