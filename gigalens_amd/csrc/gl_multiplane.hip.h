// gl_multiplane.hip.h -- multi-plane ray tracing: lenses on up to MP_MAXK planes at redshifts of their own (beyond the reference,
// which bends every ray at one plane).  gl_model_set_lens_planes attaches the planes; the two kernels below serve such a model.
//
// Planes are numbered by ascending redshift.  Every lens keeps its parameters as the reduced deflection for the model's
// reference plane; plane i acts on plane j > i with the coupling C_ij = [D_ij / D_j] / [D_i,ref / D_ref] (cosmology.MultiPlane):
//   theta_j = theta - sum_{i<j} C_ij a_i,    a_i = sum_{lenses l on plane i} alpha_l(theta_i),    theta_0 = theta
//   beta_t  = theta - sum_i T_i a_i          (T: the couplings of a target -- a source light, an arbitrary plane; 0 for the
//                                             planes at or behind it),        A_t = d beta_t / d theta
// With one plane this is beta = theta - c sum alpha, what the single-plane kernels compute.
//
// The recursion (mp_trace) is generic in the number type: on Dual<float, 2> seeded with d theta / d theta = I it carries
// d theta_j / d theta through every plane, so the per-plane sums hold d a_i / d theta and A_t -- not symmetric once two planes are
// offset -- is their combination; on float it is the ray shooting of the render kernel.  Lenses are visited in plane order (the
// host's stable sort of plane_of_lens), so a_i is complete when the first lens of plane i + 1 asks for theta_{i+1}.  The per-plane
// sums never live in a runtime-indexed private array (MpRegSums, MpLdsSums below): nothing of them goes to scratch.
//   maps    (point, sample):                out[6][n_pts][B] = beta_x, beta_y, f_xx, f_xy, f_yx, f_yy with f = I - A_t, the
//                                           layout of gl_lens_maps (f_xy != f_yx here); dPIS lenses add their convergence excess
//                                           to the diagonal of their own Hessian, as gl_lens_maps_kernel does
//   render  (supersampled pixel, sample):   lens lights at theta, source s at beta_s, NaN -> 0, x out_scale, written to the
//                                           supersampled frame (pix_region: the listed pixels; the host clears the rest).  The
//                                           model's own PSF + pooling launch (post_fwd) follows, as after the single-plane render.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "gl_dual.h"
#include "gl_kernels.hip.h"
#include "gl_positions.hip.h"

namespace glk {

constexpr int MP_MAXK = 4;  // lens planes served
constexpr int MP_WG = 256;

struct MpArgs {
  const int* order;    // [n_lens] lenses sorted by plane (stable)
  const int* plane;    // [n_lens] plane of every lens
  const float* scale;  // [MP_MAXK][MP_MAXK] C_ij (strictly upper triangular, zero-padded), then [MP_MAXK][n_src] source couplings
};
struct MpTarget { float c[MP_MAXK]; };  // couplings of one target plane, zero-padded

struct MpRender {
  const float* gx;  // [N] supersampled pixel positions
  const float* gy;
  const int* pix;   // [N] index of a listed pixel in the supersampled frame, or null: the whole frame
  int N, n_ll, n_src;
  unsigned parts;   // 1 deflect the sources, 2 lens light, 4 source light (gl_simulate_parts_fwd)
  float out_scale;
  long long img_stride;
  float* img;       // [B][Hs Ws]
};

__device__ __forceinline__ float mp_value(float x) { return x; }
__device__ __forceinline__ float mp_value(const gld::Dual<float, 2>& x) { return x.v; }
// the dPIS convergence excess e of one lens: its Hessian is d alpha / d theta_j + e I, so d a / d theta gains e d theta_j / d theta
__device__ __forceinline__ void mp_add_excess(float&, float&, float, float, float) {}
__device__ __forceinline__ void mp_add_excess(gld::Dual<float, 2>& ax, gld::Dual<float, 2>& ay, const gld::Dual<float, 2>& x,
                                              const gld::Dual<float, 2>& y, float e) {
  ax.d[0] += e * x.d[0]; ax.d[1] += e * x.d[1];
  ay.d[0] += e * y.d[0]; ay.d[1] += e * y.d[1];
}

// Where the per-plane sums a_i live.  On float (render kernel) they are eight registers: arrays that only unrolled loops with
// constant indices touch, the plane of a lens selecting by comparison -- no private memory.  On Dual<float, 2> (maps kernel) they
// are 24 floats that stay live across the largest lens template and would push it over the register file, so each thread parks
// them in a column of LDS of its own (entry e of thread t at lds[e][t]: conflict-free, no barrier, and indexable by the plane).
struct MpRegSums {
  float x[MP_MAXK], y[MP_MAXK];
  __device__ __forceinline__ MpRegSums() {
#pragma unroll
    for (int i = 0; i < MP_MAXK; ++i) { x[i] = 0.f; y[i] = 0.f; }
  }
  // theta_pl = theta - sum_{i<pl} C[i][pl] a_i (the planes at and behind pl do not enter, whatever their sums hold)
  __device__ __forceinline__ void to_plane(int pl, const float* __restrict__ scale, float& px, float& py) const {
#pragma unroll
    for (int i = 0; i < MP_MAXK - 1; ++i)
      if (i < pl) {
        const float c = scale[i * MP_MAXK + pl];
        px -= c * x[i];
        py -= c * y[i];
      }
  }
  __device__ __forceinline__ void add(int pl, float ax, float ay) {
#pragma unroll
    for (int i = 0; i < MP_MAXK; ++i)
      if (i == pl) { x[i] += ax; y[i] += ay; }
  }
};

constexpr int MP_MAPS_WG = 64;
struct MpLdsSums {
  using R = gld::Dual<float, 2>;
  float* col;  // this thread's column: a_i = (x.v, x.d0, x.d1, y.v, y.d0, y.d1) at col[(6 i + e) MP_MAPS_WG]
  __device__ __forceinline__ explicit MpLdsSums(float* c) : col(c) {
    for (int e = 0; e < 6 * MP_MAXK; ++e) col[e * MP_MAPS_WG] = 0.f;
  }
  __device__ __forceinline__ float at(int i, int e) const { return col[(6 * i + e) * MP_MAPS_WG]; }
  __device__ __forceinline__ void to_plane(int pl, const float* __restrict__ scale, R& px, R& py) const {
    for (int i = 0; i < pl; ++i) {
      const float c = scale[i * MP_MAXK + pl];
      px.v -= c * at(i, 0); px.d[0] -= c * at(i, 1); px.d[1] -= c * at(i, 2);
      py.v -= c * at(i, 3); py.d[0] -= c * at(i, 4); py.d[1] -= c * at(i, 5);
    }
  }
  __device__ __forceinline__ void add(int pl, const R& ax, const R& ay) {
    float* q = col + 6 * pl * MP_MAPS_WG;
    q[0] += ax.v; q[MP_MAPS_WG] += ax.d[0]; q[2 * MP_MAPS_WG] += ax.d[1];
    q[3 * MP_MAPS_WG] += ay.v; q[4 * MP_MAPS_WG] += ay.d[0]; q[5 * MP_MAPS_WG] += ay.d[1];
  }
};

// mp_trace's `skip` of the callers that evaluate every lens wherever the ray meets its plane
struct MpSkipNone {
  __device__ __forceinline__ bool operator()(const CompDesc&, const float*, float, float) const { return false; }
};

// the plane recursion for sample b of a.params from (tx, ty): on return `sums` holds every a_i (zero for the planes the model lacks).
// CATS: lens_point's (no model with planes holds a catalogue; false leaves the catalogue loop out of the kernel)
// skip(cd, raw parameters, x_j, y_j) == true: the lens is not evaluated at the ray's position on its plane and its plane sum becomes
// NaN (the lens-equation solver on planes, gl_multiplane_images.hip.h: a singular centre, a ray that is not finite)
template <class R, bool CATS = true, class Sums, class Skip = MpSkipNone>
__device__ __forceinline__ void mp_trace(const PosArgs& a, const MpArgs& mp, int b, const R& tx, const R& ty, Sums& sums,
                                         const Skip& skip = Skip()) {
  for (int t = 0; t < a.n_lens; ++t) {
    const int l = mp.order[t], pl = mp.plane[l];
    const CompDesc cd = a.comps[l];
    R x = tx, y = ty;
    sums.to_plane(pl, mp.scale, x, y);
    R p[POS_MAXP];
    float pf[POS_MAXP];
#pragma unroll
    for (int k = 0; k < POS_MAXP; ++k) {
      pf[k] = k < cd.n_par ? a.params[(size_t)b * a.P + cd.p_off + k] : 0.f;
      p[k] = R(pf[k]);
    }
    R ax, ay;
    if (skip(cd, pf, mp_value(x), mp_value(y))) {
      ax = ay = R(__builtin_nanf(""));
    } else {
      lens_point<R, CATS>(a, cd, p, x, y, ax, ay);
      if constexpr (!std::is_same<R, float>::value)
        mp_add_excess(ax, ay, x, y, lens_kappa_excess<float>(a, cd, pf, mp_value(x), mp_value(y)));
    }
    sums.add(pl, ax, ay);
  }
}

__global__ void __launch_bounds__(MP_MAPS_WG) gl_mp_maps_kernel(PosArgs a, MpArgs mp, MpTarget tg, const float* __restrict__ x,
                                                               const float* __restrict__ y, long long n_pts, int xy_batched,
                                                               float* __restrict__ out) {
  __shared__ float lds[6 * MP_MAXK][MP_MAPS_WG];
  const long long i = (long long)blockIdx.x * MP_MAPS_WG + threadIdx.x;
  if (i >= n_pts * a.B) return;
  const PointAt at(i, a.B, xy_batched, x, y);
  using R = gld::Dual<float, 2>;
  R xd(at.x), yd(at.y);
  xd.d[0] = 1.f;
  yd.d[1] = 1.f;
  MpLdsSums sums(&lds[0][threadIdx.x]);
  mp_trace<R>(a, mp, at.b, xd, yd, sums);
  float bx = at.x, by = at.y, fxx = 0.f, fxy = 0.f, fyx = 0.f, fyy = 0.f;
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k) {
    const float c = tg.c[k];
    if (c != 0.f) {  // (a plane at or behind the target: not part of its ray, even where its own sum is not finite)
      bx -= c * sums.at(k, 0); by -= c * sums.at(k, 3);
      fxx += c * sums.at(k, 1); fxy += c * sums.at(k, 2); fyx += c * sums.at(k, 4); fyy += c * sums.at(k, 5);
    }
  }
  const long long st = n_pts * a.B;
  out[i] = bx; out[st + i] = by; out[2 * st + i] = fxx; out[3 * st + i] = fxy; out[4 * st + i] = fyx; out[5 * st + i] = fyy;
}

// one light component at (x, y) from its raw parameters: the per-kind templates gl_point_kernel evaluates
__device__ __forceinline__ float mp_light(const CompDesc& cd, const float* __restrict__ p, float x, float y) {
  using namespace glp;
  switch (cd.kind) {
    case K_SERSIC: { float d[SER_NDX]; sersic_prep<float>(p, false, d); return sersic_fwd(d, x, y); }
    case K_SERSIC_ELLIPSE: { float d[SER_NDX]; sersic_prep<float>(p, true, d); return sersic_fwd(d, x, y); }
    case K_CORE_SERSIC: { float d[CSR_ND]; core_sersic_prep<float>(p, d); return core_sersic_fwd<float>(d, x, y); }
    default: return __builtin_nanf("");  // (not reached: gl_model_set_lens_planes refuses every other light kind)
  }
}

__global__ void __launch_bounds__(MP_WG) gl_mp_render_kernel(PosArgs a, MpArgs mp, MpRender r) {
  const int n = blockIdx.x * MP_WG + threadIdx.x, b = blockIdx.y;
  if (n >= r.N) return;
  const float tx = r.gx[n], ty = r.gy[n];
  const bool src = (r.parts & 4u) && r.n_src > 0, deflect = src && (r.parts & 1u);
  MpRegSums sums;
  if (deflect) mp_trace<float>(a, mp, b, tx, ty, sums);
  const float* row = a.params + (size_t)b * a.P;
  float v = 0.f;
  if (r.parts & 2u)
    for (int i = 0; i < r.n_ll; ++i) {
      const CompDesc cd = a.comps[a.n_lens + i];
      v += mp_light(cd, row + cd.p_off, tx, ty);
    }
  if (src)
    for (int s = 0; s < r.n_src; ++s) {
      const CompDesc cd = a.comps[a.n_lens + r.n_ll + s];
      float bx = tx, by = ty;
      if (deflect) {
#pragma unroll
        for (int k = 0; k < MP_MAXK; ++k) {
          const float c = mp.scale[MP_MAXK * MP_MAXK + k * r.n_src + s];
          if (c != 0.f) { bx -= c * sums.x[k]; by -= c * sums.y[k]; }
        }
      }
      v += mp_light(cd, row + cd.p_off, bx, by);
    }
  v = (isnan_(v) ? 0.f : v) * r.out_scale;
  r.img[(size_t)b * r.img_stride + (r.pix ? r.pix[n] : n)] = v;
}

}  // namespace glk
