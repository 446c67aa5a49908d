// gl_multiplane_pos.hip.h -- the image-position likelihood (gl_positions.hip.h) on lens planes (gl_multiplane.hip.h): family f sits at
// a redshift of its own, and its images are traced back through the planes in front of it,
//   beta = theta - sum_i T_f,i a_i ,   A = d beta / d theta ,   theta_j = theta - sum_{i<j} C_ij a_i
// (T_f: the couplings of the family's plane, 0 for the planes at or behind it; gl_model_set_position_targets).  The likelihood is
// the single-plane one -- err = sigma det A, chi^2 against the family's mean beta, the log(2 pi err^2) norm -- so of its four
// kernels only the two that evaluate lenses differ:
//   P1  (sample, image):                   mp_trace on Dual<float, 2> with the per-thread LDS columns of the maps kernel, combined
//                                          with the couplings of the image's family -> w_pos = beta, f = I - A (not symmetric)
//   P2  gl_pos_p2_kernel, unchanged        statistics and the adjoints d ll / d (beta, det A)
//   P3  (sample, image, lens parameter):   the recursion on Dual<Dual<float, 1>, 2> with that one parameter seeded: theta_j, a_j and
//                                          d theta_j / d theta of every plane behind the owning lens's carry the parameter direction,
//                                          the dPIS excess is evaluated with it in the parameters AND in theta_j, and
//                                          g = adj_bx d beta_x + adj_by d beta_y + adj_det d det A from the traced A
//   P4  gl_pos_p4_kernel, unchanged        sums over the images
// No atomics; every output element is written by one thread from a fixed order of operations: two calls give identical bits.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_dual.h"
#include "gl_kernels.hip.h"
#include "gl_multiplane.hip.h"
#include "gl_positions.hip.h"

// the number type P3 runs the lens templates on: the TNFW's fp64 core as a call (gl_extra.h)
template <> struct glp::TnfwCoreOutlined<gld::Dual<gld::Dual<float, 1>, 1>> { static constexpr bool value = true; };

namespace glk {

constexpr int MP_POS_WG = 64;

// the last plane in front of the family (the largest i with T_i != 0), or -1: nothing behind it is part of the family's rays
__device__ __forceinline__ int mp_pos_last_plane(const float* __restrict__ T) {
  int last = -1;
#pragma unroll
  for (int i = 0; i < MP_MAXK; ++i)
    if (T[i] != 0.f) last = i;
  return last;
}

// `tg` [J][MP_MAXK]: the couplings of every image's family, zero-padded
__global__ void __launch_bounds__(MP_POS_WG) gl_mp_pos_p1_kernel(PosArgs a, MpArgs mp, const float* __restrict__ tg) {
  static_assert(MP_POS_WG == MP_MAPS_WG, "MpLdsSums strides its columns by the workgroup of the maps kernel");
  __shared__ float lds[6 * MP_MAXK][MP_POS_WG];
  const int i = blockIdx.x * MP_POS_WG + threadIdx.x;
  if (i >= a.B * a.J) return;
  const int b = i / a.J, j = i - b * a.J;
  const float px = a.px[j], py = a.py[j];
  using R = gld::Dual<float, 2>;
  R xd(px), yd(py);
  xd.d[0] = 1.f;
  yd.d[1] = 1.f;
  MpLdsSums sums(&lds[0][threadIdx.x]);
  mp_trace<R, false>(a, mp, b, xd, yd, sums);
  const float* T = tg + (size_t)j * MP_MAXK;
  float bx = px, by = py, fxx = 0.f, fxy = 0.f, fyx = 0.f, fyy = 0.f;
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k) {
    const float c = T[k];
    if (c != 0.f) {  // (a plane at or behind the family: not part of its rays, even where its own sum is not finite)
      bx -= c * sums.at(k, 0); by -= c * sums.at(k, 3);
      fxx += c * sums.at(k, 1); fxy += c * sums.at(k, 2); fyx += c * sums.at(k, 4); fyy += c * sums.at(k, 5);
    }
  }
  float* o = a.w_pos + (size_t)i * 6;
  o[0] = bx; o[1] = by; o[2] = fxx; o[3] = fxy; o[4] = fyx; o[5] = fyy;
}

// The per-plane sums of P3: a_i = (a_x, a_y) on Dual<Dual<float, 1>, 2> is 12 floats -- of each component v.v, v.d, d0.v, d0.d, d1.v,
// d1.d -- and 48 for the four planes.  They stay live across the largest lens template on nested duals, so each thread keeps them in
// a column of LDS of its own, as MpLdsSums does (entry e of thread t at lds[e][t]: conflict-free, no barrier, indexable by the plane).
struct MpLdsSums2 {
  using R1 = gld::Dual<float, 1>;
  using R = gld::Dual<R1, 2>;
  float* col;
  __device__ __forceinline__ explicit MpLdsSums2(float* c) : col(c) {
    for (int e = 0; e < 12 * MP_MAXK; ++e) col[e * MP_POS_WG] = 0.f;
  }
  __device__ __forceinline__ float at(int i, int e) const { return col[(12 * i + e) * MP_POS_WG]; }
  __device__ __forceinline__ static void sub(R& p, float c, const float* __restrict__ q) {
    p.v.v -= c * q[0]; p.v.d[0] -= c * q[MP_POS_WG];
    p.d[0].v -= c * q[2 * MP_POS_WG]; p.d[0].d[0] -= c * q[3 * MP_POS_WG];
    p.d[1].v -= c * q[4 * MP_POS_WG]; p.d[1].d[0] -= c * q[5 * MP_POS_WG];
  }
  __device__ __forceinline__ void to_plane(int pl, const float* __restrict__ scale, R& px, R& py) const {
    for (int i = 0; i < pl; ++i) {
      const float c = scale[i * MP_MAXK + pl];
      const float* q = col + 12 * i * MP_POS_WG;
      sub(px, c, q);
      sub(py, c, q + 6 * MP_POS_WG);
    }
  }
  __device__ __forceinline__ static void acc(float* q, const R& v) {
    q[0] += v.v.v; q[MP_POS_WG] += v.v.d[0];
    q[2 * MP_POS_WG] += v.d[0].v; q[3 * MP_POS_WG] += v.d[0].d[0];
    q[4 * MP_POS_WG] += v.d[1].v; q[5 * MP_POS_WG] += v.d[1].d[0];
  }
  __device__ __forceinline__ void add(int pl, const R& ax, const R& ay) {
    float* q = col + 12 * pl * MP_POS_WG;
    acc(q, ax);
    acc(q + 6 * MP_POS_WG, ay);
  }
};

// the dPIS convergence excess of one lens at a position that carries the parameter direction (lens_kappa_excess takes it as float,
// which is the whole of it only on the first plane); zero for every other kind served on lens planes
template <class R1> __device__ __forceinline__ R1 mp_pos_kappa_excess(const CompDesc& cd, const R1* p, const R1& x, const R1& y) {
  using namespace glp;
  if (cd.kind != K_DPIS) return R1(0.f);
  R1 d[DPX_ND];
  dpie_prep<R1>(cd.kind, p, d);
  return dpis_kappa_excess<R1>(d, d + DP_NS, x, y);
}

// theta_pl of image j with d theta / d theta = I seeded, from the sums of the planes in front of pl
__device__ __forceinline__ void mp_pos_theta(const PosArgs& a, const MpArgs& mp, const MpLdsSums2& sums, int j, int pl, MpLdsSums2::R& x,
                                             MpLdsSums2::R& y) {
  using R1 = MpLdsSums2::R1;
  x = MpLdsSums2::R(R1(a.px[j]));
  y = MpLdsSums2::R(R1(a.py[j]));
  x.d[0] = R1(1.f);
  y.d[1] = R1(1.f);
  sums.to_plane(pl, mp.scale, x, y);
}
// parameter m of lens cd in sample b, carrying the direction when it is the thread's column (m == k)
__device__ __forceinline__ gld::Dual<float, 1> mp_pos_param(const PosArgs& a, const CompDesc& cd, int b, int m, int k) {
  gld::Dual<float, 1> v(m < cd.n_par ? a.params[(size_t)b * a.P + cd.p_off + m] : 0.f);
  if (m == k) v.d[0] = 1.f;
  return v;
}

// What a thread of P3 knows about itself -- sample, image, owning lens, parameter within it, last plane in front of the family --
// is parked in five more entries of its LDS column and read back where it is used, and every pass over a lens adds what it found
// to the sums at once: nothing but the loop counters is live in registers across the lens templates, which fill the register file
// on their own.  The fp64 core of the TNFW is a call (TnfwCoreOutlined above): inlined in this loop its fp64 constants are
// hoisted out of it and the kernel spills.
constexpr int MP_POS_ROWS = 12 * MP_MAXK + 5;
enum { MPP_B = 12 * MP_MAXK, MPP_J, MPP_OWN, MPP_K, MPP_LAST };

__global__ void __launch_bounds__(MP_POS_WG) gl_mp_pos_p3_kernel(PosArgs a, MpArgs mp, const float* __restrict__ tg, int lens_params) {
  __shared__ float lds[MP_POS_ROWS][MP_POS_WG];
  const int i = blockIdx.x * MP_POS_WG + threadIdx.x;
  if (i >= a.B * a.J * lens_params) return;
  float* mine = &lds[0][threadIdx.x];
  // (volatile: read where it is used, not once before the loop and kept)
  auto geti = [&](int e) { return __float_as_int(((const volatile float*)mine)[e * MP_POS_WG]); };
  {
    const int col = i % lens_params, bj = i / lens_params;
    const int b = bj / a.J, j = bj - b * a.J;
    const int own = lens_of_column(a, col);
    const int last = mp_pos_last_plane(tg + (size_t)j * MP_MAXK);
    if (mp.plane[own] > last) {  // the column's plane lies at or behind the family: its rays never meet the lens
      a.w_g[((size_t)b * a.J + j) * a.P + col] = 0.f;
      return;
    }
    mine[MPP_B * MP_POS_WG] = __int_as_float(b);
    mine[MPP_J * MP_POS_WG] = __int_as_float(j);
    mine[MPP_OWN * MP_POS_WG] = __int_as_float(own);
    mine[MPP_K * MP_POS_WG] = __int_as_float(col - a.comps[own].p_off);
    mine[MPP_LAST * MP_POS_WG] = __int_as_float(last);
  }
  using R1 = gld::Dual<float, 1>;
  using R = gld::Dual<R1, 2>;
  using Q = gld::Dual<R1, 1>;
  MpLdsSums2 sums(mine);
  for (int t = 0; t < a.n_lens; ++t) {
    const int l = mp.order[t], pl = mp.plane[l];
    if (pl > geti(MPP_LAST)) break;  // (lenses come in plane order: everything from here on lies at or behind the family)
    const CompDesc cd = a.comps[l];
    // The lens at theta_j.  The outer dual parts of a result are linear in those of the position, ax.d[n] = H_xx x.d[n] + H_xy y.d[n]
    // in R1 arithmetic, so the templates need not carry d theta_j / d theta: they run on the VALUE of theta_j with its parameter
    // direction and a unit seed, one image-plane direction per pass (Dual<R1, 1>: four floats a value, not six), and give alpha
    // and the column H_., dir = d alpha / d theta_j,dir, each with its total parameter derivative (through the lens's own
    // parameters and through theta_j).  d theta_j / d theta is applied after them, from the sums of the planes in front (which
    // this lens does not change: theta_j is formed again rather than kept).
#pragma nounroll
    for (int dir = 0; dir < 2; ++dir) {
      Q qx, qy;
      {
        const int b = geti(MPP_B), j = geti(MPP_J), k = l == geti(MPP_OWN) ? geti(MPP_K) : -1;
        R x, y;
        mp_pos_theta(a, mp, sums, j, pl, x, y);
        Q xs(x.v), ys(y.v);
        xs.d[0] = R1(dir == 0 ? 1.f : 0.f);
        ys.d[0] = R1(dir == 0 ? 0.f : 1.f);
        Q p[POS_MAXP];
#pragma unroll
        for (int m = 0; m < POS_MAXP; ++m) p[m] = Q(mp_pos_param(a, cd, b, m, k));
        [[clang::always_inline]] lens_point<Q, false, false, false>(a, cd, p, xs, ys, qx, qy);  // (without the multipole: with it P3 spills; the host refuses)
      }
      const int j = geti(MPP_J);
      R x, y;
      mp_pos_theta(a, mp, sums, j, pl, x, y);
      R ax, ay;
      if (dir == 0) {
        ax.v = qx.v;
        ay.v = qy.v;
        ax.d[0] = qx.d[0] * x.d[0]; ax.d[1] = qx.d[0] * x.d[1];
        ay.d[0] = qy.d[0] * x.d[0]; ay.d[1] = qy.d[0] * x.d[1];
        if (cd.kind == glp::K_DPIS) {
          // the dPIS Hessian is d alpha / d theta_j + e I, e with the parameter direction in the parameters and in theta_j
          const int b = geti(MPP_B), k = l == geti(MPP_OWN) ? geti(MPP_K) : -1;
          R1 p1[POS_MAXP];
#pragma unroll
          for (int m = 0; m < POS_MAXP; ++m) p1[m] = mp_pos_param(a, cd, b, m, k);
          const R1 e = mp_pos_kappa_excess<R1>(cd, p1, x.v, y.v);
          ax.d[0] += e * x.d[0]; ax.d[1] += e * x.d[1];
          ay.d[0] += e * y.d[0]; ay.d[1] += e * y.d[1];
        }
      } else {
        ax.d[0] = qx.d[0] * y.d[0]; ax.d[1] = qx.d[0] * y.d[1];
        ay.d[0] = qy.d[0] * y.d[0]; ay.d[1] = qy.d[0] * y.d[1];
      }
      sums.add(pl, ax, ay);
    }
  }
  const int b = geti(MPP_B), j = geti(MPP_J);
  // beta = theta - sum T a ;  A = I - sum T d a / d theta ;  det A = A_xx A_yy - A_xy A_yx -- values and parameter derivatives
  const float* T = tg + (size_t)j * MP_MAXK;
  float dbx = 0.f, dby = 0.f, axx = 1.f, axy = 0.f, ayx = 0.f, ayy = 1.f, daxx = 0.f, daxy = 0.f, dayx = 0.f, dayy = 0.f;
#pragma unroll
  for (int n = 0; n < MP_MAXK; ++n) {
    const float c = T[n];
    if (c != 0.f) {
      dbx -= c * sums.at(n, 1); dby -= c * sums.at(n, 7);
      axx -= c * sums.at(n, 2); daxx -= c * sums.at(n, 3);
      axy -= c * sums.at(n, 4); daxy -= c * sums.at(n, 5);
      ayx -= c * sums.at(n, 8); dayx -= c * sums.at(n, 9);
      ayy -= c * sums.at(n, 10); dayy -= c * sums.at(n, 11);
    }
  }
  const float* adj = a.w_adj + ((size_t)b * a.J + j) * 3;
  const float ddet = daxx * ayy + axx * dayy - daxy * ayx - axy * dayx;
  a.w_g[((size_t)b * a.J + j) * a.P + a.comps[geti(MPP_OWN)].p_off + geti(MPP_K)] = adj[0] * dbx + adj[1] * dby + adj[2] * ddet;
}

}  // namespace glk
