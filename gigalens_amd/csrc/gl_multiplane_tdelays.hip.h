// gl_multiplane_tdelays.hip.h -- the time-delay likelihood of the image families (gl_tdelays.hip.h) on lens planes
// (gl_multiplane_pos.hip.h).  Family f sits at z_f behind the planes 0 .. K_f - 1; its observed images theta_j are traced as the
// position likelihood on planes traces them, beta_j = theta_j - sum_i T_f,i a_i(theta_j,i), and its source is the barycentre
// mean beta over ALL its images.  With the weights (g_f [K], v [K]) of MultiPlane.delay_weights(z_f) (gl_mp_delay.h),
//   phi_j = T(theta_j; mean beta) = sum_{i<K_f} [ g_f,i |theta_j,i - theta_j,next(i)|^2 / 2 - v_i psi_i(theta_j,i) ],
//   theta_j,next(K_f - 1) = mean beta                                                              (arcsec^2 c / H0)
// and everything after phi_j is the single-plane term: w = 1 / s^2 over the measured images, the w-weighted means, lambda_f given
// or sum w t~ phi~ / sum w phi~^2, chi2_f = sum w (t~ - lambda_f phi~)^2, ll_f = -1/2 (chi2_f + sum log(2 pi s^2)), T_f = t_bar -
// lambda_f phi_bar.  lambda_f is in days per (arcsec^2 c / H0): c / H0 [Mpc] x DAYS_PER_MPC_ARCSEC2 -- profiled, it is H0.
//
// The gradient is the partial derivative at fixed (lambda_f, T_f).  With a_j = lambda_f w_j (t~_j - lambda_f phi~_j):
//   through the source   d ll / d mean beta = -sum a_j g_f,last (theta_j,last - mean beta), 1 / n_f of it into the beta adjoint of
//                        every image of the family, which gl_mp_pos_p3_kernel carries; nothing into the det A adjoint;
//   direct part          d ll / d p = sum a_j d T(theta_j; mean beta) / d p at fixed mean beta.  Not -d psi / d p alone: the ray
//                        positions theta_j,i on the planes behind the owning lens move with p, and the observed theta_j are not
//                        stationary points of T.  Forward mode through the plane recursion with the one parameter seeded.
//
// Three kernels in the plane branch of run_positions -- P1, P2, flux, TRACE, STATS, P3, GRAD, P4:
//   gl_mp_pos_tdelay_trace_kernel  (sample, image): the ray on double with MpDelayState and the lens loop of gl_mp_fermat_kernel
//                                  (tdelay_trace_wide of gl_tdelays.hip.h: why double).  Five doubles per image: beta_j (on the
//                                  float32 couplings of the family, as P1 uses them), theta_j,last and T0_j = T without its last
//                                  geometric summand -- the only part that sees mean beta, so no thread traces a family twice and
//                                  none evaluates the lenses for several images in turn.
//   gl_mp_pos_tdelay_kernel        (sample, family), the thread that owns the family's w_fam / w_adj elements in P2 and in the
//                                  flux kernel; the `accumulate` rule of gl_pos_tdelay_kernel.  No lens: mean beta, phi_j = T0_j +
//                                  g_last |theta_j,last - mean beta|^2 / 2 and the sums in a fixed order in double.
//   gl_mp_pos_tdelay_grad_kernel   (sample, image, lens-parameter column), after P3 and before P4: a_j == 0 exactly or a lens at
//                                  or behind the family: nothing is touched; else the recursion and `arrival` on Dual<double, 1>
//                                  with the column seeded, a_j d T / d p added to w_g.  (double: the adjoints of a family sum to
//                                  zero, so what the images' derivatives have in common cancels -- tdelay_dpsi.)
// No atomics; every output element is written by one thread in a fixed order: two calls give identical bits.  The delay tables and
// the scratch are kernel arguments of their own: PosArgs keeps its layout.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_dual.h"
#include "gl_mp_delay.h"
#include "gl_multiplane.hip.h"
#include "gl_multiplane_pos.hip.h"
#include "gl_potential.hip.h"

namespace glk {

constexpr int MP_TDELAY_WG = 64;

struct MpDelayArgs {
  const float* delay;      // [J] arrival times (NaN: not measured), the concatenated image order of the position tables
  const float* delay_err;  // [J]
  const float* lam_given;  // [F] lambda_f, NaN: profiled
  const double* geom;      // [J][MP_MAXK] g_f of every image's family, zero-padded
  const double* pot;       // [MP_MAXK] v_i
  double* trace;           // [B][J][5] beta_x, beta_y, theta_last x, y, T0
  double* src;             // [B][F][2] mean beta
  double* aj;              // [B][J] a_j (0 for an image without a measured time)
};

// planes in front of the family: the non-zero head of its weight row (that of its coupling row; the setter sees to it)
__device__ __forceinline__ int mp_tdelay_planes(const double* __restrict__ g) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < MP_MAXK; ++i)
    if (g[i] != 0.) n = i + 1;
  return n;
}

// the unit derivative of the seeded parameter (a plain ray carries none)
__device__ __forceinline__ void mp_tdelay_seed(double&) {}
__device__ __forceinline__ void mp_tdelay_seed(gld::Dual<double, 1>& v) { v.d[0] = 1.; }

// One lens of sample b at the ray's position on its plane: deflection and potential (the multipole included, as in
// gl_mp_fermat_kernel).  k: the parameter of this lens that carries the direction, or -1.
template <class R>
__device__ __forceinline__ void mp_tdelay_lens(const PosArgs& a, const CompDesc& cd, int b, int k, const R& x, const R& y, R& ax, R& ay,
                                               R& psi) {
  R p[POS_MAXP];
#pragma unroll
  for (int m = 0; m < POS_MAXP; ++m) {
    p[m] = R(m < cd.n_par ? (double)a.params[(size_t)b * a.P + cd.p_off + m] : 0.);
    if (m == k) mp_tdelay_seed(p[m]);
  }
  lens_point<R, false>(a, cd, p, x, y, ax, ay);
  psi = lens_potential_point<R, false>(a, cd, p, x, y);
}

// ... as functions of their own (the outlined lens calls of gl_tdelays.hip.h): the sums of the recursion are not held in registers
// across the lens templates, which fill the register file on double (inlined, the trace kernel spills 6 VGPRs)
static __device__ __attribute__((noinline)) void mp_tdelay_lens_value(const PosArgs& a, const CompDesc& cd, int b, const double& x,
                                                                      const double& y, double& ax, double& ay, double& psi) {
  mp_tdelay_lens<double>(a, cd, b, -1, x, y, ax, ay, psi);
}
static __device__ __attribute__((noinline)) void mp_tdelay_lens_dual(const PosArgs& a, const CompDesc& cd, int b, int k,
                                                                     const gld::Dual<double, 1>& x, const gld::Dual<double, 1>& y,
                                                                     gld::Dual<double, 1>& ax, gld::Dual<double, 1>& ay,
                                                                     gld::Dual<double, 1>& psi) {
  mp_tdelay_lens<gld::Dual<double, 1>>(a, cd, b, k, x, y, ax, ay, psi);
}

__global__ void __launch_bounds__(MP_TDELAY_WG) gl_mp_pos_tdelay_trace_kernel(PosArgs a, MpArgs mp, const float* __restrict__ tg,
                                                                              MpDelayArgs q) {
  const int i = blockIdx.x * MP_TDELAY_WG + threadIdx.x;
  if (i >= a.B * a.J) return;
  const int b = i / a.J, j = i - b * a.J;
  const double* geom = q.geom + (size_t)j * MP_MAXK;
  const int last = mp_tdelay_planes(geom) - 1;
  const double tx = (double)a.px[j], ty = (double)a.py[j];
  glp::MpDelayState<MP_MAXK> st;
  for (int t = 0; t < a.n_lens; ++t) {
    const int l = mp.order[t], pl = mp.plane[l];
    if (pl > last) break;  // (lenses come in plane order: everything from here on lies at or behind the family)
    const CompDesc cd = a.comps[l];
    double x = tx, y = ty;
    st.to_plane(pl, mp.scale, x, y);
    double ax, ay, psi;
    mp_tdelay_lens_value(a, cd, b, x, y, ax, ay, psi);
    st.add(pl, ax, ay, psi);
  }
  const float* T = tg + (size_t)j * MP_MAXK;
  double bx = tx, by = ty;
#pragma unroll
  for (int k = 0; k < MP_MAXK; ++k) {
    const float c = T[k];
    if (c != 0.f) {  // (a plane at or behind the family is not part of its rays)
      bx -= (double)c * st.ax[k];
      by -= (double)c * st.ay[k];
    }
  }
  double lx, ly;
  const double T0 = st.arrival_head(mp.scale, tx, ty, geom, q.pot, MP_MAXK, lx, ly);
  double* o = q.trace + (size_t)i * 5;
  o[0] = bx; o[1] = by; o[2] = lx; o[3] = ly; o[4] = T0;
}

// scale, offset [B][F] (lambda_f, T_f) and model_delay [B][J] (lambda_f phi_j + T_f) or null
__global__ void __launch_bounds__(MP_TDELAY_WG) gl_mp_pos_tdelay_kernel(PosArgs a, MpDelayArgs q, int accumulate, float* __restrict__ scale,
                                                                        float* __restrict__ offset, float* __restrict__ model_delay) {
  const int i = blockIdx.x * MP_TDELAY_WG + threadIdx.x;
  if (i >= a.B * a.F) return;
  const int b = i / a.F, f = i - b * a.F;
  const int j0 = a.fam_off[f], j1 = a.fam_off[f + 1], nf = j1 - j0;
  const double* tr = q.trace + (size_t)b * a.J * 5;
  double* tab = q.aj + (size_t)b * a.J;
  const float two_pi = 6.283185307179586f;
  // the barycentre of ALL images
  double mbx = 0., mby = 0.;
  for (int j = j0; j < j1; ++j) {
    mbx += tr[j * 5];
    mby += tr[j * 5 + 1];
  }
  mbx /= (double)nf;
  mby /= (double)nf;
  q.src[(size_t)i * 2] = mbx;
  q.src[(size_t)i * 2 + 1] = mby;
  double glast = 0.;  // the weight of the last plane in front of the family
  {
    // (the row of the family's first image: gl_model_set_position_plane_delays copies the family's row to every one of its images)
    const double* g = q.geom + (size_t)j0 * MP_MAXK;
#pragma unroll
    for (int k = 0; k < MP_MAXK; ++k)
      if (g[k] != 0.) glast = g[k];
  }
  auto fermat = [&](int j) {
    const double dx = tr[j * 5 + 2] - mbx, dy = tr[j * 5 + 3] - mby;
    return tr[j * 5 + 4] + glast * (0.5 * (dx * dx + dy * dy));
  };
  // the weighted means.  All sums of this thread run in float64 (gl_pos_tdelay_kernel: why)
  double sw = 0., swp = 0., swt = 0.;
  float norm = 0.f;
  int n = 0;
  for (int j = j0; j < j1; ++j) {
    const float t = q.delay[j];
    if (t != t) continue;
    const float s = q.delay_err[j];
    const double wt = 1. / ((double)s * (double)s);
    sw += wt;
    swp += wt * fermat(j);
    swt += wt * (double)t;
    norm += logf(two_pi * s * s);
    ++n;
  }
  const double pbar = swp / sw, tbar = swt / sw;  // (a family without delays: 0 / 0, the NaN its optional outputs report)
  double lam = (double)q.lam_given[f];
  if (lam != lam) {
    double stp = 0., spp = 0.;
    for (int j = j0; j < j1; ++j) {
      const float t = q.delay[j];
      if (t != t) continue;
      const float s = q.delay_err[j];
      const double wt = 1. / ((double)s * (double)s), pc = fermat(j) - pbar;
      stp += wt * ((double)t - tbar) * pc;
      spp += wt * pc * pc;
    }
    lam = stp / spp;
  }
  if (!n) lam = (double)__builtin_nanf("");
  if (scale) scale[(size_t)b * a.F + f] = (float)lam;
  if (offset) offset[(size_t)b * a.F + f] = (float)(tbar - lam * pbar);
  if (model_delay)
    for (int j = j0; j < j1; ++j) model_delay[(size_t)b * a.J + j] = (float)(tbar + lam * (fermat(j) - pbar));
  // residuals, chi2, a_j and the adjoint of the barycentre
  double chi2d = 0., gxd = 0., gyd = 0.;
  for (int j = j0; j < j1; ++j) {
    const float t = q.delay[j];
    double ad = 0.;
    if (t == t) {
      const float s = q.delay_err[j];
      const double wt = 1. / ((double)s * (double)s);
      const double r = ((double)t - tbar) - lam * (fermat(j) - pbar);
      chi2d += wt * r * r;
      ad = lam * wt * r;
      gxd -= ad * glast * (tr[j * 5 + 2] - mbx);
      gyd -= ad * glast * (tr[j * 5 + 3] - mby);
    }
    tab[j] = ad;
  }
  const float chi2 = (float)chi2d;
  float gx = (float)gxd, gy = (float)gyd;
  float* fam = a.w_fam + ((size_t)b * a.F + f) * 2;
  const float ll = n ? -0.5f * (chi2 + norm) : 0.f;
  if (!accumulate) {
    fam[0] = ll;
    fam[1] = chi2;
  } else if (n) {  // (a family without delays keeps the bits of the kernels before)
    fam[0] += ll;
    fam[1] += chi2;
  }
  if (!a.grad) return;
  gx /= (float)nf;
  gy /= (float)nf;
  for (int j = j0; j < j1; ++j) {
    float* o = a.w_adj + ((size_t)b * a.J + j) * 3;
    if (!accumulate) {
      o[0] = gx;
      o[1] = gy;
      o[2] = 0.f;
    } else if (n) {
      o[0] += gx;
      o[1] += gy;
    }
  }
}

__global__ void __launch_bounds__(MP_TDELAY_WG) gl_mp_pos_tdelay_grad_kernel(PosArgs a, MpArgs mp, MpDelayArgs q, int lens_params) {
  const int i = blockIdx.x * MP_TDELAY_WG + threadIdx.x;
  if (i >= a.B * a.J * lens_params) return;
  const int col = i % lens_params, bj = i / lens_params;
  const int b = bj / a.J, j = bj - b * a.J;
  const double aw = q.aj[(size_t)b * a.J + j];
  if (aw == 0.) return;  // (no measured time: P3's bits stay)
  const double* geom = q.geom + (size_t)j * MP_MAXK;
  const int last = mp_tdelay_planes(geom) - 1;
  const int own = lens_of_column(a, col);
  if (mp.plane[own] > last) return;  // the column's plane lies at or behind the family: its rays never meet the lens
  const int kown = col - a.comps[own].p_off;
  int f = 0;  // the image's family: mean beta
  while (a.fam_off[f + 1] <= j) ++f;
  using W = gld::Dual<double, 1>;
  const W tx((double)a.px[j]), ty((double)a.py[j]);
  glp::MpDelayState<MP_MAXK, W> st;
  for (int t = 0; t < a.n_lens; ++t) {
    const int l = mp.order[t], pl = mp.plane[l];
    if (pl > last) break;
    const CompDesc cd = a.comps[l];
    W x = tx, y = ty;
    st.to_plane(pl, mp.scale, x, y);
    W ax, ay, psi;
    mp_tdelay_lens_dual(a, cd, b, l == own ? kown : -1, x, y, ax, ay, psi);
    st.add(pl, ax, ay, psi);
  }
  const double* s = q.src + ((size_t)b * a.F + f) * 2;
  const W T = st.arrival(mp.scale, tx, ty, W(s[0]), W(s[1]), geom, q.pot, MP_MAXK, nullptr);
  a.w_g[((size_t)b * a.J + j) * a.P + col] += (float)(aw * T.d[0]);
}

}  // namespace glk
