// gl_multipole.h -- MULTIPOLE: an m-th order multipole perturbation of the lensing potential (lenstronomy's MULTIPOLE by name and
// parameters; not in the reference).  The usual companion of an EPL: m = 4 makes the isodensity contours boxy or discy, m = 3 skews them.
//
//   [a_m, phi_m, center_x, center_y],  m an integer constant of the profile, 2 <= m <= 8 (CompDesc::iparam)
//   dx = x - center_x, dy = y - center_y, r = |(dx, dy)|, phi the polar angle of (dx, dy)
//   C = cos(m (phi - phi_m)),  S = sin(m (phi - phi_m)),  k = a_m / (1 - m^2)
//   psi     = k r C
//   alpha_x = k (cos phi C + m sin phi S)
//   alpha_y = k (sin phi C - m cos phi S)
//   Hessian = (a_m C / r) t t^T,  t = (-sin phi, cos phi)            (kappa = a_m C / (2 r))
// The deflection does not depend on r; psi is homogeneous of degree 1, so x . alpha = psi.  (m = 1 has another potential, with a
// branch cut in the angle: it is refused, as is every m outside the range -- kind_num_params.)
//
// No atan2, sin or cos per point: prep takes cos / sin of phi_m once per sample; a point forms (cos phi, sin phi) = (dx, dy) / r,
// rotates it by -phi_m and raises it to the m-th power with m - 1 complex multiplications (m is uniform over a wave: the loop is
// a scalar-counted loop of at most 7 trips).
//
// r = 0: the direction is undefined.  (dx, dy) / r is taken as (0, 0) there, which makes the deflection, the potential, every
// gradient sum and the cotangent of the point exact zeros -- the convention of sis_fwd / sis_vjp.
//
// Layout rules of gl_profiles.h.  The order m is an argument of the per-point templates (the kernels hand in CompDesc::iparam).
#pragma once
#include "gl_profiles.h"

namespace glp {

enum { MPL_CX = 0, MPL_CY, MPL_CM /* cos phi_m */, MPL_SM /* sin phi_m */, MPL_K /* a_m / (1 - m^2) */, MPL_MK /* m k */, MPL_AM,
       MPL_K1 /* 1 / (1 - m^2) */, MPL_ND = 8 };
enum { MPLA_CX = 0, MPLA_CY, MPLA_AM, MPLA_PHI, MPL_NACC };

template <class R> GL_HD void multipole_prep(const R* p, int m, R* d) {
  const R k1 = (R)1 / (R)(float)(1 - m * m);
  d[MPL_CX] = p[2];
  d[MPL_CY] = p[3];
  p_sincos(p[1], d[MPL_SM], d[MPL_CM]);
  d[MPL_K] = p[0] * k1;
  d[MPL_MK] = (R)(float)m * (p[0] * k1);
  d[MPL_AM] = p[0];
  d[MPL_K1] = k1;
}

// what every per-point template starts from: 1 / r (0 at the centre), (c, s) = (cos phi, sin phi) and (C, S)
template <class R> struct MultipoleAt { R ir, c, s, C, S; };
template <class R> GL_HD MultipoleAt<R> multipole_at(const R* d, int m, R x, R y) {
  MultipoleAt<R> o;
  const R dx = x - d[MPL_CX], dy = y - d[MPL_CY];
  const R r2 = dx * dx + dy * dy;
  o.ir = r2 > (R)0 ? rcp(sqrt_(r2)) : (R)0;
  o.c = dx * o.ir;
  o.s = dy * o.ir;
  const R c1 = o.c * d[MPL_CM] + o.s * d[MPL_SM], s1 = o.s * d[MPL_CM] - o.c * d[MPL_SM];  // e^{i (phi - phi_m)}
  R ec = c1, es = s1;
#pragma unroll 1
  for (int k = 1; k < m; ++k) {
    const R t = ec * c1 - es * s1;
    es = ec * s1 + es * c1;
    ec = t;
  }
  o.C = ec;
  o.S = es;
  return o;
}

template <class R> GL_HD void multipole_fwd(const R* d, int m, R x, R y, R& ax, R& ay) {
  const MultipoleAt<R> o = multipole_at<R>(d, m, x, y);
  const R kC = d[MPL_K] * o.C, mkS = d[MPL_MK] * o.S;
  ax = o.c * kC + o.s * mkS;
  ay = o.s * kC - o.c * mkS;
}

// psi = k r C with r = (dx^2 + dy^2) / r
template <class R> GL_HD R multipole_pot(const R* d, int m, R x, R y) {
  const MultipoleAt<R> o = multipole_at<R>(d, m, x, y);
  const R dx = x - d[MPL_CX], dy = y - d[MPL_CY];
  return d[MPL_K] * ((dx * dx + dy * dy) * o.ir) * o.C;
}

// adds (gx, gy) . d (alpha_x, alpha_y) / d (centre, a_m, phi_m) into acc (MPLA_*) and the cotangent of the evaluation point into
// (gpx, gpy).  From the closed forms:
//   point:  Hessian g = (a_m C / r) (t . g) t, and the centre sums are its negative;
//   a_m:    alpha is linear in a_m, so the sum is g . alpha formed with 1 / (1 - m^2) in place of k (finite at a_m = 0);
//   phi_m:  dC / dphi_m = m S, dS / dphi_m = -m C.
template <class R> GL_HD void multipole_vjp(const R* d, int m, R x, R y, R gx, R gy, R* acc, R& gpx, R& gpy) {
  const MultipoleAt<R> o = multipole_at<R>(d, m, x, y);
  const R gr = gx * o.c + gy * o.s;  // g . (cos phi, sin phi)
  const R gt = gy * o.c - gx * o.s;  // g . t
  const R h = d[MPL_AM] * o.C * o.ir * gt;
  const R hx = -o.s * h, hy = o.c * h;
  const R mf = (R)(float)m;
  acc[MPLA_CX] -= hx;
  acc[MPLA_CY] -= hy;
  acc[MPLA_AM] += d[MPL_K1] * (gr * o.C - mf * (gt * o.S));
  acc[MPLA_PHI] += mf * (d[MPL_K] * o.S * gr + d[MPL_MK] * o.C * gt);
  gpx += hx;
  gpy += hy;
}
template <class R> GL_HD void multipole_finalize(const R* p, const R* acc, R* g) {
  (void)p;
  g[0] = acc[MPLA_AM];
  g[1] = acc[MPLA_PHI];
  g[2] = acc[MPLA_CX];
  g[3] = acc[MPLA_CY];
}

}  // namespace glp
