// gl_interp_mass.h -- INTERPOL_SCALED: a lens given as two deflection maps on a grid (lenstronomy's INTERPOL_SCALED by name; not in
// the reference, whose lenses are all parametric).  The mass-side twin of gl_interp.h, whose conventions it keeps.
//
//   [scale_factor, center_x, center_y],  alpha_x[H][W], alpha_y[H][W] (arcsec) constants of the model, shared by the whole batch
//   dx = x - center_x, dy = y - center_y
//   u = dx / pitch + (W - 1) / 2        column coordinate, +x = increasing column
//   v = dy / pitch + (H - 1) / 2        row coordinate,    +y = increasing row
//   alpha_x(x, y) = scale_factor sum_j sum_i w(v - j) w(u - i) alpha_x[j][i]        (alpha_y likewise)
// with the maps zero-extended over all integers and w Keys' cubic convolution kernel with a = -1/2 (the cubic path of
// interp_weights, nothing else: a bilinear deflection has a Hessian whose parameter derivatives vanish inside a cell).  The
// deflection is C1 everywhere and identically 0 once u < -2, u > W + 1, v < -2 or v > H + 1.  The Hessian of the lens is the
// derivative of this interpolant, entry by entry: f_xy and f_yx are equal only as far as the maps are the gradient of one potential.
//
// Tables, range test and tap clamps are those of gl_interp.h: each map carries a two-pixel zero apron, tab[H + 4][W + 4]; the range
// test is made on the value of (u, v) before anything is converted to an integer -- a NaN or an infinite coordinate fails it -- and a
// lane that fails it evaluates the node (0, 0) with its result replaced by exact zeros.  The weights are polynomials in t = u -
// floor(u) of the number type R (float, double, or the forward-mode duals of the point kernels: floor, the range test and the index
// clamps act on the value part); the taps are float.
#pragma once
#include "gl_interp.h"

namespace glp {

enum { IM_CX = 0, IM_CY, IM_IP /* 1 / pitch */, IM_U0 /* (W - 1) / 2 */, IM_V0 /* (H - 1) / 2 */, IM_SF, IM_PAD0, IM_PAD1, IM_ND = 8 };
enum { IMA_SF = 0, IMA_CX, IMA_CY, IM_NACC };

// the two maps of one interpolated lens as the kernels read them (one per component, indexed by CompDesc::iparam).  S: the type
// 1 / pitch is kept in (float on the device)
template <class S> struct InterpMassTab {
  const float* ax;  // [(h + 4)][(w + 4)], zero apron included
  const float* ay;
  int h, w;
  S inv_pitch;
};

template <class R, class S> GL_HD void interpmass_prep(const R* p, const InterpMassTab<S>& tb, R* d) {
  d[IM_CX] = p[1];
  d[IM_CY] = p[2];
  d[IM_IP] = (R)tb.inv_pitch;
  d[IM_U0] = (R)0.5 * (R)(float)(tb.w - 1);
  d[IM_V0] = (R)0.5 * (R)(float)(tb.h - 1);
  d[IM_SF] = p[0];
  d[IM_PAD0] = (R)0;
  d[IM_PAD1] = (R)0;
}

// the in-range test and the tap geometry of one evaluation point: weights (and their derivatives in u, v) in R, clamped columns,
// row of the first tap.  Returns the range test; an out-of-range lane holds the geometry of the node (0, 0)
template <class R> struct InterpMassAt {
  R wu[4], du[4], wv[4], dv[4];
  int col[4], iv;
};
template <class R, class S> GL_HD bool interpmass_at(const R* d, const InterpMassTab<S>& tb, R x, R y, InterpMassAt<R>& o) {
  const R u = (x - d[IM_CX]) * d[IM_IP] + d[IM_U0], v = (y - d[IM_CY]) * d[IM_IP] + d[IM_V0];
  // the range test, on values, before any conversion to int: false for NaN and for infinities
  const bool in = u >= (R)(float)-INT_APRON && u <= (R)(float)(tb.w + 1) && v >= (R)(float)-INT_APRON && v <= (R)(float)(tb.h + 1);
  const R us = in ? u : (R)0, vs = in ? v : (R)0;
  const auto fu = floor_(us), fv = floor_(vs);  // plain scalars
  const int iu = (int)fu;                        // (iu, iv) in [-2, w + 1] x [-2, h + 1]
  o.iv = (int)fv;
  interp_weights<R>(false, us - (R)fu, o.wu, o.du);
  interp_weights<R>(false, vs - (R)fv, o.wv, o.dv);
  for (int i = 0; i < 4; ++i) o.col[i] = interp_clampi(iu - 1 + i, -INT_APRON, tb.w + 1) + INT_APRON;
  return in;
}
// offset of tap row j of an evaluation point inside a table; entry j of a weight set (selects: j may be a run-time value)
template <class R, class S> GL_HD int interpmass_row(const InterpMassTab<S>& tb, const InterpMassAt<R>& o, int j) {
  return (interp_clampi(o.iv - 1 + j, -INT_APRON, tb.h + 1) + INT_APRON) * (tb.w + 2 * INT_APRON);
}
template <class R> GL_HD R interpmass_pick(const R* w, int j) { return j == 0 ? w[0] : (j == 1 ? w[1] : (j == 2 ? w[2] : w[3])); }

// deflection of the lens at (x, y), generic in the number type.  On float (the pixel kernels) the sixteen taps of both maps are one
// unrolled block; on the wider types (the point kernels' duals, float64) the row loop stays a loop, so that only one row of taps
// and one row weight are live beside the caller's state
template <class R, class S> GL_HD void interpmass_fwd(const R* d, const InterpMassTab<S>& tb, R x, R y, R& ax, R& ay) {
  InterpMassAt<R> o;
  const bool in = interpmass_at<R, S>(d, tb, x, y, o);
  R sx = (R)0, sy = (R)0;
  auto row = [&](int j) {
    const int r = interpmass_row<R, S>(tb, o, j);
    const float* rx = tb.ax + r;
    const float* ry = tb.ay + r;
    const R wj = interpmass_pick<R>(o.wv, j);
    sx += wj * (o.wu[0] * (R)rx[o.col[0]] + o.wu[1] * (R)rx[o.col[1]] + o.wu[2] * (R)rx[o.col[2]] + o.wu[3] * (R)rx[o.col[3]]);
    sy += wj * (o.wu[0] * (R)ry[o.col[0]] + o.wu[1] * (R)ry[o.col[1]] + o.wu[2] * (R)ry[o.col[2]] + o.wu[3] * (R)ry[o.col[3]]);
  };
  if constexpr (sizeof(R) == sizeof(float)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) row(j);
  } else {
#pragma unroll 1
    for (int j = 0; j < 4; ++j) row(j);
  }
  ax = in ? d[IM_SF] * sx : (R)0;
  ay = in ? d[IM_SF] * sy : (R)0;
}

// adds (gx, gy) . d (alpha_x, alpha_y) / d (scale_factor, centre) into acc (IMA_*) and the cotangent of the evaluation point into
// (gpx, gpy).  (gx, gy) is the cotangent of the deflection, as for every lens VJP: beta = x - sum alpha, so the kernels hand in
// -(g_beta_x, g_beta_y).  The two maps are contracted with the cotangent tap by tap, so one 4 x 4 pass serves both; an out-of-range
// lane adds exact zeros
template <class R, class S>
GL_HD void interpmass_vjp(const R* d, const InterpMassTab<S>& tb, R x, R y, R gx, R gy, R* acc, R& gpx, R& gpy) {
  InterpMassAt<R> o;
  const bool in = interpmass_at<R, S>(d, tb, x, y, o);
  const R hx = in ? gx : (R)0, hy = in ? gy : (R)0;  // (a cotangent that is not finite must not meet the node (0, 0) of a lane out of range)
  R s = (R)0, su = (R)0, sv = (R)0;
  for (int j = 0; j < 4; ++j) {
    const int r = interpmass_row<R, S>(tb, o, j);
    const float* rx = tb.ax + r;
    const float* ry = tb.ay + r;
    R q = (R)0, qu = (R)0;
    for (int i = 0; i < 4; ++i) {
      const R c = hx * (R)rx[o.col[i]] + hy * (R)ry[o.col[i]];
      q += o.wu[i] * c;
      qu += o.du[i] * c;
    }
    s += o.wv[j] * q;
    su += o.wv[j] * qu;
    sv += o.dv[j] * q;
  }
  const R k = d[IM_SF] * d[IM_IP];
  const R gdx = in ? k * su : (R)0, gdy = in ? k * sv : (R)0;
  acc[IMA_SF] += in ? s : (R)0;
  acc[IMA_CX] -= gdx;
  acc[IMA_CY] -= gdy;
  gpx += gdx;
  gpy += gdy;
}
template <class R> GL_HD void interpmass_finalize(const R* p, const R* acc, R* g) {
  (void)p;
  g[0] = acc[IMA_SF];
  g[1] = acc[IMA_CX];
  g[2] = acc[IMA_CY];
}

}  // namespace glp
