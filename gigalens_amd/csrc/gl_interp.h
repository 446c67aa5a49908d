// gl_interp.h -- INTERPOL: a light profile that renders a pixelated source image (lenstronomy's INTERPOL by name; not in the
// reference, whose light profiles are all parametric).
//
//   [center_x, center_y, phi, scale, amp],  image[H][W] a constant of the model, shared by the whole batch
//   dx = px - center_x, dy = py - center_y
//   u = ( dx cos phi + dy sin phi) / scale + (W - 1) / 2        column coordinate, +x = increasing column
//   v = (-dx sin phi + dy cos phi) / scale + (H - 1) / 2        row coordinate,    +y = increasing row
//   I = amp sum_j sum_i w(v - j) w(u - i) image[j][i]           surface brightness: no division by scale^2
// with the image zero-extended over all integers, w the hat function (order 1) or Keys' cubic convolution kernel with
// a = -1/2 (order 3): I is continuous everywhere (C1 for order 3) and identically 0 once u < -2, u > W + 1, v < -2 or v > H + 1.
//
// Both orders run one 4 x 4-tap path: the four weights of an axis are polynomials in t = u - floor(u), order 1 being
// (0, 1 - t, t, 0).  The table the kernels read carries a two-pixel zero apron, tab[H + 4][W + 4]; a lane is IN RANGE when its
// (u, v) passes the test above, made in the real type before anything is converted to an integer -- a NaN or an infinite
// coordinate fails it -- and every other lane evaluates the node (0, 0) with its result discarded, so no coordinate that failed
// the test ever becomes an index.  For -2 <= u < -1 and W <= u <= W + 1 one or two of the four taps lie beyond the apron, where
// the image is zero like the apron itself: the tap indices of an axis are clamped into the apron (four integer clamps per
// axis), never tested per tap.
#pragma once
#include "gl_profiles.h"

namespace glp {

enum { INT_CX = 0, INT_CY, INT_C /* cos phi / scale */, INT_S /* sin phi / scale */, INT_U0 /* (W - 1) / 2 */, INT_V0 /* (H - 1) / 2 */,
       INT_AMP, INT_PAD, INT_ND = 8 };
enum { INTA_AMP = 0, INTA_CX, INTA_CY, INTA_PHI, INTA_SC, INT_NACC };
constexpr int INT_APRON = 2;
constexpr int INT_MAX_SIDE = 2048;  // largest image height / width (gl_model_set_light_image)

// the table of one interpolated component as the kernels read it (one per component, indexed by CompDesc::iparam)
template <class R> struct InterpTab {
  const R* tab;  // [(h + 4)][(w + 4)], zero apron included
  int h, w;
};

template <class R> GL_HD void interp_prep(const R* p, int h, int w, R* d) {
  const R inv = (R)1 / p[3];
  d[INT_CX] = p[0];
  d[INT_CY] = p[1];
  d[INT_C] = p_cos(p[2]) * inv;
  d[INT_S] = p_sin(p[2]) * inv;
  d[INT_U0] = (R)0.5 * (R)(w - 1);
  d[INT_V0] = (R)0.5 * (R)(h - 1);
  d[INT_AMP] = p[4];
  d[INT_PAD] = (R)0;
}

// the four weights of one axis at t in [0, 1): taps floor(u) - 1 .. floor(u) + 2, and their derivatives in u
template <class R> GL_HD void interp_weights(bool linear, R t, R* w, R* dw) {
  if (linear) {
    w[0] = (R)0; w[1] = (R)1 - t; w[2] = t; w[3] = (R)0;
    dw[0] = (R)0; dw[1] = (R)-1; dw[2] = (R)1; dw[3] = (R)0;
  } else {
    w[0] = (((R)-0.5 * t + (R)1) * t - (R)0.5) * t;
    w[1] = ((R)1.5 * t - (R)2.5) * t * t + (R)1;
    w[2] = (((R)-1.5 * t + (R)2) * t + (R)0.5) * t;
    w[3] = ((R)0.5 * t - (R)0.5) * t * t;
    dw[0] = ((R)-1.5 * t + (R)2) * t - (R)0.5;
    dw[1] = ((R)4.5 * t - (R)5) * t;
    dw[2] = ((R)-4.5 * t + (R)4) * t + (R)0.5;
    dw[3] = ((R)1.5 * t - (R)1) * t;
  }
}

template <class R> struct InterpPix { R ur, vr, S, Su, Sv; };  // rotated offsets in pixels; sum, d sum / du, d sum / dv (amplitude 1)

GL_HD int interp_clampi(int k, int lo, int hi) { return k < lo ? lo : (k > hi ? hi : k); }

template <class R, bool GRAD> GL_HD void interp_pix(const R* d, const InterpTab<R>& tb, bool linear, R x, R y, InterpPix<R>& o) {
  const R dx = x - d[INT_CX], dy = y - d[INT_CY];
  const R ur = dx * d[INT_C] + dy * d[INT_S], vr = dy * d[INT_C] - dx * d[INT_S];
  const R u = ur + d[INT_U0], v = vr + d[INT_V0];
  // the range test, in R, before any conversion to int: false for NaN and for infinities
  const bool in = u >= (R)-INT_APRON && u <= (R)(tb.w + 1) && v >= (R)-INT_APRON && v <= (R)(tb.h + 1);
  o.ur = in ? ur : (R)0;  // (an offset that is not finite must not meet a zero cotangent in the pose sums: 0 x NaN)
  o.vr = in ? vr : (R)0;
  const R us = in ? u : (R)0, vs = in ? v : (R)0;
  const R fu = floor_(us), fv = floor_(vs);
  const int iu = (int)fu, iv = (int)fv;  // in [-2, w + 1] x [-2, h + 1]
  R wu[4], du[4], wv[4], dv[4];
  interp_weights<R>(linear, us - fu, wu, du);
  interp_weights<R>(linear, vs - fv, wv, dv);
  const int ws = tb.w + 2 * INT_APRON;
  int col[4];
  for (int i = 0; i < 4; ++i) col[i] = interp_clampi(iu - 1 + i, -INT_APRON, tb.w + 1) + INT_APRON;
  R S = (R)0, Su = (R)0, Sv = (R)0;
  for (int j = 0; j < 4; ++j) {
    const R* row = tb.tab + (interp_clampi(iv - 1 + j, -INT_APRON, tb.h + 1) + INT_APRON) * ws;
    const R a0 = row[col[0]], a1 = row[col[1]], a2 = row[col[2]], a3 = row[col[3]];
    const R r = wu[0] * a0 + wu[1] * a1 + wu[2] * a2 + wu[3] * a3;
    S += wv[j] * r;
    if (GRAD) {
      Su += wv[j] * (du[0] * a0 + du[1] * a1 + du[2] * a2 + du[3] * a3);
      Sv += dv[j] * r;
    }
  }
  o.S = in ? S : (R)0;
  o.Su = in ? Su : (R)0;
  o.Sv = in ? Sv : (R)0;
}

// surface brightness with the component's amplitude; interp_fwd_unit: amplitude 1 (the basis image of the linear solve)
template <class R> GL_HD R interp_fwd_unit(const R* d, const InterpTab<R>& tb, bool linear, R x, R y) {
  InterpPix<R> o;
  interp_pix<R, false>(d, tb, linear, x, y, o);
  return o.S;
}
template <class R> GL_HD R interp_fwd(const R* d, const InterpTab<R>& tb, bool linear, R x, R y) {
  return d[INT_AMP] * interp_fwd_unit<R>(d, tb, linear, x, y);
}
// adds gI dI/d(amp, centre, phi, scale) into acc (INTA_*; the scale as the sum over pixels of g . (ur, vr), see interp_finalize)
// and the cotangent of the evaluation point into (gpx, gpy); an out-of-range lane adds zeros
template <class R> GL_HD R interp_vjp(const R* d, const InterpTab<R>& tb, bool linear, R x, R y, R gI, R* acc, R& gpx, R& gpy) {
  InterpPix<R> o;
  interp_pix<R, true>(d, tb, linear, x, y, o);
  const R gS = gI * d[INT_AMP];
  const R gu = gS * o.Su, gv = gS * o.Sv;
  const R gdx = gu * d[INT_C] - gv * d[INT_S], gdy = gu * d[INT_S] + gv * d[INT_C];
  acc[INTA_AMP] += gI * o.S;
  acc[INTA_CX] -= gdx;
  acc[INTA_CY] -= gdy;
  acc[INTA_PHI] += gu * o.vr - gv * o.ur;  // du / dphi = vr, dv / dphi = -ur
  acc[INTA_SC] += gu * o.ur + gv * o.vr;   // du / dscale = -ur / scale, dv / dscale = -vr / scale
  gpx += gdx;
  gpy += gdy;
  return d[INT_AMP] * o.S;
}
template <class R> GL_HD void interp_finalize(const R* p, const R* acc, R* g) {
  g[0] = acc[INTA_CX];
  g[1] = acc[INTA_CY];
  g[2] = acc[INTA_PHI];
  g[3] = -acc[INTA_SC] / p[3];
  g[4] = acc[INTA_AMP];
}

}  // namespace glp
