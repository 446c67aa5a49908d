// gl_mp_delay.h -- the arithmetic of the multi-plane arrival time, apart from the lens templates: what one ray carries through
// the plane recursion and how it becomes T.  Plain C++ on double (GL_HD), so that the kernel (gl_multiplane_fermat.hip.h) and
// the float64 host build of the tests (tests/hostmath/multiplane_fermat_host.cpp) run the same statements.
//
// Planes by ascending redshift, theta_0 = theta the image position, a_i the deflection sum and psi_i the potential sum of the
// lenses on plane i at theta_i, theta_j = theta - sum_{i<j} C_ij a_i.  A source at beta behind the planes 0 .. Ks-1 (the non-zero
// head of its weight row `geom`):
//   T = sum_{i<Ks} [ geom_i |theta_i - theta_next(i)|^2 / 2 - pot_i psi_i ],    theta_next(Ks-1) = beta
// in arcsec^2 c / H0 (cosmology.MultiPlane.delay_weights).  Planes at or behind the source do not enter, whatever their sums hold.
//
// R: the number type of the ray -- double, or a dual on double that carries one parameter direction through the recursion (the
// gradient of the time-delay likelihood on planes, gl_multiplane_tdelays.hip.h).  The couplings and the weights stay plain numbers.
#pragma once
#include "gl_math.h"

namespace glp {

// 2 MAXK + MAXK values that only unrolled loops with constant indices touch (the plane of a lens selects by comparison, as
// MpRegSums of gl_multiplane.hip.h): registers, no private memory
template <int MAXK, class R = double> struct MpDelayState {
  R ax[MAXK], ay[MAXK], psi[MAXK];
  GL_HD MpDelayState() {
#pragma unroll
    for (int i = 0; i < MAXK; ++i) { ax[i] = R(0.); ay[i] = R(0.); psi[i] = R(0.); }
  }
  // theta_pl = theta - sum_{i<pl} C[i][pl] a_i on the float32 couplings the model holds
  GL_HD void to_plane(int pl, const float* scale, R& px, R& py) const {
#pragma unroll
    for (int i = 0; i < MAXK - 1; ++i)
      if (i < pl) {
        const double c = (double)scale[i * MAXK + pl];
        px -= R(c) * ax[i];
        py -= R(c) * ay[i];
      }
  }
  GL_HD void add(int pl, R dax, R day, R dpsi) {
#pragma unroll
    for (int i = 0; i < MAXK; ++i)
      if (i == pl) { ax[i] += dax; ay[i] += day; psi[i] += dpsi; }
  }
  // T of the ray from (tx, ty) to the source (bx, by) once every sum is complete.  terms (or null): sum of the magnitudes of the
  // summands, the scale rounding errors of T are measured against
  GL_HD R arrival(const float* scale, R tx, R ty, R bx, R by, const double* geom, const double* pot, int K, R* terms) const {
    using glm::fabs_;
    R T = R(0.), mag = R(0.);
    R cx = tx, cy = ty;  // theta_i
#pragma unroll
    for (int i = 0; i < MAXK; ++i) {
      const double g = i < K ? geom[i] : 0.;
      if (g != 0.) {
        const bool last = i + 1 >= K || geom[i + 1 < K ? i + 1 : i] == 0.;
        R nx = tx, ny = ty;  // theta_next(i)
        if (last) { nx = bx; ny = by; }
        else to_plane(i + 1, scale, nx, ny);
        const R dx = cx - nx, dy = cy - ny;
        const R geo = R(g) * (R(0.5) * (dx * dx + dy * dy)), grav = R(pot[i]) * psi[i];
        T += geo - grav;
        mag += fabs_(geo) + fabs_(grav);
        cx = nx;
        cy = ny;
      }
    }
    if (terms) *terms = mag;
    return T;
  }
  // T without the geometric summand of the last plane in front of the source -- the only part of T that sees the source -- and
  // (lx, ly) = theta on that plane:  T = head + geom_last |(lx, ly) - beta|^2 / 2  (the time-delay likelihood on planes, whose
  // source is the barycentre of the family's rays: known only once every image has been traced)
  GL_HD R arrival_head(const float* scale, R tx, R ty, const double* geom, const double* pot, int K, R& lx, R& ly) const {
    R T = R(0.);
    R cx = tx, cy = ty;  // theta_i
#pragma unroll
    for (int i = 0; i < MAXK; ++i) {
      const double g = i < K ? geom[i] : 0.;
      if (g != 0.) {
        const bool last = i + 1 >= K || geom[i + 1 < K ? i + 1 : i] == 0.;
        if (!last) {
          R nx = tx, ny = ty;  // theta_next(i)
          to_plane(i + 1, scale, nx, ny);
          const R dx = cx - nx, dy = cy - ny;
          T += R(g) * (R(0.5) * (dx * dx + dy * dy));
          cx = nx;
          cy = ny;
        }
        T -= R(pot[i]) * psi[i];
      }
    }
    lx = cx;
    ly = cy;
    return T;
  }
};

}  // namespace glp
