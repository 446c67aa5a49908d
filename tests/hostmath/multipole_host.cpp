// Host instantiation of the multipole templates (gigalens_amd/csrc/gl_multipole.h) -- test harness only, its own build like
// interpmass_host.cpp:
//   g++ -O2 -std=c++17 -shared -fPIC -o libmultipole_host.so multipole_host.cpp     (tests/multipole_cases.py loads it with ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o multipole_host_check multipole_host.cpp
// The second form is a stand-alone program: it walks every order m = 2..8 through prep / fwd / pot / vjp / finalize on float,
// Dual<float, 2>, Dual<Dual<float, 1>, 2> and Dual<double, 1> (the types the kernels instantiate) at points around the centre, at
// the centre itself, far away and at huge coordinates, and checks that the centre gives exact zeros and every other point finite
// values that satisfy x . alpha = psi.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../gigalens_amd/csrc/gl_dual.h"
#include "../../gigalens_amd/csrc/gl_multipole.h"

using namespace glp;

namespace {
// p = [a_m, phi_m, center_x, center_y]; (gx, gy): cotangent of the deflection.  ax, ay, psi [n]; grad[4] = sum_i g_i . d alpha_i / dp;
// gpx, gpy [n] = g_i . d alpha_i / d (x_i, y_i)
template <class R>
void run(int m, const R* p, int n, const R* x, const R* y, const R* gx, const R* gy, R* ax, R* ay, R* psi, R* grad, R* gpx, R* gpy) {
  R d[MPL_ND], acc[MPL_NACC] = {0, 0, 0, 0};
  multipole_prep<R>(p, m, d);
  for (int i = 0; i < n; ++i) {
    multipole_fwd<R>(d, m, x[i], y[i], ax[i], ay[i]);
    psi[i] = multipole_pot<R>(d, m, x[i], y[i]);
    gpx[i] = gpy[i] = (R)0;
    multipole_vjp<R>(d, m, x[i], y[i], gx[i], gy[i], acc, gpx[i], gpy[i]);
  }
  multipole_finalize<R>(p, acc, grad);
}

// every scalar a (nested) dual carries
void leaves(float v, std::vector<double>& o) { o.push_back(v); }
void leaves(double v, std::vector<double>& o) { o.push_back(v); }
template <class T, int N> void leaves(const gld::Dual<T, N>& v, std::vector<double>& o) {
  leaves(v.v, o);
  for (int i = 0; i < N; ++i) leaves(v.d[i], o);
}

// fwd and pot of one point on the number type R with every seedable slot seeded: all leaves of alpha_x, alpha_y, psi
template <class R, class Seed> std::vector<double> eval_all(int m, const float* pf, float x, float y, Seed&& seed) {
  R p[4] = {R(pf[0]), R(pf[1]), R(pf[2]), R(pf[3])}, xd(x), yd(y), d[MPL_ND], ax, ay;
  seed(p, xd, yd);
  multipole_prep<R>(p, m, d);
  multipole_fwd<R>(d, m, xd, yd, ax, ay);
  const R psi = multipole_pot<R>(d, m, xd, yd);
  std::vector<double> o;
  leaves(ax, o);
  leaves(ay, o);
  leaves(psi, o);
  return o;
}
}  // namespace

extern "C" {

void multipole_d(int m, const double* p, int n, const double* x, const double* y, const double* gx, const double* gy, double* ax,
                 double* ay, double* psi, double* grad, double* gpx, double* gpy) {
  run<double>(m, p, n, x, y, gx, gy, ax, ay, psi, grad, gpx, gpy);
}

// Dual<double, 2> seeded in (x, y): out[9][n] = alpha_x, alpha_y, f_xx, f_xy, f_yx, f_yy (from fwd), psi, d psi / dx, d psi / dy (from pot)
void multipole_jet_d(int m, const double* p, int n, const double* x, const double* y, double* out) {
  using R = gld::Dual<double, 2>;
  const R pr[4] = {R(p[0]), R(p[1]), R(p[2]), R(p[3])};
  R d[MPL_ND];
  multipole_prep<R>(pr, m, d);
  for (int i = 0; i < n; ++i) {
    R xd(x[i]), yd(y[i]), ax, ay;
    xd.d[0] = 1.0;
    yd.d[1] = 1.0;
    multipole_fwd<R>(d, m, xd, yd, ax, ay);
    const R psi = multipole_pot<R>(d, m, xd, yd);
    out[i] = ax.v; out[n + i] = ay.v;
    out[2 * n + i] = ax.d[0]; out[3 * n + i] = ax.d[1]; out[4 * n + i] = ay.d[0]; out[5 * n + i] = ay.d[1];
    out[6 * n + i] = psi.v; out[7 * n + i] = psi.d[0]; out[8 * n + i] = psi.d[1];
  }
}

}  // extern "C"

int main() {
  int bad = 0, checked = 0;
  const float pf[4] = {0.04f, 0.7f, 0.03f, -0.02f};
  const float offs[] = {0.f, 1e-30f, -1e-20f, 1e-6f, -0.37f, 1.f, 2.5f, -1e4f, 1e15f, -3e18f};
  for (int m = MPL_MMIN; m <= MPL_MMAX; ++m) {
    std::vector<float> x, y;
    for (float ox : offs)
      for (float oy : offs) {
        x.push_back(pf[2] + ox);
        y.push_back(pf[3] + oy);
      }
    const int n = (int)x.size();
    std::vector<float> g1(n, 1.f), g2(n, -0.5f), ax(n), ay(n), psi(n), gpx(n), gpy(n);
    float grad[4];
    run<float>(m, pf, n, x.data(), y.data(), g1.data(), g2.data(), ax.data(), ay.data(), psi.data(), grad, gpx.data(), gpy.data());
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(grad[k])) { ++bad; std::printf("m=%d: gradient %d not finite\n", m, k); }
    for (int i = 0; i < n; ++i) {
      ++checked;
      const bool centre = x[i] == pf[2] && y[i] == pf[3];
      using J = gld::Dual<float, 2>;
      using N1 = gld::Dual<float, 1>;
      using N2 = gld::Dual<N1, 2>;
      using W = gld::Dual<double, 1>;
      std::vector<double> all = {ax[i], ay[i], psi[i], gpx[i], gpy[i]};
      const auto j = eval_all<J>(m, pf, x[i], y[i], [](J*, J& xd, J& yd) { xd.d[0] = 1.f; yd.d[1] = 1.f; });
      const auto h = eval_all<N2>(m, pf, x[i], y[i], [](N2* p, N2& xd, N2& yd) { xd.d[0] = N1(1.f); yd.d[1] = N1(1.f); p[1].v.d[0] = 1.f; });
      const auto w = eval_all<W>(m, pf, x[i], y[i], [](W* p, W&, W&) { p[0].d[0] = 1.0; });
      all.insert(all.end(), j.begin(), j.end());
      if (centre) {  // the parameter seeds meet the zero direction as well
        all.insert(all.end(), h.begin(), h.end());
        all.insert(all.end(), w.begin(), w.end());
      }
      const float dx = x[i] - pf[2], dy = y[i] - pf[3];
      const bool tiny = std::fabs(dx) < 1e-15f && std::fabs(dy) < 1e-15f;  // (1 / r and dx^2 leave the float range: the Hessian may be inf)
      for (double v : all) {
        if (centre && v != 0.0) { ++bad; std::printf("m=%d: non-zero at the centre: %g\n", m, v); }
        if (!centre && !tiny && !std::isfinite(v)) { ++bad; std::printf("m=%d: not finite at offset (%g, %g)\n", m, dx, dy); }
      }
      for (double v : h) if (!centre && !tiny && !std::isfinite(v)) { ++bad; std::printf("m=%d: nested dual not finite at (%g, %g)\n", m, dx, dy); }
      for (double v : w) if (!centre && !tiny && !std::isfinite(v)) { ++bad; std::printf("m=%d: wide dual not finite at (%g, %g)\n", m, dx, dy); }
      // Euler: x . alpha = psi (float: a few ulp of |k| r)
      if (!centre && !tiny) {
        const float e = dx * ax[i] + dy * ay[i] - psi[i], tol = 2e-5f * std::fabs(pf[0]) * std::hypot(dx, dy);
        if (!(std::fabs(e) <= tol)) { ++bad; std::printf("m=%d: x . alpha - psi = %g at (%g, %g)\n", m, e, dx, dy); }
      }
    }
  }
  std::printf("multipole_host: %d points checked, %d bad\n", checked, bad);
  return bad ? 1 : 0;
}
