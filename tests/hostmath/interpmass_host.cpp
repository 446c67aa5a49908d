// Host instantiation of the interpolated-lens templates (gigalens_amd/csrc/gl_interp_mass.h) -- test harness only, its own build
// like interp_host.cpp:
//   g++ -O2 -std=c++17 -shared -fPIC -o libinterpmass_host.so interpmass_host.cpp     (tests/interpmass_cases.py loads it with ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o interpmass_host_check interpmass_host.cpp
// The second form is a stand-alone program: it walks maps of several shapes with in-range, apron, far, huge, negative and
// non-finite coordinates through the FLOAT instantiation of prep / fwd / vjp / finalize (the one the kernels run) and on
// Dual<float, 2>, and checks that a lane outside the range contributes exact zeros and that every lane inside is finite.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../gigalens_amd/csrc/gl_dual.h"
#include "../../gigalens_amd/csrc/gl_interp_mass.h"

using namespace glp;

namespace {
// map [h][w] -> table [(h + 4)][(w + 4)] with the two-pixel zero apron (what gl_model_set_lens_maps uploads)
std::vector<float> padded(const float* map, int h, int w) {
  const int ws = w + 2 * INT_APRON;
  std::vector<float> t((size_t)(h + 2 * INT_APRON) * ws, 0.f);
  for (int j = 0; j < h; ++j)
    for (int i = 0; i < w; ++i) t[(size_t)(j + INT_APRON) * ws + i + INT_APRON] = map[(size_t)j * w + i];
  return t;
}

// p = [scale_factor, center_x, center_y]; (gx, gy): cotangent of the deflection.  ax, ay [n]; grad[3] = sum_i g_i . d alpha_i / dp;
// gpx, gpy [n] = g_i . d alpha_i / d (x_i, y_i)
template <class R>
void run(int h, int w, const float* map_x, const float* map_y, R pitch, const R* p, int n, const R* x, const R* y, const R* gx,
         const R* gy, R* ax, R* ay, R* grad, R* gpx, R* gpy) {
  const std::vector<float> tx = padded(map_x, h, w), ty = padded(map_y, h, w);
  const InterpMassTab<R> tb{tx.data(), ty.data(), h, w, (R)1 / pitch};
  R d[IM_ND], acc[IM_NACC] = {0, 0, 0};
  interpmass_prep<R>(p, tb, d);
  for (int i = 0; i < n; ++i) {
    interpmass_fwd<R>(d, tb, x[i], y[i], ax[i], ay[i]);
    gpx[i] = gpy[i] = (R)0;
    interpmass_vjp<R>(d, tb, x[i], y[i], gx[i], gy[i], acc, gpx[i], gpy[i]);
  }
  interpmass_finalize<R>(p, acc, grad);
}
}  // namespace

extern "C" {

void interpmass_d(int h, int w, const float* map_x, const float* map_y, double pitch, const double* p, int n, const double* x,
                  const double* y, const double* gx, const double* gy, double* ax, double* ay, double* grad, double* gpx, double* gpy) {
  run<double>(h, w, map_x, map_y, pitch, p, n, x, y, gx, gy, ax, ay, grad, gpx, gpy);
}

// the deflection and its derivative in (x, y) from Dual<double, 2>: out[6][n] = alpha_x, alpha_y, f_xx, f_xy, f_yx, f_yy
void interpmass_jet_d(int h, int w, const float* map_x, const float* map_y, double pitch, const double* p, int n, const double* x,
                      const double* y, double* out) {
  using R = gld::Dual<double, 2>;
  const std::vector<float> tx = padded(map_x, h, w), ty = padded(map_y, h, w);
  const InterpMassTab<double> tb{tx.data(), ty.data(), h, w, 1.0 / pitch};
  const R pr[3] = {R(p[0]), R(p[1]), R(p[2])};
  R d[IM_ND];
  interpmass_prep<R>(pr, tb, d);
  for (int i = 0; i < n; ++i) {
    R xd(x[i]), yd(y[i]), ax, ay;
    xd.d[0] = 1.0;
    yd.d[1] = 1.0;
    interpmass_fwd<R>(d, tb, xd, yd, ax, ay);
    out[i] = ax.v; out[n + i] = ay.v;
    out[2 * n + i] = ax.d[0]; out[3 * n + i] = ax.d[1]; out[4 * n + i] = ay.d[0]; out[5 * n + i] = ay.d[1];
  }
}

}  // extern "C"

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const int shapes[4][2] = {{1, 1}, {2, 3}, {5, 4}, {16, 16}};
  int bad = 0, checked = 0;
  for (const auto& hw : shapes) {
    const int h = hw[0], w = hw[1];
    std::vector<float> mx((size_t)h * w), my((size_t)h * w);
    for (size_t k = 0; k < mx.size(); ++k) {
      mx[k] = 1.f + 0.37f * (float)((k * 7919u) % 13u) - 0.11f * (float)k;
      my[k] = -0.5f + 0.21f * (float)((k * 104729u) % 11u) + 0.07f * (float)k;
    }
    const float pitch = 0.05f, p[3] = {1.3f, 0.03f, -0.02f};
    // pixel coordinates (u, v) to visit, mapped back to the sky
    std::vector<float> us, vs;
    const float edge[] = {-3.4e38f, -1e30f, -1e10f, -3.f, -2.001f, -2.f, -1.5f, -1.f, -0.25f, 0.f, 0.5f, 1.f, (float)w - 1, (float)w - 0.5f,
                          (float)w, (float)w + 0.999f, (float)w + 1, (float)w + 1.001f, (float)w + 7, 3e9f, 1e30f, 3.4e38f, inf, -inf, nan};
    for (float u : edge)
      for (float v : {-2.5f, -2.f, -0.5f, 0.f, 0.5f * (h - 1), (float)h, (float)h + 1, (float)h + 1.5f, -3e9f, 1e30f, inf, nan}) {
        us.push_back(u);
        vs.push_back(v);
      }
    const int n = (int)us.size();
    std::vector<float> x(n), y(n), g1(n, 1.f), g2(n, -0.5f), ax(n), ay(n), gpx(n), gpy(n);
    for (int i = 0; i < n; ++i) {
      x[i] = p[1] + (us[i] - 0.5f * (w - 1)) * pitch;
      y[i] = p[2] + (vs[i] - 0.5f * (h - 1)) * pitch;
    }
    float grad[3];
    run<float>(h, w, mx.data(), my.data(), pitch, p, n, x.data(), y.data(), g1.data(), g2.data(), ax.data(), ay.data(), grad, gpx.data(),
               gpy.data());
    // the same points on Dual<float, 2>, the type of the lens maps and of the solver kernels
    using J = gld::Dual<float, 2>;
    const std::vector<float> tx = padded(mx.data(), h, w), ty = padded(my.data(), h, w);
    const InterpMassTab<float> tb{tx.data(), ty.data(), h, w, 1.f / pitch};
    const J pj[3] = {J(p[0]), J(p[1]), J(p[2])};
    J dj[IM_ND];
    interpmass_prep<J>(pj, tb, dj);
    for (int i = 0; i < n; ++i) {
      ++checked;
      J xd(x[i]), yd(y[i]), jx, jy;
      xd.d[0] = 1.f;
      yd.d[1] = 1.f;
      interpmass_fwd<J>(dj, tb, xd, yd, jx, jy);
      // well outside (a margin covers the rounding of the round trip through the sky): exact zeros
      const bool far = !(us[i] > -2.01f && us[i] < w + 1.01f && vs[i] > -2.01f && vs[i] < h + 1.01f);
      const float all[] = {ax[i], ay[i], gpx[i], gpy[i], jx.v, jy.v, jx.d[0], jx.d[1], jy.d[0], jy.d[1]};
      for (float v : all) {
        if (far && v != 0.f) {
          ++bad;
          std::printf("non-zero outside: %dx%d u=%g v=%g value=%g\n", h, w, us[i], vs[i], v);
        }
        if (!far && !std::isfinite(v)) {
          ++bad;
          std::printf("not finite inside: %dx%d u=%g v=%g\n", h, w, us[i], vs[i]);
        }
      }
    }
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(grad[k])) {
        ++bad;
        std::printf("gradient %d not finite: %dx%d\n", k, h, w);
      }
  }
  std::printf("interpmass_host: %d points checked, %d bad\n", checked, bad);
  return bad ? 1 : 0;
}
