// Host instantiation of the interpolated-light templates (gigalens_amd/csrc/gl_interp.h) in float64 -- test harness only, its own
// build like potential_host.cpp:
//   g++ -O2 -std=c++17 -shared -fPIC -o libinterp_host.so interp_host.cpp          (tests/interp_cases.py loads it with ctypes)
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -o interp_host interp_host.cpp && ./interp_host
// The second form is a stand-alone program: it walks images of several shapes with in-range, apron, far, huge, negative and
// non-finite coordinates through prep / fwd / vjp / finalize and checks that a lane outside the range contributes exact zeros.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../gigalens_amd/csrc/gl_interp.h"

using namespace glp;

namespace {
// image [h][w] -> table [(h + 4)][(w + 4)] with the two-pixel zero apron (what gl_model_set_light_image uploads)
std::vector<double> padded(const double* image, int h, int w) {
  const int ws = w + 2 * INT_APRON;
  std::vector<double> t((size_t)(h + 2 * INT_APRON) * ws, 0.0);
  for (int j = 0; j < h; ++j)
    for (int i = 0; i < w; ++i) t[(size_t)(j + INT_APRON) * ws + i + INT_APRON] = image[(size_t)j * w + i];
  return t;
}
}  // namespace

extern "C" {

// p = [center_x, center_y, phi, scale, amp]; I[n]; grad[5] = sum_i gI[i] dI_i/dp; gpx, gpy [n] = gI[i] dI_i/d(x_i, y_i)
void interp_light_d(int linear, int h, int w, const double* image, const double* p, int n, const double* x, const double* y,
                    const double* gI, double* I, double* grad, double* gpx, double* gpy) {
  const std::vector<double> tab = padded(image, h, w);
  const InterpTab<double> tb{tab.data(), h, w};
  double d[INT_ND], acc[INT_NACC] = {0, 0, 0, 0, 0};
  interp_prep<double>(p, h, w, d);
  for (int i = 0; i < n; ++i) {
    I[i] = interp_fwd<double>(d, tb, linear != 0, x[i], y[i]);
    gpx[i] = gpy[i] = 0.0;
    interp_vjp<double>(d, tb, linear != 0, x[i], y[i], gI[i], acc, gpx[i], gpy[i]);
  }
  interp_finalize<double>(p, acc, grad);
}

// the four weights of one axis and their derivatives at t
void interp_weights_d(int linear, double t, double* w, double* dw) { interp_weights<double>(linear != 0, t, w, dw); }

}  // extern "C"

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int shapes[4][2] = {{1, 1}, {2, 3}, {5, 4}, {16, 16}};
  int bad = 0, checked = 0;
  for (const auto& hw : shapes) {
    const int h = hw[0], w = hw[1];
    std::vector<double> img((size_t)h * w);
    for (size_t k = 0; k < img.size(); ++k) img[k] = 1.0 + 0.37 * (double)((k * 7919u) % 13u) - 0.11 * (double)k;
    for (int linear = 0; linear < 2; ++linear) {
      const double p[5] = {0.03, -0.02, 0.4, 0.05, 2.5};
      // pixel coordinates (u, v) to visit, mapped back to the sky through the inverse pose
      std::vector<double> us, vs;
      const double edge[] = {-1e300, -1e30, -3.0, -2.0 - 1e-9, -2.0, -1.5, -1.0, -0.25, 0.0, 0.5, 1.0, (double)w - 1, (double)w - 0.5,
                             (double)w, (double)w + 0.999, (double)w + 1, (double)w + 1 + 1e-9, (double)w + 7, 1e30, 1e300, inf, -inf, nan};
      for (double u : edge)
        for (double v : {-2.5, -2.0, -0.5, 0.0, 0.5 * (h - 1), (double)h, (double)h + 1, (double)h + 1.5, 1e30, nan}) {
          us.push_back(u);
          vs.push_back(v);
        }
      const int n = (int)us.size();
      std::vector<double> x(n), y(n), gI(n, 1.0), I(n), gpx(n), gpy(n);
      const double c = std::cos(p[2]), s = std::sin(p[2]);
      for (int i = 0; i < n; ++i) {
        const double ur = (us[i] - 0.5 * (w - 1)) * p[3], vr = (vs[i] - 0.5 * (h - 1)) * p[3];
        x[i] = p[0] + ur * c - vr * s;
        y[i] = p[1] + ur * s + vr * c;
      }
      double grad[5];
      interp_light_d(linear, h, w, img.data(), p, n, x.data(), y.data(), gI.data(), I.data(), grad, gpx.data(), gpy.data());
      for (int i = 0; i < n; ++i) {
        ++checked;
        // well outside (a margin covers the rounding of the round trip through the sky): exact zeros
        const bool far = !(us[i] > -2.001 && us[i] < w + 1.001 && vs[i] > -2.001 && vs[i] < h + 1.001);
        if (far && !(I[i] == 0.0 && gpx[i] == 0.0 && gpy[i] == 0.0)) {
          ++bad;
          std::printf("non-zero outside: %dx%d linear=%d u=%g v=%g I=%g\n", h, w, linear, us[i], vs[i], I[i]);
        }
        if (!far && !(std::isfinite(I[i]) && std::isfinite(gpx[i]) && std::isfinite(gpy[i]))) {
          ++bad;
          std::printf("not finite inside: %dx%d linear=%d u=%g v=%g\n", h, w, linear, us[i], vs[i]);
        }
      }
      for (int k = 0; k < 5; ++k)
        if (!std::isfinite(grad[k])) {
          ++bad;
          std::printf("gradient %d not finite: %dx%d linear=%d\n", k, h, w, linear);
        }
    }
  }
  std::printf("interp_host: %d points checked, %d bad\n", checked, bad);
  return bad ? 1 : 0;
}
