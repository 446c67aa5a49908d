// TEST HARNESS ONLY -- never linked into the product library.
// Instantiates the lensing-potential templates (*_pot of gl_profiles.h, gl_dpie.h, gl_extra.h) on the host in double and
// float, so that tests can check them against the float64 oracle's deflections without a GPU and give the GPU kernel a
// float64 reference.  The product evaluates the same templates only inside gl_lens_potential_kernel.
#include <cmath>
#include <vector>

#include "../../gigalens_amd/csrc/gl_profiles.h"
#include "../../gigalens_amd/csrc/gl_dpie.h"
#include "../../gigalens_amd/csrc/gl_extra.h"

using namespace glp;

namespace {

// psi of one free-standing built-in mass kind (the switch of lens_potential_point, gl_potential.hip.h)
template <class R> R pot_one(int kind, int iparam, const R* p, R x, R y) {
  switch (kind) {
    case K_EPL: return epl_pot<R>(p, iparam > 0 ? iparam : 50, x, y);
    case K_SIE: { R d[SIE_ND + 1]; sie_prep<R>(p, d); return sie_pot<R>(d, x, y); }
    case K_NFW: { R d[NFW_ND]; nfw_prep<R>(p, d); return nfw_pot<R>(d, x, y); }
    case K_SHEAR: { R d[4]; shear_prep<R>(p, d); return shear_pot<R>(d, x, y); }
    case K_SIS: { R d[4]; sis_prep<R>(p, d); return sis_pot<R>(d, x, y); }
    case K_DPIS: case K_DPIE: case K_DPIEP: { R d[DPX_ND]; dpie_prep<R>(kind, p, d); return dpie_pot<R>(kind, d, x, y); }
    case K_NFW_ELLIPSE: { R d[NFE_ND]; nfw_ell_prep<R>(p, d); return nfw_ell_pot<R>(d, x, y); }
    case K_TNFW: { R d[TNF_ND]; tnfw_prep<R>(p, d); return tnfw_pot<R>(d, x, y); }
  }
  return (R)NAN;
}

template <class R> void pot_mass(int kind, int iparam, const R* p, int n, const R* x, const R* y, R* out) {
  for (int i = 0; i < n; ++i) out[i] = pot_one<R>(kind, iparam, p, x[i], y[i]);
}

// ScalingRelation over a dPIE-family catalogue: the member sum with the scaled parameters of scaled_dyn
template <class R> void pot_scaled(int base_kind, int n_gal, const float* table, const int* cols, const R* scales, int n,
                                   const R* x, const R* y, R* out) {
  ScaledDesc sd{base_kind, n_gal, {cols[0], cols[1], cols[2]}};
  for (int i = 0; i < n; ++i) out[i] = 0;
  for (int g = 0; g < n_gal; ++g) {
    R ds[DP_NS], dd[DP_ND];
    scaled_static<R>(base_kind, table + 7 * g, ds);
    scaled_dyn<R>(sd, table + 7 * g, scales, dd);
    for (int i = 0; i < n; ++i)
      out[i] += base_kind == K_DPIE ? piemd_pot<R>(ds, dd, x[i], y[i]) : piep_pot<R>(ds, dd, x[i], y[i]);
  }
}

}  // namespace

extern "C" {
void pot_mass_d(int kind, int iparam, const double* p, int n, const double* x, const double* y, double* out) {
  pot_mass<double>(kind, iparam, p, n, x, y, out);
}
void pot_mass_f(int kind, int iparam, const float* p, int n, const float* x, const float* y, float* out) {
  pot_mass<float>(kind, iparam, p, n, x, y, out);
}
void pot_scaled_d(int base_kind, int n_gal, const float* table, const int* cols, const double* scales, int n, const double* x,
                  const double* y, double* out) {
  pot_scaled<double>(base_kind, n_gal, table, cols, scales, n, x, y, out);
}
}
