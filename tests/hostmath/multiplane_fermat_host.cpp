// TEST HARNESS ONLY -- never linked into the product library.
// The float64 host build of the multi-plane arrival time (gigalens_amd/csrc/gl_multiplane_fermat.hip.h): the thread body of
// gl_mp_fermat_kernel, statement for statement, on the same templates -- the per-kind deflection and potential (the switches of
// lens_point and lens_potential_point, as potential_host.cpp restates the latter) and MpDelayState of gl_mp_delay.h, which the
// kernel includes as well.  What differs from the kernel is the math library (and which multiply-adds are fused).
//   g++ -O2 -std=c++17 -shared -fPIC -o libmultiplane_fermat_host.so multiplane_fermat_host.cpp   (tests/mp_tdelay_cases.py)
#include <cmath>

#include "../../gigalens_amd/csrc/gl_profiles.h"
#include "../../gigalens_amd/csrc/gl_dpie.h"
#include "../../gigalens_amd/csrc/gl_extra.h"
#include "../../gigalens_amd/csrc/gl_multipole.h"
#include "../../gigalens_amd/csrc/gl_mp_delay.h"

using namespace glp;

namespace {

constexpr int MAXK = 4;  // MP_MAXK
constexpr int MAXP = 7;  // POS_MAXP

void deflection(int kind, int iparam, const double* p, double x, double y, double& ax, double& ay) {
  using R = double;
  switch (kind) {
    case K_MULTIPOLE: { R d[MPL_ND]; multipole_prep<R>(p, iparam, d); multipole_fwd<R>(d, iparam, x, y, ax, ay); } break;
    case K_EPL: epl_point<R>(p, iparam, x, y, ax, ay); break;
    case K_SIE: { R d[SIE_ND + 1]; sie_prep<R>(p, d); sie_fwd<R>(d, x, y, ax, ay); } break;
    case K_NFW: { R d[NFW_ND]; nfw_prep<R>(p, d); nfw_fwd<R>(d, x, y, ax, ay); } break;
    case K_SHEAR: { R d[4]; shear_prep<R>(p, d); shear_fwd<R>(d, x, y, ax, ay); } break;
    case K_DPIS: case K_DPIE: case K_DPIEP: { R d[DPX_ND]; dpie_prep<R>(kind, p, d); dpie_fwd<R>(kind, d, x, y, ax, ay); } break;
    case K_NFW_ELLIPSE: { R d[NFE_ND]; nfw_ell_prep<R>(p, d); nfw_ell_fwd<R>(d, x, y, ax, ay); } break;
    case K_TNFW: { R d[TNF_ND]; tnfw_prep<R>(p, d); tnfw_fwd<R>(d, x, y, ax, ay); } break;
    default: { R d[4]; sis_prep<R>(p, d); sis_fwd<R>(d, x, y, ax, ay); } break;
  }
}

double potential(int kind, int iparam, const double* p, double x, double y) {
  using R = double;
  switch (kind) {
    case K_EPL: return epl_pot<R>(p, iparam, x, y);
    case K_SIE: { R d[SIE_ND + 1]; sie_prep<R>(p, d); return sie_pot<R>(d, x, y); }
    case K_NFW: { R d[NFW_ND]; nfw_prep<R>(p, d); return nfw_pot<R>(d, x, y); }
    case K_SHEAR: { R d[4]; shear_prep<R>(p, d); return shear_pot<R>(d, x, y); }
    case K_DPIS: case K_DPIE: case K_DPIEP: { R d[DPX_ND]; dpie_prep<R>(kind, p, d); return dpie_pot<R>(kind, d, x, y); }
    case K_NFW_ELLIPSE: { R d[NFE_ND]; nfw_ell_prep<R>(p, d); return nfw_ell_pot<R>(d, x, y); }
    case K_TNFW: { R d[TNF_ND]; tnfw_prep<R>(p, d); return tnfw_pot<R>(d, x, y); }
    case K_MULTIPOLE: { R d[MPL_ND]; multipole_prep<R>(p, iparam, d); return multipole_pot<R>(d, iparam, x, y); }
    default: { R d[4]; sis_prep<R>(p, d); return sis_pot<R>(d, x, y); }
  }
}

}  // namespace

extern "C" {

// kind, iparam, n_par, p_off, plane [n_lens] in the model's order; order [n_lens] the lenses sorted by plane (stable); scale
// [MAXK][MAXK] the float32 couplings, zero-padded; params [B][P] float32; x, y [B][S][M] and src_x, src_y [B][S] float32;
// geom [S][K], pot [K]; out, terms [B][S][M]: T and the sum of the magnitudes of its summands
void mp_fermat_host(int n_lens, const int* kind, const int* iparam, const int* n_par, const int* p_off, const int* plane,
                    const int* order, const float* scale, const float* params, int P, int B, int S, int M, const float* x,
                    const float* y, const float* src_x, const float* src_y, const double* geom, const double* pot, int K, double* out,
                    double* terms) {
  for (long long i = 0; i < (long long)B * S * M; ++i) {
    const int b = (int)(i / ((long long)S * M));
    const long long bs = i / M;
    const int s = (int)(bs - (long long)b * S);
    const double tx = (double)x[i], ty = (double)y[i];
    MpDelayState<MAXK> st;
    for (int t = 0; t < n_lens; ++t) {
      const int l = order[t], pl = plane[l];
      double px = tx, py = ty;
      st.to_plane(pl, scale, px, py);
      double p[MAXP];
      for (int k = 0; k < MAXP; ++k) p[k] = k < n_par[l] ? (double)params[(size_t)b * P + p_off[l] + k] : 0.;
      double ax, ay;
      deflection(kind[l], iparam[l], p, px, py, ax, ay);
      st.add(pl, ax, ay, potential(kind[l], iparam[l], p, px, py));
    }
    const double T = st.arrival(scale, tx, ty, (double)src_x[bs], (double)src_y[bs], geom + (size_t)s * K, pot, K, terms + i);
    out[i] = std::isfinite(T) ? T : (double)NAN;
  }
}

}  // extern "C"
