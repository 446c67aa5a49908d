// gl_potential.hip.h -- lensing potential psi summed over a model's lenses on arbitrary points or the model's own grid
// (beyond the reference, which has no potential), the building block of Fermat potentials and time delays.
//
// psi is the potential whose gradient is THIS library's deflection (lens_point, gl_positions.hip.h), reference quirks
// included; each kind's closed form (or quadrature, TNFW) and its additive constant are documented at its *_pot template
// (gl_profiles.h, gl_dpie.h, gl_extra.h).  Only differences of psi are physical.  Series-expansion lenses (their field
// holds no potential) and user-written bodies (K_USER_MASS, which includes the run-time compiled ScalingRelation member
// loops) have none: gl_lens_potential refuses them on the host, so the switch below never sees them.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_positions.hip.h"

namespace glk {

// psi of one lens at (x, y) with raw parameters p (K_SCALED: the member sum with the scaled parameters of scaled_dyn).  CATS = false:
// for models that hold no catalogue (lens planes refuse them), as lens_point_closed -- the member loop indexes p at run time
template <class R, bool CATS = true> __device__ R lens_potential_point(const PosArgs& a, const CompDesc& cd, const R* p, R x, R y) {
  using namespace glp;
  switch (cd.kind) {
    case K_EPL: return epl_pot<R>(p, cd.iparam, x, y);
    case K_SIE: { R d[SIE_ND + 1]; sie_prep<R>(p, d); return sie_pot<R>(d, x, y); }
    case K_NFW: { R d[NFW_ND]; nfw_prep<R>(p, d); return nfw_pot<R>(d, x, y); }
    case K_SHEAR: { R d[4]; shear_prep<R>(p, d); return shear_pot<R>(d, x, y); }
    case K_DPIS:
    case K_DPIE:
    case K_DPIEP: { R d[DPX_ND]; dpie_prep<R>(cd.kind, p, d); return dpie_pot<R>(cd.kind, d, x, y); }
    case K_NFW_ELLIPSE: { R d[NFE_ND]; nfw_ell_prep<R>(p, d); return nfw_ell_pot<R>(d, x, y); }
    case K_TNFW: { R d[TNF_ND]; tnfw_prep<R>(p, d); return tnfw_pot<R>(d, x, y); }
    case K_MULTIPOLE: { R d[MPL_ND]; multipole_prep<R>(p, cd.iparam, d); return multipole_pot<R>(d, cd.iparam, x, y); }
    case K_SCALED: if constexpr (!CATS) {
      return R(__builtin_nanf(""));  // (not reached)
    } else {
      const CatDev cat = a.cats[cd.iparam];
      const ScaledDesc sd{cat.base_kind, cat.n_gal, {cat.col[0], cat.col[1], cat.col[2]}};
      R psi = R(0.f);
      for (int g = 0; g < cat.n_gal; ++g) {
        const float* gs = a.gal_static + (size_t)(cat.g_off + g) * DP_NS;
        R ds[DP_NS], dd[DP_ND];
        for (int i = 0; i < DP_NS; ++i) ds[i] = R(gs[i]);
        scaled_dyn<R>(sd, a.gal_table + (size_t)(cat.g_off + g) * 7, p, dd);
        psi += cat.base_kind == K_DPIE ? piemd_pot<R>(ds, dd, x, y) : piep_pot<R>(ds, dd, x, y);
      }
      return psi;
    }
    default: { R d[4]; sis_prep<R>(p, d); return sis_pot<R>(d, x, y); }
  }
}

constexpr int POT_WG = 256;

// out[n_pts][B] = sum over the lenses of psi; thread = (point, sample), sample fastest, as gl_lens_maps_kernel
__global__ void __launch_bounds__(POT_WG) gl_lens_potential_kernel(PosArgs a, const float* __restrict__ x,
                                                                  const float* __restrict__ y, long long n_pts,
                                                                  int xy_batched, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * POT_WG + threadIdx.x;
  if (i >= n_pts * a.B) return;
  const PointAt at(i, a.B, xy_batched, x, y);
  float psi = 0.f;
  for (int l = 0; l < a.n_lens; ++l) {
    const CompDesc cd = a.comps[l];
    float p[POS_MAXP];
    for (int k = 0; k < cd.n_par; ++k) p[k] = a.params[(size_t)at.b * a.P + cd.p_off + k];
    psi += lens_potential_point<float>(a, cd, p, at.x, at.y);
  }
  out[i] = psi;
}

// MassProfile.potential at plugin level: one free-standing built-in lens, params [B][n_par], out[n_pts][B]
__global__ void __launch_bounds__(POT_WG) gl_profile_potential_kernel(CompDesc cd, const float* __restrict__ x,
                                                                     const float* __restrict__ y, long long n_pts, int B,
                                                                     int xy_batched, const float* __restrict__ params,
                                                                     float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * POT_WG + threadIdx.x;
  if (i >= n_pts * B) return;
  const PointAt at(i, B, xy_batched, x, y);
  float p[7];
  for (int k = 0; k < cd.n_par; ++k) p[k] = params[(size_t)at.b * cd.n_par + k];
  PosArgs none{};
  out[i] = lens_potential_point<float>(none, cd, p, at.x, at.y);
}

}  // namespace glk
