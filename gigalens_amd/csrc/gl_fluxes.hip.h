// gl_fluxes.hip.h -- flux-ratio likelihood of the image families (beyond the reference, which has no such term).  Family f has
// observed images j with beta_j and A_j = d beta / d theta as P1 of the image-position likelihood traces them (gl_positions.hip.h /
// gl_multiplane_pos.hip.h: w_pos, six floats per image), hence  m_j = |mu_j| = 1 / |det A_j|.  Images with a measured flux F_j and
// error s_j enter with weight w_j = 1 / s_j^2 (a NaN flux: no measurement).  The unlensed flux S_f of the family's source is no
// parameter: it is profiled out in closed form,
//   S_f = sum_j w_j F_j m_j / sum_j w_j m_j^2 ,  chi2_f = sum_j w_j (F_j - S_f m_j)^2 ,  ll_f = -1/2 (chi2_f + sum_j log(2 pi s_j^2)).
// S_f minimises chi2_f, so the gradient is the partial derivative at fixed S_f:
//   d ll / d m_j = S_f w_j (F_j - S_f m_j) ,  m = 1 / |det|  =>  d ll / d det_j = -S_f w_j (F_j - S_f m_j) mu_j |mu_j| .
// That adjoint goes into the det slot of w_adj, which P3 and P4 of either path consume unchanged; the term adds nothing to
// d ll / d beta.  Only ratios are constrained: (F, s) -> (c F, c s) leaves chi2_f alone and scales S_f by c.
//
// One kernel, one thread per (sample, family) -- the thread that owns the same elements of w_fam and w_adj in P2:
//   alone       it owns w_fam and w_adj: writes ll / chi2 and adj = (0, 0, d ll / d det)
//   accumulate  launched after gl_pos_p2_kernel on the same stream, it adds to what P2 wrote
// No atomics, a fixed order of operations: two calls give identical bits.  The flux tables are kernel arguments of their own: PosArgs
// keeps the layout the run-time compiled point programs of user-written lenses were built against.
#pragma once
#include "gl_positions.hip.h"

namespace glk {

// flux, flux_err [J] in the concatenated image order of the position tables; amp [B][F] (S_f) and model_flux [B][J] (S_f m_j) or null
__global__ void __launch_bounds__(64) gl_pos_flux_kernel(PosArgs a, const float* __restrict__ flux, const float* __restrict__ flux_err,
                                                         int accumulate, float* __restrict__ amp, float* __restrict__ model_flux) {
  int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.B * a.F) return;
  int b = i / a.F, f = i - b * a.F;
  const int j0 = a.fam_off[f], j1 = a.fam_off[f + 1];
  const float* pos = a.w_pos + ((size_t)b * a.J) * 6;
  const float two_pi = 6.283185307179586f;
  float sfm = 0.f, smm = 0.f, norm = 0.f;
  int n = 0;
  for (int j = j0; j < j1; ++j) {
    const float F = flux[j];
    if (F != F) continue;  // no measurement
    const float* q = pos + j * 6;
    const float det = (1.f - q[2]) * (1.f - q[5]) - q[3] * q[4];
    const float mag = 1.f / fabsf(det), s = flux_err[j], wt = 1.f / (s * s);
    sfm += wt * F * mag;
    smm += wt * mag * mag;
    norm += logf(two_pi * s * s);
    ++n;
  }
  const float S = sfm / smm;  // (a family without fluxes: 0 / 0, the NaN its optional outputs report)
  if (amp) amp[(size_t)b * a.F + f] = S;
  if (model_flux)
    for (int j = j0; j < j1; ++j) {
      const float* q = pos + j * 6;
      model_flux[(size_t)b * a.J + j] = S * (1.f / fabsf((1.f - q[2]) * (1.f - q[5]) - q[3] * q[4]));
    }
  float chi2 = 0.f;
  for (int j = j0; j < j1; ++j) {
    const float F = flux[j];
    if (F != F) continue;
    const float* q = pos + j * 6;
    const float det = (1.f - q[2]) * (1.f - q[5]) - q[3] * q[4];
    const float s = flux_err[j], r = (F - S * (1.f / fabsf(det))) / s;
    chi2 += r * r;
  }
  float* fam = a.w_fam + ((size_t)b * a.F + f) * 2;
  const float ll = n ? -0.5f * (chi2 + norm) : 0.f;
  if (!accumulate) {
    fam[0] = ll;
    fam[1] = chi2;
  } else if (n) {  // (a family without fluxes keeps P2's bits)
    fam[0] += ll;
    fam[1] += chi2;
  }
  if (!a.grad) return;
  for (int j = j0; j < j1; ++j) {
    const float F = flux[j];
    float* o = a.w_adj + ((size_t)b * a.J + j) * 3;
    float g = 0.f;
    if (F == F) {
      const float* q = pos + j * 6;
      const float det = (1.f - q[2]) * (1.f - q[5]) - q[3] * q[4];
      const float mu = 1.f / det, mag = fabsf(mu), s = flux_err[j], wt = 1.f / (s * s);
      g = -S * wt * (F - S * mag) * mu * mag;
    }
    if (!accumulate) {
      o[0] = 0.f;
      o[1] = 0.f;
      o[2] = g;
    } else if (F == F) {
      o[2] += g;
    }
  }
}

}  // namespace glk
