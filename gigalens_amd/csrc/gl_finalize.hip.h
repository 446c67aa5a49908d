// gl_finalize.hip.h -- the back end of a call: the chunk partials of every sample summed in a fixed order, the chain rule to the raw
// parameters and (unconstrained-space calls) on to z with the log-prior.  Included by gigalens_hip.hip alone, which launches it.
#pragma once
#include "gl_frontend.hip.h"  // z_eval

namespace glk {

// ---- finalize: sum chunk partials (fixed order), chain rule to raw parameters -------------------
// With zcols != null the gradient is carried on to the unconstrained vector z and the log-prior
// + log|J| is added:  log_prob = loglike + sum_k [log p_k(x_k) + fldj_k(z_k)]   (tf/model.py:164-167).

// one sample, executed by NT threads of one workgroup; `s`: LDS scratch of A + P + d_z (+12) floats
// BASIC: only EPL / SIE / Shear / SIS / Sersic in the model -- the other families' chain rules (TNFW's float64 core, shapelets,
// dPIE, ...) stay out of the kernel: a third of the code, and the finalize launch is instruction-fetch bound
template <int NT, bool BASIC = false>
__device__ __forceinline__ void finalize_sample(const CompDesc* __restrict__ comps, const FinArgs& f,
                                                const float* __restrict__ partial, int n_chunks, int b, int tid,
                                                float* s) {
  const int A = f.A, P = f.P, d_z = f.d_z;
  float* s_g = s + ((A + 3) & ~3);
  float* s_t = s_g + ((P + 3) & ~3);
  float* s_e = s_t + ((d_z + 3) & ~3);  // [4][d_z]: dlogp/dx, dx/dz, dfldj/dz, parameter column of every column of z
  const float* src = partial + (size_t)b * n_chunks * A;
  // Phase 0 -- three independent jobs on three groups of threads, so their global round trips and transcendentals overlap
  // instead of queueing behind two barriers: (a) sum the chunk partials, (b) bijector / prior terms of z (they do not depend
  // on the accumulators), (c) fetch the component descriptors
  for (int k = tid; k < A; k += NT) {
    float v = 0.f;
    if (f.use_partial)
      for (int ch = 0; ch < n_chunks; ++ch) v += src[(size_t)ch * A + k];
    if (f.extra_stats && k < 2) v += f.extra_stats[2 * b + k];  // chi2 / normalisation of a materialised image (PSF path)
    s[k] = v;
  }
  constexpr int ZT0 = NT / 2;  // the upper half of the workgroup serves the columns of z
  if (f.zcols && tid >= ZT0) {
    for (int k = tid - ZT0; k < d_z; k += NT - ZT0) {
      const ZCol c = f.zcols[k];
      const ZEval e = z_eval(c, f.z[(size_t)b * d_z + k]);
      s_t[k] = e.logp_plus_fldj;
      s_e[k] = e.dlogp_dx;
      s_e[d_z + k] = e.dxdz;
      s_e[2 * d_z + k] = e.dfldj_dz;
      s_e[3 * d_z + k] = __int_as_float(c.param_col);
    }
  }
  const bool want_grad = f.grad != nullptr || f.grad_z != nullptr;
  CompDesc cd{};
  // the sample's parameter row goes to LDS whole, requested together with everything else (the components' own slices would
  // be a round trip that can only start once their descriptors have arrived)
  float* s_p = s_e + 4 * d_z + 4;
  if (want_grad) {
    for (int k = tid; k < P; k += NT) s_p[k] = f.params[(size_t)b * P + k];
    if (tid < f.n_comp) cd = comps[tid];
  }
  __syncthreads();
  if (want_grad) {
    for (int c = tid; c < f.n_comp; c += NT) {
      if (c != tid) cd = comps[c];
      const float* p = s_p + cd.p_off;
      float* g = s_g + cd.p_off;
      const float* acc = s + cd.a_off;
      switch (cd.kind) {
        case K_EPL: epl_finalize<float>(p, acc, g); break;
        case K_SIE: sie_finalize<float>(p, acc, g); break;
        case K_NFW: if constexpr (!BASIC) nfw_finalize<float>(p, acc, g); break;
        case K_SHEAR: shear_finalize<float>(p, acc, g); break;
        case K_SIS: sis_finalize<float>(p, acc, g); break;
        case K_DPIS: case K_DPIE: case K_DPIEP: if constexpr (!BASIC) dpie_finalize<float>(cd.kind, p, acc, g); break;
        case K_SCALED:
          if constexpr (!BASIC) {
            const CatDev cat = f.cats[cd.iparam];
            for (int k = 0; k < 3; ++k)
              if (cat.col[k] >= 0) g[cat.col[k]] = acc[k];
          }
          break;
        case K_SERIES: if constexpr (!BASIC) { g[0] = acc[0]; g[1] = acc[1]; } break;
        case K_NFW_ELLIPSE: if constexpr (!BASIC) nfw_ell_finalize<float>(p, acc, g); break;
        case K_TNFW: if constexpr (!BASIC) tnfw_finalize<float>(p, acc, g); break;
        case K_INTERPOL_MASS: if constexpr (!BASIC) interpmass_finalize<float>(p, acc, g); break;
        case K_MULTIPOLE: if constexpr (!BASIC) multipole_finalize<float>(p, acc, g); break;
        case K_CORE_SERSIC: if constexpr (!BASIC) core_sersic_finalize<float>(p, acc, g); break;
        case K_INTERPOL: if constexpr (!BASIC) interp_finalize<float>(p, acc, g); break;
        case K_SERSIC: sersic_finalize<float>(p, false, acc, g); break;
        case K_SERSIC_ELLIPSE: sersic_finalize<float>(p, true, acc, g); break;
        case K_SHAPELETS: if constexpr (!BASIC) shapelets_finalize<float>(p, cd.iparam, acc, g); break;
        case K_USER_MASS: case K_USER_LIGHT: if constexpr (!BASIC) { for (int k = 0; k < cd.iparam; ++k) g[k] = acc[k]; } break;  // d/dp_k as summed
      }
    }
    __syncthreads();
    if (f.pos_grad) {  // image-position likelihood: its parameter gradient joins before the chain to z
      for (int k = tid; k < P; k += NT) s_g[k] += f.pos_grad[(size_t)b * P + k];
      __syncthreads();
    }
    // A NaN log-likelihood (sigma^2 = bg^2 + model / t < 0 somewhere: tf/model.py:96 takes its square root) has a NaN gradient
    // in the reference -- the square root's derivative is NaN there and NaN x 0 stays NaN through every pixel sum -- while the
    // cotangent the kernels form (from 1 / sigma^2) stays finite: the whole row follows the reference.
    const float poison = (s[0] + s[1]) != (s[0] + s[1]) ? __int_as_float(0x7fc00000) : 0.f;
    if (f.grad)
      for (int k = tid; k < P; k += NT) f.grad[(size_t)b * P + k] = s_g[k] + poison;
    if (f.zcols && f.grad_z && tid >= ZT0)
      for (int k = tid - ZT0; k < d_z; k += NT - ZT0)
        f.grad_z[(size_t)b * d_z + k] = (s_g[__float_as_int(s_e[3 * d_z + k])] + s_e[k]) * s_e[d_z + k] + s_e[2 * d_z + k] + poison;
  }
  if (tid == 0 && f.loglike) {
    float ll = -0.5f * (s[0] + s[1]);  // tf/model.py:99
    float c2 = s[0] * f.chi2_scale;
    if (f.pos_ll) {  // tf/model.py:157-162
      ll += f.pos_ll[b];
      c2 += f.pos_chi2[b] * f.pos_chi2_scale;
    }
    f.loglike[b] = ll;
    f.chi2[b] = c2;
    if (f.zcols && f.logprob) {
      float lp = 0.f;
      for (int k = 0; k < d_z; ++k) lp += s_t[k];
      f.logprob[b] = ll + lp;
    }
  }
}

template <bool BASIC>
__global__ void __launch_bounds__(128) gl_finalize_kernel(const CompDesc* __restrict__ comps, FinArgs f,
                                                          const float* __restrict__ partial, int n_chunks) {
  extern __shared__ float s[];  // [A] accumulators, [P] parameter gradients, [d_z] prior terms, [4][d_z] bijector / prior derivatives, [P] parameters
#ifdef GL_EXPERIMENTS
  if (n_chunks < 0) return;  // GIGALENS_HIP_DBGFLAGS & 8: the cost of the bare launch (results undefined)
#endif
  finalize_sample<128, BASIC>(comps, f, partial, n_chunks, blockIdx.x, threadIdx.x, s);
}

}  // namespace glk
