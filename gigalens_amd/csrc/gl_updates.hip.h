// gl_updates.hip.h -- the elementwise kernels of the inference loops: the Adam update, the Gaussian surrogate of SVI, the leapfrog
// and the Metropolis step of HMC.  Included by gl_api_plugin.hip alone, which launches them.
#pragma once
#include "gl_kernels.hip.h"

namespace glk {

// ---- the optimiser update of the MAP / SVI loops (tf/inference.py:33-39 hands the gradient to a Keras Adam) ----------
// One launch instead of ~10 elementwise ones: x -= lr * (m / c1) / (sqrt(v / c2) + eps) with m, v updated in place,
// grad scaled by grad_scale first; c1 = 1 - b1^t, c2 = 1 - b2^t with t from the host or, inside a captured graph,
// from a device counter that thread 0 of block 0 advances AFTER every block has read it (it is read at kernel start
// and written only by the last block to finish, see the ticket).
__global__ void __launch_bounds__(256) gl_adam_kernel(float* __restrict__ x, const float* __restrict__ grad,
                                                      float* __restrict__ m, float* __restrict__ v, long long n,
                                                      float grad_scale, float lr, float b1, float b2, float eps,
                                                      double t_host, double* __restrict__ t_dev,
                                                      unsigned* __restrict__ ticket, float c1_host, float c2_host) {
  // the bias corrections 1 - beta^t: from the host when it knows the step count (two double-precision pow per THREAD were most
  // of this kernel's 4.5 us), on the device only under graph replay, where the count lives in t_dev
  const double t = (t_dev ? t_dev[0] : t_host) + (t_dev ? 1.0 : 0.0);
  float c1 = c1_host, c2 = c2_host;
  if (t_dev) {
    c1 = (float)(1.0 - ::pow((double)b1, t));
    c2 = (float)(1.0 - ::pow((double)b2, t));
  }
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float g = grad[i] * grad_scale;
    const float mi = m[i] * b1 + g * (1.0f - b1);
    const float vi = v[i] * b2 + (g * g) * (1.0f - b2);
    m[i] = mi;
    v[i] = vi;
    const float upd = lr * (mi / c1) / (sqrtf(vi / c2) + eps);
    if (upd != 0.f) x[i] -= upd;  // a zero update (lr == 0) leaves the bits of x alone: -0.0f - (-0.0f) is +0.0f; a NaN still lands
  }
  if (t_dev) {  // advance the device counter once per launch, after the last reader
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      const unsigned done = atomicAdd(ticket, 1u);
      if (done == gridDim.x - 1) {
        t_dev[0] = t;
        *ticket = 0u;
      }
    }
  }
}

// ---- the Gaussian surrogate of the SVI loop (tf/inference.py:64-91; jax/inference.py:98-128) ---------------------------
// q(z) = N(mu, L L^T) with L = FillScaleTriL(diag_bijector=Exp, diag_shift) over the row-major lower-triangle packing
// (full rank) or L = diag(exp(p)) (mean field).  Two small launches bracket the native forward+gradient call:
//   gl_svi_sample_kernel  z_i = mu + L eps_i
//   gl_svi_grad_kernel    the fused collective buffer  [ELBO, dELBO/dmu (d), dELBO/dp (packed)]  from eps, log p(z_i) and
//                         G_i = d log p / d z_i:  dELBO/dmu = -mean G,  dELBO/dL_jk = -mean G_ij eps_ik (k <= j), Exp diagonal
//                         and -log det L of log q in closed form.  One workgroup per output, fixed-order reduction over i.
__device__ __forceinline__ void tril_jk(int t, int& j, int& k) {
  j = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((j + 1) * (j + 2) / 2 <= t) ++j;
  while (j * (j + 1) / 2 > t) --j;
  k = t - j * (j + 1) / 2;
}

__global__ void __launch_bounds__(256) gl_svi_sample_kernel(const float* __restrict__ mu, const float* __restrict__ lp,
                                                            int d, int full_rank, const float* __restrict__ eps, int n,
                                                            float diag_shift, float* __restrict__ z) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * d) return;
  const int r = (int)(i / d), j = (int)(i - (long long)r * d);
  const float* e = eps + (size_t)r * d;
  float v = mu[j];
  if (full_rank) {
    const float* row = lp + j * (j + 1) / 2;
    for (int k = 0; k < j; ++k) v += row[k] * e[k];
    v += (expf(row[j]) + diag_shift) * e[j];
  } else {
    v += expf(lp[j]) * e[j];
  }
  z[i] = v;
}

__global__ void __launch_bounds__(256) gl_svi_grad_kernel(const float* __restrict__ lp, int d, int full_rank,
                                                          const float* __restrict__ eps, const float* __restrict__ logp,
                                                          const float* __restrict__ G, int n, float diag_shift,
                                                          float* __restrict__ buf) {
  __shared__ float red[4];
  const int o = blockIdx.x, tid = threadIdx.x;
  int j = 0, k = 0;
  const int kind = o == 0 ? 0 : (o <= d ? 1 : 2);  // ELBO, d/dmu_j, d/dp_t
  if (kind == 1) j = o - 1;
  if (kind == 2) {
    if (full_rank) tril_jk(o - 1 - d, j, k);
    else j = k = o - 1 - d;
  }
  float acc = 0.f;
  for (int i = tid; i < n; i += 256) {
    if (kind == 0) {
      const float* e = eps + (size_t)i * d;
      float q = 0.f;
      for (int c = 0; c < d; ++c) q += e[c] * e[c];
      acc += -0.5f * q - logp[i];
    } else if (kind == 1) {
      acc -= G[(size_t)i * d + j];
    } else {
      acc -= G[(size_t)i * d + j] * eps[(size_t)i * d + k];
    }
  }
  acc = wave_sum63(acc);
  if ((tid & 63) == 63) red[tid >> 6] = acc;
  __syncthreads();
  if (tid != 0) return;
  float v = (red[0] + red[1] + red[2] + red[3]) / (float)n;
  if (kind == 0) {
    float log_det = 0.f;
    for (int c = 0; c < d; ++c) log_det += full_rank ? logf(expf(lp[c * (c + 1) / 2 + c]) + diag_shift) : lp[c];
    v += -log_det - 0.5f * (float)d * 1.8378770664093453f;  // log 2 pi
  } else if (kind == 2 && j == k) {
    const float p = lp[full_rank ? j * (j + 1) / 2 + j : j];
    const float e = expf(p);
    v = full_rank ? v * e - e / (e + diag_shift) : v * e - 1.f;
  }
  buf[o] = v;
}

// ---- the leapfrog of the preconditioned HMC loop (tf/inference.py:95-182) ----------------------------------------------
// Momentum precision = the surrogate covariance Sigma = L L^T, so a drift is z += eps * (p Sigma).  One launch does the
// momentum kick that precedes a drift and the drift itself; one launch closes a transition: last half kick, kinetic
// energies 1/2 |p L|^2, Metropolis test against the supplied uniforms, and the in-place selection of the state.
// One workgroup per chain, any d (cluster models: d = 132): the chain's momentum row is staged in LDS, thread j owns
// column j, so the rows of Sigma / L are read coalesced and every output element is read and written by the same
// thread (the calls may run in place: p_out == p_in, z_out == z_in).
constexpr int HMC_WG = 128;

__global__ void __launch_bounds__(HMC_WG) gl_hmc_kick_drift_kernel(const float* p_in, const float* __restrict__ grad,
                                                                   float kick, const float* z_in,
                                                                   const float* __restrict__ sigma, float eps, int n, int d,
                                                                   float* p_out, float* z_out) {
  extern __shared__ float s_p[];  // [d]
  const int i = blockIdx.x, tid = threadIdx.x;
  const size_t row = (size_t)i * d;
  for (int j = tid; j < d; j += HMC_WG) {
    const float v = p_in[row + j] + kick * grad[row + j];
    s_p[j] = v;
    p_out[row + j] = v;
  }
  __syncthreads();
  for (int j = tid; j < d; j += HMC_WG) {
    float s = 0.f;
    for (int k = 0; k < d; ++k) s += s_p[k] * sigma[(size_t)k * d + j];
    z_out[row + j] = z_in[row + j] + eps * s;
  }
}

__global__ void __launch_bounds__(HMC_WG) gl_hmc_accept_kernel(float* z, float* g, float* lp, const float* __restrict__ zn,
                                                               const float* __restrict__ gn, const float* __restrict__ lpn,
                                                               const float* __restrict__ p0, const float* __restrict__ pn,
                                                               float kick, const float* __restrict__ L,
                                                               const float* __restrict__ u, int n, int d,
                                                               float* __restrict__ acc_prob) {
  extern __shared__ float s_ab[];  // [2][d] momenta at both ends, then [4] reduction slots
  float* s_a = s_ab;
  float* s_b = s_ab + d;
  __shared__ float red[2][HMC_WG / 64];
  __shared__ int s_take;
  const int i = blockIdx.x, tid = threadIdx.x;
  const size_t row = (size_t)i * d;
  for (int j = tid; j < d; j += HMC_WG) {
    s_a[j] = p0[row + j];
    s_b[j] = pn[row + j] + kick * gn[row + j];
  }
  __syncthreads();
  float ke0 = 0.f, ke1 = 0.f;
  for (int k = tid; k < d; k += HMC_WG) {  // (p L)_k = sum_{j >= k} p_j L_jk, L lower triangular
    float s0 = 0.f, s1 = 0.f;
    for (int j = k; j < d; ++j) {
      const float l = L[(size_t)j * d + k];
      s0 += s_a[j] * l;
      s1 += s_b[j] * l;
    }
    ke0 += s0 * s0;
    ke1 += s1 * s1;
  }
  ke0 = wave_sum63(ke0);
  ke1 = wave_sum63(ke1);
  if ((tid & 63) == 63) { red[0][tid >> 6] = ke0; red[1][tid >> 6] = ke1; }
  __syncthreads();
  if (tid == 0) {
    float k0 = 0.f, k1 = 0.f;
    for (int w = 0; w < HMC_WG / 64; ++w) { k0 += red[0][w]; k1 += red[1][w]; }
    float log_acc = (lpn[i] - 0.5f * k1) - (lp[i] - 0.5f * k0);
    if (!(fabsf(log_acc) <= 3.0e38f)) log_acc = -INFINITY;  // NaN / inf proposals are rejected
    acc_prob[i] = expf(fminf(log_acc, 0.f));
    const int take = logf(u[i]) < log_acc;
    s_take = take;
    if (take) lp[i] = lpn[i];
  }
  __syncthreads();
  if (s_take)
    for (int j = tid; j < d; j += HMC_WG) {
      z[row + j] = zn[row + j];
      g[row + j] = gn[row + j];
    }
}

}  // namespace glk
