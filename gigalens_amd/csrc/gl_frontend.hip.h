// gl_frontend.hip.h -- the front end of a call: raw parameter rows (or the unconstrained vector z) -> derived constants, the
// catalogue members' constants and the cost order of the dispatch.  Included by gigalens_hip.hip alone, which launches them.
#pragma once
#include "gl_kernels.hip.h"

namespace glk {

// ---- unconstrained-space front/back end: bijector + prior fused into prep / finalize -------------
// One ZCol (gl_kernels.hip.h) per column k of z.  Default event-space bijectors and log-densities restate TFP's (Identity / Exp / Sigmoid(lo,hi);
// Normal / LogNormal / Uniform / TruncatedNormal) -- see gigalens_amd/prior.py for the same maths in torch.
struct ZEval { float x, dxdz, logp_plus_fldj, dlogp_dx, dfldj_dz; };

// Sigmoid(lo, hi): the constrained value, kept inside [lo, hi] -- at saturation lo + (hi - lo) * 1 may round above hi, where the
// support test of Uniform / TruncatedNormal would return -inf for a z whose density is finite.  (A NaN stays a NaN.)
__device__ __forceinline__ float z_sigmoid_x(float lo, float hi, float z) {
  float x = lo + (hi - lo) * (1.f / (1.f + expf(-z)));
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

__device__ __forceinline__ ZEval z_eval(const ZCol& c, float z) {
  ZEval o;
  float fldj;
  float lnx = 0.f;
  if (c.bijector == 0) {
    o.x = z; o.dxdz = 1.f; fldj = 0.f; o.dfldj_dz = 0.f;
  } else if (c.bijector == 1) {
    o.x = expf(z); o.dxdz = o.x; fldj = z; o.dfldj_dz = 1.f; lnx = z;
  } else {
    const float w = c.hi - c.lo;
    o.x = z_sigmoid_x(c.lo, c.hi, z);
    // sg (1 - sg) = e / (1 + e)^2 with e = exp(-|z|): the product form cancels in 1 - sg (relative error 1e-3 at |z| = 10, 0.17
    // at 15); 1 - 2 sg = -tanh(z / 2) for the same reason around z = 0
    const float az = fabsf(z), e = expf(-az), r = 1.f / (1.f + e);
    o.dxdz = w * e * (r * r);
    // log(hi-lo) - softplus(-z) - softplus(z)
    fldj = logf(w) - az - 2.f * log1pf(e);
    o.dfldj_dz = -tanhf(0.5f * z);
  }
  const float half_log_2pi = 0.91893853320467274178f;
  float logp;
  if (c.prior == 0 || c.prior == 3) {
    float u = (o.x - c.a) / c.b;
    logp = -0.5f * u * u - logf(c.b) - half_log_2pi - (c.prior == 3 ? c.log_norm : 0.f);
    o.dlogp_dx = -u / c.b;
    if (c.prior == 3 && !(o.x >= c.lo && o.x <= c.hi)) { logp = -INFINITY; o.dlogp_dx = 0.f; }
  } else if (c.prior == 1) {
    if (c.bijector != 1) lnx = logf(o.x);
    float u = (lnx - c.a) / c.b;
    logp = -0.5f * u * u - logf(c.b) - half_log_2pi - lnx;
    o.dlogp_dx = (-u / c.b - 1.f) / o.x;
  } else {
    bool in = (o.x >= c.lo && o.x <= c.hi);
    logp = in ? -logf(c.hi - c.lo) : -INFINITY;
    o.dlogp_dx = 0.f;
  }
  o.logp_plus_fldj = logp + fldj;
  return o;
}

// the constrained value alone (the front end needs nothing else of z_eval)
__device__ __forceinline__ float z_eval_x(const ZCol& c, float z) {
  if (c.bijector == 0) return z;
  if (c.bijector == 1) return expf(z);
  return z_sigmoid_x(c.lo, c.hi, z);
}

// ---- per-sample prep: raw parameter rows -> derived constants --------------------------------
// derived block `d` of one component from its slice `p` of the constrained row: the one per-kind switch of the front end
__device__ __forceinline__ void prep_component(const CompDesc& cd, const float* p, float* d, const InterpDev* __restrict__ interp,
                                               const InterpMassDev* __restrict__ interp_mass) {
  switch (cd.kind) {
    case K_EPL: epl_prep<float>(p, cd.iparam, d); break;
    case K_SIE: sie_prep<float>(p, d); break;
    case K_NFW: nfw_prep<float>(p, d); break;
    case K_SHEAR: shear_prep<float>(p, d); break;
    case K_SIS: sis_prep<float>(p, d); break;
    case K_DPIS: case K_DPIE: case K_DPIEP: dpie_prep<float>(cd.kind, p, d); break;
    case K_SCALED: d[0] = d[1] = d[2] = d[3] = 0.f; break;
    case K_SERIES: d[0] = p[0]; d[1] = p[1]; d[2] = d[3] = 0.f; break;
    case K_NFW_ELLIPSE: nfw_ell_prep<float>(p, d); break;
    case K_TNFW: tnfw_prep<float>(p, d); break;
    case K_INTERPOL_MASS: interpmass_prep<float>(p, interp_mass[cd.iparam], d); break;
    case K_MULTIPOLE: multipole_prep<float>(p, cd.iparam, d); break;
    case K_CORE_SERSIC: core_sersic_prep<float>(p, d); break;
    case K_INTERPOL: interp_prep<float>(p, interp[cd.iparam].h, interp[cd.iparam].w, d); break;
    case K_SERSIC: sersic_prep<float>(p, false, d); break;
    case K_SERSIC_ELLIPSE: sersic_prep<float>(p, true, d); break;
    case K_SHAPELETS: shapelets_prep<float>(p, cd.iparam, d); break;
    case K_USER_MASS: case K_USER_LIGHT: for (int k = 0; k < cd.iparam; ++k) d[k] = p[k]; break;  // the body reads its parameters
  }
}

// Thread per component.  params_in != null: packed constrained rows in; else z -> params_out (kept for finalize) through the
// bijectors, then the same.  `cost` (optional): per-sample dispatch cost = the EPL trip count, written by the thread of component
// `cost_comp` (models with exactly one EPL), so that gl_order_kernel reads one coalesced int array
__global__ void __launch_bounds__(128) gl_prep_kernel(const CompDesc* __restrict__ comps, int n_comp,
                                                      const float* __restrict__ params_in, const float* __restrict__ z, int d_z,
                                                      const ZCol* __restrict__ zcols, const int* __restrict__ src,
                                                      const float* __restrict__ const_row, int P, int B,
                                                      float* __restrict__ params_out, float* __restrict__ derived, int D,
                                                      int* __restrict__ cost, int cost_comp, const InterpDev* __restrict__ interp,
                                                      const InterpMassDev* __restrict__ interp_mass) {
  int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= B * n_comp) return;
  int b = i / n_comp, c = i - b * n_comp;
  CompDesc cd = comps[c];
  const float* p;
  if (params_in) {
    p = params_in + (size_t)b * P + cd.p_off;
  } else {
    float* po = params_out + (size_t)b * P + cd.p_off;
    for (int j = 0; j < cd.n_par; ++j) {
      int col = cd.p_off + j;
      int k = src[col];
      po[j] = (k >= 0) ? z_eval(zcols[k], z[(size_t)b * d_z + k]).x : const_row[col];
    }
    p = po;
  }
  float* d = derived + (size_t)b * D + cd.d_off;
  prep_component(cd, p, d, interp, interp_mass);
  if (cost && c == cost_comp) cost[b] = reinterpret_cast<const int*>(d)[EPL_KI];
}

// ---- wave-per-sample front end (models with EPL lenses) --------------------------------------------------------------
// The thread-per-component kernel above leaves the EPL coefficient table to ONE thread: ~15-50 dependent iterations with a
// division each, 7.5 us of latency in front of a 90 us main kernel.  Here one wavefront owns a sample: lane c does what the
// thread of component c does above except the table, then all 64 lanes build the table of each EPL lens -- lane n takes
// row n: its factors (one division), and the running products by an inclusive scan over the lanes.  The recurrence
//   (c, cf, ct) <- (c p, cf p + c r, ct p + c dp/dt)      [r = p / f = dp/df]
// is the product of matrices [[p,0,0],[r,p,0],[dpdt,0,p]], closed under (P, Qf, Qt) o (P', Qf', Qt') =
// (P P', Qf P' + P Qf', Qt P' + P Qt'): associative, so six shuffle steps replace the chain (no division by p or f:
// f = 0 and gamma = 1 stay finite exactly like the sequential form).
struct EplScan { float P, Qf, Qt; };
__device__ __forceinline__ EplScan epl_scan_combine(const EplScan& lo, const EplScan& hi) {  // rows of `lo` come first
  return EplScan{lo.P * hi.P, lo.Qf * hi.P + lo.P * hi.Qf, lo.Qt * hi.P + lo.P * hi.Qt};
}
__device__ __forceinline__ void epl_table_wave(float f, float two_mt, int K, float* __restrict__ tab, int lane) {
  EplScan carry{1.f, 0.f, 0.f};
  for (int base = 0; base <= K + 3; base += 64) {
    const int n = base + lane;
    EplScan v{1.f, 0.f, 0.f};  // row 0: c_0 = 1, derivatives 0
    if (n >= 1 && n <= K) {
      float r, pn, dpdt;
      epl_row_factors<float>(n, f, two_mt, r, pn, dpdt);
      v = EplScan{pn, r, dpdt};
    }
#pragma unroll
    for (int delta = 1; delta < 64; delta <<= 1) {
      EplScan u{__shfl_up(v.P, delta), __shfl_up(v.Qf, delta), __shfl_up(v.Qt, delta)};
      if (lane >= delta) v = epl_scan_combine(u, v);
    }
    v = epl_scan_combine(carry, v);
    if (n <= K) {
      reinterpret_cast<float4*>(tab)[n] = float4{v.P, (float)(2 * n + 1) * v.P, v.Qf, v.Qt};
    } else if (n <= K + 3) {
      reinterpret_cast<float4*>(tab)[n] = float4{0.f, 0.f, 0.f, 0.f};  // the four-row trips of the Clenshaw loop may start above K
    }
    carry = EplScan{__shfl(v.P, 63), __shfl(v.Qf, 63), __shfl(v.Qt, 63)};
  }
}

// counting sort of the samples on their cost (<= 255), heaviest first, by ONE workgroup of NT threads: LDS histogram, one
// wavefront's scan over the 256 bins in descending order (four bins per lane + a shuffle scan), scatter through the bins'
// running offsets.  cost_of(b) is evaluated twice per sample (no staging array).
// split_rank >= 0 (B <= 4 NT, NT = 256): the order inside the cost bin that straddles that rank is made the sample order instead
// of the order of arrival of the atomics, so WHICH samples have a rank below split_rank is the same on every launch
// (tail_plan: they are summed over other pixel chunks than the rest, and results stay bitwise reproducible).
template <int NT, class F>
__device__ __forceinline__ void gl_order_sort(F&& cost_of, int B, int* __restrict__ order, int split_rank = -1) {
  __shared__ int hist[256];
  __shared__ int offs[256];
  __shared__ int s_split, s_group[4 * NT / 64];
  const int tid = threadIdx.x;
  for (int i = tid; i < 256; i += NT) hist[i] = 0;
  if (tid == 0) s_split = -1;
  __syncthreads();
  // the first four samples of a thread stay in registers between the two passes (B <= 4 NT: all of them), their loads in flight together
  int mine[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = tid + i * NT;
    mine[i] = b < B ? max(0, min(cost_of(b), 255)) : 0;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (tid + i * NT < B) atomicAdd(&hist[mine[i]], 1);
  for (int b = tid + 4 * NT; b < B; b += NT) atomicAdd(&hist[max(0, min(cost_of(b), 255))], 1);
  __syncthreads();
  if (tid < 64) {
    const int top = 255 - 4 * tid;  // this lane's bins, heaviest first: top, top - 1, top - 2, top - 3
    const int h0 = hist[top], h1 = hist[top - 1], h2 = hist[top - 2], h3 = hist[top - 3];
    const int sum = h0 + h1 + h2 + h3;
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (tid >= d) incl += t;
    }
    const int excl = incl - sum;  // samples in strictly heavier bins of other lanes
    offs[top] = excl;
    offs[top - 1] = excl + h0;
    offs[top - 2] = excl + h0 + h1;
    offs[top - 3] = excl + h0 + h1 + h2;
  }
  __syncthreads();
  int sb = -1;
  if (split_rank >= 0 && NT == 256) {  // wave-uniform
    if (offs[tid] < split_rank && split_rank < offs[tid] + hist[tid]) s_split = tid;  // at most one bin
    __syncthreads();
    sb = s_split;
  }
  if (sb >= 0) {
    // stable ranks inside bin sb: samples 64 g .. 64 g + 63 are group g = 4 i + wavefront; per-group counts, then a prefix
    const int lane = tid & 63, wv = tid >> 6;
    int rk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long mk = __ballot(tid + i * NT < B && mine[i] == sb);
      rk[i] = __popcll(mk & ((1ull << lane) - 1ull));
      if (lane == 0) s_group[i * (NT / 64) + wv] = __popcll(mk);
    }
    __syncthreads();
    const int base = offs[sb];  // no atomic touches this bin's counter below
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (tid + i * NT < B && mine[i] == sb) {
        int pre = 0;
        for (int g = 0; g < i * (NT / 64) + wv; ++g) pre += s_group[g];
        order[base + pre + rk[i]] = tid + i * NT;
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (tid + i * NT < B && mine[i] != sb) order[atomicAdd(&offs[mine[i]], 1)] = tid + i * NT;
  for (int b = tid + 4 * NT; b < B; b += NT) order[atomicAdd(&offs[max(0, min(cost_of(b), 255))], 1)] = b;
}

// params_in != null: packed constrained rows in; else z -> params_out through the bijectors (as gl_prep_kernel).  n_comp <= 64.
__global__ void __launch_bounds__(256) gl_prep_wave_kernel(const CompDesc* __restrict__ comps, int n_comp,
                                                           const float* __restrict__ params_in, const float* __restrict__ z,
                                                           int d_z, const ZCol* __restrict__ zcols,
                                                           const int* __restrict__ src, const float* __restrict__ const_row,
                                                           int P, int B, float* __restrict__ params_out,
                                                           float* __restrict__ derived, int D, int* __restrict__ cost,
                                                           int cost_comp, int* __restrict__ order, int row_lds, int split_rank,
                                                           const InterpDev* __restrict__ interp,
                                                           const InterpMassDev* __restrict__ interp_mass) {
  // Cost-ordered dispatch without a launch of its own: with `order` the grid carries ONE extra workgroup that sorts the samples
  // by the trip count of their EPL series while the others build the samples' constants.  It needs no result of theirs: the count
  // depends on (e1, e2) alone (epl_cost), which it takes from the parameter rows -- or, on the z path, through the two columns'
  // bijectors.  (A "last workgroup to arrive sorts" scheme was measured first: 256 device-scope atomics on one counter, 0.5 ms.)
  if (order && blockIdx.x == gridDim.x - 1) {
    const CompDesc ce = comps[cost_comp];
    const int c1 = ce.p_off + 2, c2 = ce.p_off + 3, cap = ce.iparam;
    // what is the same for every sample is fetched once: where e1 and e2 come from (a z column and its bijector, or a constant)
    int k1 = -1, k2 = -1;
    ZCol z1{}, z2{};
    float k1c = 0.f, k2c = 0.f;
    if (!params_in) {
      k1 = src[c1];
      k2 = src[c2];
      if (k1 >= 0) z1 = zcols[k1]; else k1c = const_row[c1];
      if (k2 >= 0) z2 = zcols[k2]; else k2c = const_row[c2];
    }
    gl_order_sort<256>([&](int b) {
      float e1, e2;
      if (params_in) {
        e1 = params_in[(size_t)b * P + c1];
        e2 = params_in[(size_t)b * P + c2];
      } else {
        e1 = k1 >= 0 ? z_eval_x(z1, z[(size_t)b * d_z + k1]) : k1c;
        e2 = k2 >= 0 ? z_eval_x(z2, z[(size_t)b * d_z + k2]) : k2c;
      }
      return epl_cost<float>(e1, e2, cap);
    }, B, order, split_rank);
    return;
  }
  const int b = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (b >= B) return;  // whole wavefronts leave together
  float f = 0.f, two_mt = 0.f;
  int K = 0;
  // The constrained row of the sample goes to params_out (the finalize kernel reads it) AND, with row_lds, into the wavefront's own
  // LDS row: the component lanes take their parameters from there instead of reading the global row back (a round trip through
  // the L2 behind a store), and the component descriptors are requested before the bijector loads, not after them -- the
  // front end is a chain of dependent memory round trips and nothing else (5.7 us at C2 with four of them in a row).
  extern __shared__ float s_rows[];  // [4 wavefronts][P], or nothing
  float* row = row_lds ? s_rows + (threadIdx.x >> 6) * P : nullptr;
  CompDesc cd{};
  if (lane < n_comp) cd = comps[lane];
  if (!params_in) {
    // z -> constrained row, one COLUMN per lane: the bijectors of a sample's columns are independent, so their loads
    // (column descriptor, z) and transcendentals overlap instead of forming one lane's chain of n_par dependent round trips
    float* po = params_out + (size_t)b * P;
    for (int k = lane; k < d_z; k += 64) {
      const ZCol zc = zcols[k];
      const float v = z_eval_x(zc, z[(size_t)b * d_z + k]);
      po[zc.param_col] = v;
      if (row) row[zc.param_col] = v;
    }
    for (int col = lane; col < P; col += 64)
      if (src[col] < 0) {
        const float v = const_row[col];
        po[col] = v;
        if (row) row[col] = v;
      }
    if (!row) __threadfence_block();  // the component lanes below read the global row back (same wavefront, same L1)
  } else if (row) {
    for (int col = lane; col < P; col += 64) row[col] = params_in[(size_t)b * P + col];
  }
  // a wavefront's LDS accesses execute in order: the fence only keeps the compiler from moving the reads above the writes
  if (row) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const float* prow = row ? row : (params_in ? params_in : params_out) + (size_t)b * P;
  if (lane < n_comp) {
    const float* p = prow + cd.p_off;
    float* d = derived + (size_t)b * D + cd.d_off;
    if (cd.kind == K_EPL) {  // the head here; the table below, by the whole wavefront
      K = epl_prep_head<float>(p, cd.iparam, d, f, two_mt);
    } else if (cd.kind == K_SHAPELETS) {  // the four constants here; the amplitude blocks below, by the whole wavefront
      d[SHP_CX] = p[1]; d[SHP_CY] = p[2]; d[SHP_IB] = 1.f / p[0]; d[SHP_NMAX] = (float)cd.iparam;
    } else {
      prep_component(cd, p, d, interp, interp_mass);
    }
    if (cost && lane == cost_comp) cost[b] = K;
  }
  for (int c = 0; c < n_comp; ++c) {  // wave-uniform: every lane joins the amplitude blocks of every shapelet component
    if (comps[c].kind != K_SHAPELETS) continue;  // (one lane copying 66 + 144 values one by one: 18.6 us of prep at C3)
    const CompDesc cs = comps[c];
    const float* p = prow + cs.p_off;
    float* d = derived + (size_t)b * D + cs.d_off;
    const int n_max = cs.iparam, L = sh_layers(n_max);
    const int tri = n_max > SH_CAP ? ((SH_MAXLB + 3) & ~3) : ((SH_MAXL + 3) & ~3);
    for (int i = lane; i < tri; i += 64) d[SHP_AMP + i] = i < L ? p[3 + i] : 0.f;
    if (n_max <= SH_CAP)
      for (int e = lane; e < SH_SQ * SH_SQ; e += 64) {
        const int n1 = e / SH_SQ, n2 = e - n1 * SH_SQ, n = n1 + n2;
        d[SHP_SQ + e] = n <= n_max ? p[3 + n * (n + 1) / 2 + n2] * (SH_K[n1] * SH_K[n2]) : 0.f;  // scaled for the monic basis of gl_shp.hip.h
      }
  }
  for (int c = 0; c < n_comp; ++c) {  // wave-uniform: every lane joins the table of every EPL lens
    if (comps[c].kind != K_EPL) continue;
    const float fc = __shfl(f, c), tc = __shfl(two_mt, c);
    const int Kc = __shfl(K, c);
    epl_table_wave(fc, tc, Kc, derived + (size_t)b * D + comps[c].d_off + EPL_TAB, lane);
  }
}

// per (sample, galaxy) constants of the catalogue members: radii, amplitude and the map to the scale gradients
__global__ void __launch_bounds__(128) gl_galprep_kernel(const CompDesc* __restrict__ comps,
                                                         const CatDev* __restrict__ cats, int n_cats,
                                                         const float* __restrict__ params, int P, int B,
                                                         const float* __restrict__ table,
                                                         const float* __restrict__ gal_static,
                                                         float* __restrict__ gal_dyn, int G) {
  int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= B * G) return;
  int b = i / G, g = i - b * G;
  int c = 0;
  while (c + 1 < n_cats && g >= cats[c + 1].g_off) ++c;
  const CatDev cat = cats[c];
  ScaledDesc sd{cat.base_kind, cat.n_gal, {cat.col[0], cat.col[1], cat.col[2]}};
  member_dyn(sd, table + (size_t)7 * g, gal_static + (size_t)g * DP_NS, params + (size_t)b * P + comps[cat.comp].p_off,
             gal_dyn + ((size_t)b * G + g) * GM_ND);
}

// cost-ordered dispatch as a launch of its own: samples sorted by descending EPL trip count (the only data-dependent cost on
// the path), so the heaviest workgroups start first and the tail of the launch is filled with light ones.
constexpr int ORDER_WG = 1024;
__global__ void __launch_bounds__(ORDER_WG) gl_order_kernel(const CompDesc* __restrict__ comps, int n_lens,
                                                            const float* __restrict__ derived, int D, int B,
                                                            int* __restrict__ order, const int* __restrict__ cost_in) {
  gl_order_sort<ORDER_WG>([&](int b) {
    if (cost_in) return cost_in[b];
    int k = 0;
    for (int l = 0; l < n_lens; ++l)
      if (comps[l].kind == K_EPL) k += reinterpret_cast<const int*>(derived + (size_t)b * D + comps[l].d_off)[EPL_KI];
    return k;
  }, B, order);
}

}  // namespace glk
