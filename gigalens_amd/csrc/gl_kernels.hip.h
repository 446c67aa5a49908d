// gl_kernels.hip.h -- CDNA4 (gfx950) kernels of the lens hot path.
//
// Launch geometry (all kernels): one 256-thread workgroup (4 wave64) works on ONE sample's chunk of
// pixels; grid = (n_chunks, B).  The sample's derived constants (gl_profiles.h) are staged in LDS
// once per workgroup and read by broadcast; pixels are thread-strided so that every global access
// (grid x/y, observed image, image rows) is a contiguous 256-float run per wave-instruction group.
// Reductions (chi^2, normalisation, parameter gradients) are wave64 DPP reductions into per-wave LDS
// slots, then one deterministic pass over the 4 waves, then one row of partials per (sample, chunk)
// in the caller's workspace; gl_finalize_kernel sums chunks in a fixed order (bitwise reproducible,
// no float atomics) and applies the per-sample chain rule to the raw parameters.
// MFMA is deliberately unused: the path is elementwise + transcendental (VALU-bound).
#pragma once
#include <hip/hip_runtime.h>
#include "gl_profiles.h"
#include "gl_dpie.h"
#include "gl_extra.h"
#include "gl_interp.h"
#include "gl_interp_mass.h"
#include "gl_multipole.h"
#include "gl_vec.hip.h"
#include "gl_members.hip.h"
#include "gl_series.h"
#include "gl_shapelets.hip.h"

namespace glk {
using namespace glp;

struct CompDesc {
  int kind, iparam;
  unsigned flags;
  int p_off;  // first column in the packed parameter row
  int d_off;  // offset of the derived block (floats, multiple of 4)
  int a_off;  // offset of the accumulators inside the per-sample accumulator row
  int n_acc;
  int n_par;
  int lin_off;  // light profiles: channel of the first linear basis image in the lstsq stack
};

// one galaxy catalogue of a K_SCALED component (gl_model_set_catalogue)
struct CatDev {
  int base_kind, n_gal;
  int g_off;   // first galaxy inside the model-wide galaxy arrays
  int comp;    // component index
  int col[3];  // theta_E, r_core, r_cut: column of the scale inside the component's parameter row, or -1
  int pad;
};

// coefficient field of one K_SERIES lens (gl_model_set_series): coef[2][order+1][N]
struct SeriesDev {
  const float* coef;   // [2][order+1][N]  deflection series
  const float* hcoef;  // [3][order+1][N]  Hessian series (f_xx, f_xy, f_yy) or null: lens maps only
  float r0;
  int order;
};

// image table of one K_INTERPOL light (gl_model_set_light_image): tab[(h + 4)][(w + 4)] with its zero apron; CompDesc::iparam indexes it
using InterpDev = InterpTab<float>;
// deflection maps of one K_INTERPOL_MASS lens (gl_model_set_lens_maps): two such tables and 1 / pitch; CompDesc::iparam indexes it
using InterpMassDev = InterpMassTab<float>;

// thread i of a (point, sample) launch, sample fastest: its point, its sample and the point's coordinates, which are either one
// list [n_pts] for all samples or a list per sample [n_pts][B] (xy_batched)
struct PointAt {
  long long pt;
  int b;
  float x, y;
  __device__ __forceinline__ PointAt(long long pt_, int b_, long long i, int xy_batched, const float* x_, const float* y_)
      : pt(pt_), b(b_), x(xy_batched ? x_[i] : x_[pt_]), y(xy_batched ? y_[i] : y_[pt_]) {}
  __device__ __forceinline__ PointAt(long long i, int B, int xy_batched, const float* x_, const float* y_)
      : PointAt(i / B, (int)(i - i / B * B), i, xy_batched, x_, y_) {}
};

// One ZCol per column k of z (the k-th leaf of the prior in tf.nest.flatten order, tf/model.py:76-87); evaluated by z_eval (gl_frontend.hip.h)
struct ZCol {
  int param_col;  // destination column in the packed [B,P] row
  int bijector;   // 0 identity, 1 exp, 2 sigmoid(lo,hi)
  int prior;      // 0 normal, 1 lognormal, 2 uniform, 3 truncated normal
  float a, b, lo, hi, log_norm;
};
struct FinArgs {
  int n_comp, P, A, d_z;
  const float* params;
  float *loglike, *chi2, *grad;
  const float* z;
  const ZCol* zcols;
  float *logprob, *grad_z;
  float chi2_scale;
  const float* extra_stats;
  int use_partial;
  const float *pos_ll, *pos_chi2, *pos_grad;
  float pos_chi2_scale;
  const CatDev* cats;
};

enum Mode : int { IMG_FWD = 0, IMG_BWD = 1, LL_FWD = 2, LL_GRAD = 3, IMG_BASIS = 4 };
constexpr int WG = 256;
constexpr int NSTAT = 4;  // accumulator row starts with [chi2, norm, pad, pad]

struct MainArgs {
  const CompDesc* comps;
  int n_lens, n_ll, n_src;
  const float* derived;  // [B][D]
  int D, A, Apad, ncols;
  const float* gx;
  const float* gy;
  const int* pix;  // may be null
  int N, chunk;
  float* img;         // IMG_FWD out  [B][img_stride]
  const float* gimg;  // IMG_BWD in   [B][img_stride]
  long long img_stride;
  float out_scale;  // multiplies the image (conversion factor when no PSF / pooling follows)
  const float* obs;
  const float* err;
  const float* mask;
  float bg2, inv_t;
  float* partial;  // [B][n_chunks][A]
  const float* shp_tab;
  int shp_stride;
  const int* order;  // cost-ordered dispatch: blockIdx.y -> sample index (heaviest first), or null
  // tapered end of the cost-ordered dispatch (pair kernels): the samples from rank tail_from on run as tail_rows workgroups each
  // (whole 512-pixel tiles dealt evenly) instead of gridDim.x chunks; every sample owns n_rows partial rows (tail_rows = 0: off)
  int tail_rows, tail_from, n_rows, n_samples;
  unsigned parts;    // forward-only partial renders (tf/simulator.py:242-328): bit0 deflect, bit1 lens light, bit2 sources
  // galaxy catalogues (K_SCALED): per-galaxy static blocks [G][DP_NS], per-(sample, galaxy) blocks [B][G][GM_ND]
  const CatDev* cats;
  const float* gal_static;
  const float* gal_dyn;
  int G;
  int scaled_first;  // the K_SCALED lens whose scale tangents ride along the ray-shooting pass (-1: none)
  int n_lin;         // IMG_BASIS: channels of the stack  img[B][n_lin][img_stride]
  const SeriesDev* series;
  const float* nfw_tab;  // models with NFW lenses: the shared h(X) table (gl_host_tables.h), [kNfwNodes][2]; else null
  const float* src_scale;  // per-source deflection scales c_s [n_src] (beta_s = x - c_s sum alpha), or null: one source plane
  const InterpDev* interp;  // image tables of the K_INTERPOL lights, or null: the model has none
  const InterpMassDev* interp_mass;  // deflection maps of the K_INTERPOL_MASS lenses, or null: the model has none
  const float* neutral;  // gl_clusterw_kernel: constant blocks of an unused component slot, [NFW (4) | Sersic (16)]; else null
  float grid_rmax;       // largest |(x, y)| of the pixel grid (gl_shp.hip.h: the bound on the shear's deflection)
  int blk_w;             // table-mode shapelet kernel: image width when a wave-tile is an 8-row x 16-column BLOCK of the image (0: 128 consecutive pixels)
  int careful_tiles;     // pair kernels (GIGALENS_HIP_CAREFUL_TILES, tests): whole tiles take the careful body, not the select-free one
  int dbg;  // -DGL_EXPERIMENTS builds only (GIGALENS_HIP_DBGFLAGS): 1 skip the pixel tiles, 2 skip the epilogue reductions, 4 skip the constant staging
};

// The work-skipping dissection knobs exist only in builds made with -DGL_EXPERIMENTS (never by __graft_entry__.build()):
// in the shipped library GL_DBG is a compile-time false and gl_model_create refuses the environment variables.
#ifdef GL_EXPERIMENTS
#define GL_DBG(flags, bit) (((flags) & (bit)) != 0)
#else
#define GL_DBG(flags, bit) false
#endif

// ---- wave64 sum, result valid in lane 63 (DPP row shifts + row broadcasts, no LDS) -------------
__device__ __forceinline__ float dpp_add(float v, int ctrl, int row_mask) {
  int r;
  switch (ctrl) {  // ctrl must be an immediate
    case 0x111: r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true); break;
    case 0x112: r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xF, 0xF, true); break;
    case 0x114: r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xF, 0xF, true); break;
    case 0x118: r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xF, 0xF, true); break;
    case 0x142: r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false); break;
    default: r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, false); break;
  }
  (void)row_mask;
  return v + __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float wave_sum63(float v) {
  v = dpp_add(v, 0x111, 0xF);  // row_shr:1
  v = dpp_add(v, 0x112, 0xF);  // row_shr:2
  v = dpp_add(v, 0x114, 0xF);  // row_shr:4
  v = dpp_add(v, 0x118, 0xF);  // row_shr:8   -> lane 15 of each row holds the row sum
  v = dpp_add(v, 0x142, 0xA);  // row_bcast:15 into rows 1,3
  v = dpp_add(v, 0x143, 0xC);  // row_bcast:31 into rows 2,3 -> lane 63 holds the wave sum
  return v;
}
// ---- per-tile accumulation of parameter-gradient partials ------------------------------------------
// A full wave64 reduction costs 12 VALU per value; doing it per (component, tile) dominated the
// instruction count.  Instead each value is summed over a QUAD (2 DPP adds, or over a 16-lane row with
// 4 when the model has too many accumulators for 64 LDS columns) and the quad/row leader adds it into
// its own LDS column: s_acc[col][k].  Columns are private to one lane group of one wave, so the
// read-modify-write needs no atomics and the result is order-deterministic.  The columns are summed
// once per workgroup at the end.  Apad is odd, so the 16 leader lanes of a wave hit 16 different banks.
__device__ __forceinline__ float quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));  // quad_perm:[1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));  // quad_perm:[2,3,0,1]
  return v;
}
// 4 x 4 transpose-reduction inside a quad: lane q of every quad receives  sum over the quad's lanes of v_q.
// Step 1 exchanges with lane ^ 1 (even lanes keep v0 / v2, odd lanes v1 / v3), step 2 with lane ^ 2.
__device__ __forceinline__ float dpp_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));  // quad_perm:[1,0,3,2]
}
__device__ __forceinline__ float dpp_xor2(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));  // quad_perm:[2,3,0,1]
}
__device__ __forceinline__ float quad_transpose_sum(float v0, float v1, float v2, float v3, bool odd, bool hi) {
  const float r01 = (odd ? v1 : v0) + dpp_xor1(odd ? v0 : v1);
  const float r23 = (odd ? v3 : v2) + dpp_xor1(odd ? v2 : v3);
  return (hi ? r23 : r01) + dpp_xor2(hi ? r01 : r23);
}

__device__ __forceinline__ float row_sum15(float v) {  // lane 15 of each 16-lane row holds the row sum
  v = dpp_add(v, 0x111, 0xF);
  v = dpp_add(v, 0x112, 0xF);
  v = dpp_add(v, 0x114, 0xF);
  v = dpp_add(v, 0x118, 0xF);
  return v;
}
struct AccCol {
  float* col;   // this lane group's LDS column
  bool leader;  // lane that owns the column
  bool quad;    // 64 columns (quad groups) or 16 columns (row groups)
};
__device__ __forceinline__ AccCol acc_col(float* s_acc, int Apad, int ncols, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  AccCol c;
  c.quad = ncols == 64;
  const int col = c.quad ? (wave * 16 + (lane >> 2)) : (wave * 4 + (lane >> 4));
  c.leader = c.quad ? ((lane & 3) == 0) : ((lane & 15) == 15);
  c.col = s_acc + col * Apad;
  return c;
}
// n <= G live accumulators (n is wave-uniform)
template <int G> __device__ __forceinline__ void wave_acc(float (&acc)[G], const AccCol& c, int off, int n = G) {
  if (c.quad) {
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (k < n) acc[k] = quad_sum(acc[k]);
  } else {
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (k < n) acc[k] = row_sum15(acc[k]);
  }
  if (c.leader) {
    float* dst = c.col + off;
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (k < n) dst[k] += acc[k];
  }
}

// ---- T-pixel EPL: series loop outermost so one LDS table read serves T pixels -------------------
template <int T> __device__ __forceinline__ void epl_fwd_T(const float* d, const float (&x)[T], const float (&y)[T],
                                                            float (&bx)[T], float (&by)[T]) {
  float Cs[T], Ss[T], twoc[T], Ex[T], Ey[T], Px[T], Py[T], Ox[T], Oy[T], Rc[T];
  const float c = d[EPL_C], s = d[EPL_S], q = d[EPL_Q];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float dx = x[t] - d[EPL_CX], dy = y[t] - d[EPL_CY];
    float xr = dx * c + dy * s, yr = dy * c - dx * s;
    float X = q * xr;
    float R0 = sqrt_(X * X + yr * yr);
    bool pos = R0 > 0.f;
    float inv = pos ? rcp(R0) : 0.f;
    Cs[t] = pos ? X * inv : 1.f;
    Ss[t] = yr * inv;
    Rc[t] = clamp_(R0, 1e-10f, 1e10f);
    twoc[t] = 2.f * (Cs[t] * Cs[t] - Ss[t] * Ss[t]);  // E_{n+1} = 2 cos(2 theta) E_n - E_{n-1}, see epl_fwd_v
    Ex[t] = Cs[t]; Ey[t] = Ss[t]; Px[t] = Cs[t]; Py[t] = -Ss[t]; Ox[t] = Cs[t]; Oy[t] = Ss[t];
  }
  const int K = (int)d[EPL_K];
  const float* tab = d + EPL_TAB;
  int n = 1;
  for (; n + 1 <= K; n += 2) {
    const float ca = tab[4 * n], cb = tab[4 * n + 4];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      Px[t] = twoc[t] * Ex[t] - Px[t];
      Py[t] = twoc[t] * Ey[t] - Py[t];
      Ox[t] += ca * Px[t];
      Oy[t] += ca * Py[t];
      Ex[t] = twoc[t] * Px[t] - Ex[t];
      Ey[t] = twoc[t] * Py[t] - Ey[t];
      Ox[t] += cb * Ex[t];
      Oy[t] += cb * Ey[t];
    }
  }
  if (n <= K) {
    const float ca = tab[4 * n];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      Ox[t] += ca * (twoc[t] * Ex[t] - Px[t]);
      Oy[t] += ca * (twoc[t] * Ey[t] - Py[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float L2 = log2_(d[EPL_B] * rcp(Rc[t]));
    float P = d[EPL_P0] * exp2_(d[EPL_TM1] * L2);
    float arx = P * Ox[t], ary = P * Oy[t];
    bx[t] -= arx * c - ary * s;
    by[t] -= arx * s + ary * c;
  }
}

template <int T> __device__ __forceinline__ void epl_vjp_T(const float* d, const float (&x)[T], const float (&y)[T],
                                                            const float (&gx)[T], const float (&gy)[T], float* acc) {
  float Cs[T], Ss[T], twoc[T], Ex[T], Ey[T], Px[T], Py[T], Ox[T], Oy[T], Fx[T], Fy[T], Tx[T], Ty[T];
  float xr[T], yr[T], inv[T], R0[T];
  const float c = d[EPL_C], s = d[EPL_S], q = d[EPL_Q];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float dx = x[t] - d[EPL_CX], dy = y[t] - d[EPL_CY];
    xr[t] = dx * c + dy * s;
    yr[t] = dy * c - dx * s;
    float X = q * xr[t];
    R0[t] = sqrt_(X * X + yr[t] * yr[t]);
    bool pos = R0[t] > 0.f;
    inv[t] = pos ? rcp(R0[t]) : 0.f;
    Cs[t] = pos ? X * inv[t] : 1.f;
    Ss[t] = yr[t] * inv[t];
    twoc[t] = 2.f * (Cs[t] * Cs[t] - Ss[t] * Ss[t]);
    Ex[t] = Cs[t]; Ey[t] = Ss[t]; Px[t] = Cs[t]; Py[t] = -Ss[t];
    Ox[t] = Cs[t]; Oy[t] = Ss[t];
    Fx[t] = 0.f; Fy[t] = 0.f; Tx[t] = 0.f; Ty[t] = 0.f;
  }
  const int K = (int)d[EPL_K];
  const float4* tab = reinterpret_cast<const float4*>(d + EPL_TAB);
  auto add = [&](const float4 cc, int t, float ex, float ey) {
    Ox[t] += cc.x * ex; Oy[t] += cc.x * ey;
    Fx[t] += cc.z * ex; Fy[t] += cc.z * ey;
    Tx[t] += cc.w * ex; Ty[t] += cc.w * ey;
  };
  int n = 1;
  for (; n + 1 <= K; n += 2) {
    const float4 ca = tab[n], cb = tab[n + 1];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      Px[t] = twoc[t] * Ex[t] - Px[t];
      Py[t] = twoc[t] * Ey[t] - Py[t];
      add(ca, t, Px[t], Py[t]);
      Ex[t] = twoc[t] * Px[t] - Ex[t];
      Ey[t] = twoc[t] * Py[t] - Ey[t];
      add(cb, t, Ex[t], Ey[t]);
    }
  }
  if (n <= K) {
    const float4 ca = tab[n];
#pragma unroll
    for (int t = 0; t < T; ++t) add(ca, t, twoc[t] * Ex[t] - Px[t], twoc[t] * Ey[t] - Py[t]);
  }
  const float tm1 = d[EPL_TM1], P0 = d[EPL_P0];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    bool inclamp = (R0[t] >= 1e-10f) && (R0[t] <= 1e10f);
    float iRc = rcp(clamp_(R0[t], 1e-10f, 1e10f));
    float L2 = log2_(d[EPL_B] * iRc);
    float W = exp2_(tm1 * L2);
    float P = P0 * W;
    float arx = P * Ox[t], ary = P * Oy[t];
    float ax = arx * c - ary * s, ay = arx * s + ary * c;
    float grx = gx[t] * c + gy[t] * s, gry = gy[t] * c - gx[t] * s;
    float g_phi = gy[t] * ax - gx[t] * ay;
    float gP = grx * Ox[t] + gry * Oy[t];
    float gOx = P * grx, gOy = P * gry;
    // S = sum (2n+1) c_n E_n = Omega + 2 f dOmega/df
    float g_ang = (gOy * Ox[t] - gOx * Oy[t]) + d[EPL_F2] * (gOy * Fx[t] - gOx * Fy[t]);
    float g_t = gOx * Tx[t] + gOy * Ty[t];
    float g_f = gOx * Fx[t] + gOy * Fy[t];
    float gW_W = gP * P;
    g_t += gW_W * (L2 * (float)kLn2);
    float g_b = gW_W * tm1 * d[EPL_INVB];
    float gR0 = inclamp ? -gW_W * tm1 * iRc : 0.f;
    float gX = gR0 * Cs[t] - g_ang * Ss[t] * inv[t];
    float gyr = gR0 * Ss[t] + g_ang * Cs[t] * inv[t];
    float g_q = gX * xr[t];
    float gxr = gX * q;
    float gdx = gxr * c - gyr * s, gdy = gxr * s + gyr * c;
    g_phi += gxr * yr[t] - gyr * xr[t];
    acc[EPLA_CX] -= gdx;
    acc[EPLA_CY] -= gdy;
    acc[EPLA_PHI] += g_phi;
    acc[EPLA_Q] += g_q;
    acc[EPLA_B] += g_b;
    acc[EPLA_T] += g_t;
    acc[EPLA_F] += g_f;
    acc[EPLA_P0] += gP * W;
  }
}

// ---- the main kernel ----------------------------------------------------------------------------
// SHP / FAM: the model contains shapelets / lenses of the extended families -- their code (and register budget) is
// compiled only into the variants that need it, so the common compositions keep their occupancy.
//   FAM 0: EPL, SIE, NFW, Shear, SIS | Sersic[Ellipse]     FAM 1: + dPIS / dPIE / dPIEP, catalogues, series lenses
//   FAM 2: + NFW_ELLIPSE, TNFW, CoreSersic (gl_extra.h; the fp64 core of TNFW alone costs ~80 VGPRs)
//   BIG: some shapelet component has n_max above SH_CAP (up to SH_CAPB = 20): every shapelet component of the model runs the
//   runtime-order code of gl_profiles.h on the model's wide table, amplitude gradients leave shell by shell into the LDS columns
// Where a light component is evaluated along one axis: the grid coordinate x for lens light, beta for a source -- on the source's
// own plane beta_s = x + c_s (beta - x) when the model carries per-source deflection scales (MainArgs::src_scale).  c_s == 1 takes
// beta as it stands (x + 1 (beta - x) is not beta in float32), so a model without scales computes exactly what it did before them;
// the cotangent of beta_s enters the lens VJPs as c_s times itself, which is exact at c_s == 1.  cs is wave-uniform.
__device__ __forceinline__ float light_point(bool src, float cs, float beta, float x) {
  return src ? (cs == 1.f ? beta : __builtin_fmaf(cs, beta - x, x)) : x;
}
// the scale of light component ci (lens lights and models without scales: 1)
__device__ __forceinline__ float light_scale(const MainArgs& a, int ci) {
  return (ci >= a.n_ll && a.src_scale) ? a.src_scale[ci - a.n_ll] : 1.f;
}
template <int MODE, int T, bool SHP, int FAM, bool BIG = false>
__global__ void __launch_bounds__(WG, (SHP || FAM) ? 2 : 4) gl_main_kernel(MainArgs a) {
  constexpr bool DP = FAM >= 1, XF = FAM >= 2;
  static_assert(!BIG || SHP, "BIG is a shapelet variant");
  extern __shared__ float smem[];
  float* s_d = smem;
  float* s_acc = smem + ((a.D + 3) & ~3);
  float* s_nfw = s_acc + a.ncols * a.Apad;  // models with NFW lenses: the shared h(X) table (8-byte aligned: ncols is even)
  const int tid = threadIdx.x;
  const int b = a.order ? a.order[blockIdx.y] : blockIdx.y, chunk = blockIdx.x;
  const CompDesc* __restrict__ comps = a.comps;
  {
    const float* src = a.derived + (size_t)b * a.D;
    for (int i = tid; i < a.D; i += WG) s_d[i] = src[i];
    if (a.nfw_tab)
      for (int i = tid; i < 2 * NFW_TAB_NODES; i += WG) s_nfw[i] = a.nfw_tab[i];
    if (MODE != IMG_FWD && MODE != IMG_BASIS)
      for (int i = tid; i < a.ncols * a.Apad; i += WG) s_acc[i] = 0.f;
  }
  __syncthreads();
  const AccCol ac = acc_col(s_acc, a.Apad, a.ncols, tid);
  const int n_lens = a.n_lens, n_light = a.n_ll + a.n_src, n_ll = a.n_ll;
  const int p0 = chunk * a.chunk;
  const int p1 = min(p0 + a.chunk, a.N);
  float st[2] = {0.f, 0.f};  // chi2, norm

  for (int base = p0; base < p1; base += WG * T) {
    float x[T], y[T], bx[T], by[T], m[T];
    int pidx[T];
    bool valid[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      int j = base + t * WG + tid;
      valid[t] = j < p1;
      int jj = valid[t] ? j : p1 - 1;
      x[t] = a.gx[jj];
      y[t] = a.gy[jj];
      pidx[t] = a.pix ? a.pix[jj] : jj;
      bx[t] = x[t]; by[t] = y[t]; m[t] = 0.f;
    }
    constexpr bool GRADMODE = (MODE == IMG_BWD || MODE == LL_GRAD);
    ScaleTan<v2f> tans[DP ? (T + 1) / 2 : 1];
    if constexpr (DP && GRADMODE) {
#pragma unroll
      for (int t = 0; t < (T + 1) / 2; ++t) tans[t] = ScaleTan<v2f>{v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f)};
    }
    // ---- phase 1: ray-shoot  beta = (x,y) - sum_i alpha_i(x,y)   (tf/simulator.py:72-78) ----
    for (int l = 0; l < ((a.parts & 1u) ? n_lens : 0); ++l) {
      const int kind = comps[l].kind;
      const float* d = s_d + comps[l].d_off;
      switch (kind) {
        case K_EPL: epl_fwd_T<T>(d, x, y, bx, by); break;
        case K_SIE:
#pragma unroll
          for (int t = 0; t < T; ++t) { float ax, ay; sie_fwd(d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          break;
        case K_NFW:
          if constexpr (T % 2 == 0) {  // pixel pairs -> packed fp32
#pragma unroll
            for (int t = 0; t < T; t += 2) {
              v2f vbx{bx[t], bx[t + 1]}, vby{by[t], by[t + 1]};
              nfw_fwd_v(d, s_nfw, v2f{x[t], x[t + 1]}, v2f{y[t], y[t + 1]}, vbx, vby);
              bx[t] = vbx.x; bx[t + 1] = vbx.y; by[t] = vby.x; by[t + 1] = vby.y;
            }
          } else {
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; nfw_fwd(d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_SHEAR:
#pragma unroll
          for (int t = 0; t < T; ++t) { float ax, ay; shear_fwd(d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          break;
        case K_SIS:
#pragma unroll
          for (int t = 0; t < T; ++t) { float ax, ay; sis_fwd(d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          break;
#ifdef GL_HAVE_USER  // run-time compiled variant of this kernel (gl_user.hip): the bodies of the model's user-written profiles
        case K_USER_MASS:
#pragma unroll
          for (int t = 0; t < T; ++t) { float ax, ay; glu::mass_fwd(comps[l].flags, d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          break;
#endif
        case K_DPIE:
          if constexpr (DP) {
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; piemd_fwd<float>(d, d + DP_NS, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_DPIS:
        case K_DPIEP:
          if constexpr (DP) {
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; piep_fwd<float>(d, d + DP_NS, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_NFW_ELLIPSE:
          if constexpr (XF) {
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; nfw_ell_fwd<float>(d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_TNFW:
          if constexpr (XF) {
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; tnfw_fwd<float>(d, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_INTERPOL_MASS:
          if constexpr (XF) {
            const InterpMassDev tb = a.interp_mass[comps[l].iparam];
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; interpmass_fwd<float>(d, tb, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_MULTIPOLE:
          if constexpr (XF) {
            const int m = comps[l].iparam;
#pragma unroll
            for (int t = 0; t < T; ++t) { float ax, ay; multipole_fwd<float>(d, m, x[t], y[t], ax, ay); bx[t] -= ax; by[t] -= ay; }
          }
          break;
        case K_SERIES: if constexpr (DP) {  // alpha = theta_E sum_n C_n(pixel) (r_cut - r0)^n   (series_profile.py:76-95)
          const SeriesDev sv = a.series[comps[l].flags];
          const float te = d[0], dl = d[1] - sv.r0;
          const size_t stn = (size_t)a.N;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const int j = base + t * WG + tid;
            const float* c = sv.coef + (j < p1 ? j : p1 - 1);
            float ax = c[(size_t)sv.order * stn], ay = c[(size_t)(2 * sv.order + 1) * stn];
            for (int n = sv.order - 1; n >= 0; --n) {
              ax = ax * dl + c[(size_t)n * stn];
              ay = ay * dl + c[(size_t)(sv.order + 1 + n) * stn];
            }
            bx[t] -= te * ax;
            by[t] -= te * ay;
          }
        } break;
        case K_SCALED: if constexpr (DP) {  // sum over the catalogue (scaling_relation.py:61-70), gl_members.hip.h
          const CatDev cat = a.cats[comps[l].iparam];
          const float* __restrict__ gs = a.gal_static + (size_t)cat.g_off * DP_NS;
          const float* __restrict__ gm = a.gal_dyn + ((size_t)b * a.G + cat.g_off) * GM_ND;
          const bool carry = GRADMODE && l == a.scaled_first;
#pragma unroll
          for (int t = 0; t < T; t += 2) {
            v2f vbx{bx[t], bx[t + 1]}, vby{by[t], by[t + 1]};
            const v2f vx{x[t], x[t + 1]}, vy{y[t], y[t + 1]};
            if (carry) members_v<v2f, true>(cat.base_kind, cat.n_gal, gs, gm, vx, vy, vbx, vby, tans[t / 2]);
            else members_v<v2f, false>(cat.base_kind, cat.n_gal, gs, gm, vx, vy, vbx, vby, tans[t / 2]);
            bx[t] = vbx.x; bx[t + 1] = vbx.y; by[t] = vby.x; by[t + 1] = vby.y;
          }
        } break;
      }
    }
    if constexpr (MODE == IMG_BASIS) {
      // lstsq_simulate (tf/simulator.py:183-201): every linear component as its own image, amplitude 1, NaN -> 0
      for (int ci = 0; ci < n_light; ++ci) {
        const CompDesc& cd = comps[n_lens + ci];
        const float* d = s_d + cd.d_off;
        const bool src = ci >= n_ll;
        const float cs = light_scale(a, ci);
        float* row = a.img + ((size_t)b * a.n_lin + cd.lin_off) * a.img_stride;
        if (cd.kind == K_SHAPELETS) {
          if constexpr (SHP) {
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
              if (!valid[t]) continue;
              const int pi = pidx[t];
              const long long st = a.img_stride;
              shapelets_basis<float, BIG ? SH_CAPB : SH_CAP>(d, a.shp_tab, a.shp_stride, cd.flags & 1u, light_point(src, cs, bx[t], x[t]),
                                             light_point(src, cs, by[t], y[t]), [&](int k, float v) { row[(size_t)k * st + pi] = isnan_(v) ? 0.f : v; });
            }
          }
        } else {
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const float px_ = light_point(src, cs, bx[t], x[t]), py_ = light_point(src, cs, by[t], y[t]);
            float v;
            if (XF && cd.kind == K_CORE_SERSIC) v = core_sersic_fwd<float>(d, px_, py_);
            else if (XF && cd.kind == K_INTERPOL) v = interp_fwd_unit<float>(d, a.interp[cd.iparam], cd.flags & 1u, px_, py_);  // amplitude 1
#ifdef GL_HAVE_USER
            else if (cd.kind == K_USER_LIGHT) v = glu::light_fwd(cd.flags, d, px_, py_);  // (its amplitude column holds 1, like a Sersic's)
#endif
            else v = sersic_fwd(d, px_, py_);
            if (valid[t]) row[pidx[t]] = isnan_(v) ? 0.f : v;
          }
        }
      }
      continue;
    }
    // ---- phase 2: render lens light at the grid, sources at beta (tf/simulator.py:128-138) ----
    for (int ci = 0; ci < n_light; ++ci) {
      const CompDesc& cd = comps[n_lens + ci];
      const float* d = s_d + cd.d_off;
      const bool src = ci >= n_ll;
      const float cs = light_scale(a, ci);
      if (!(a.parts & (src ? 4u : 2u))) continue;
      if (cd.kind == K_SHAPELETS) {
        if (SHP) {
          const bool interp = cd.flags & 1u;
          const float* __restrict__ gamp = a.derived + (size_t)b * a.D + cd.d_off + SHP_AMP;
#pragma unroll 1
          for (int t = 0; t < T; ++t) {
            if constexpr (BIG) {
              m[t] += shapelets_fwd<float, SH_CAPB>(d, a.shp_tab, a.shp_stride, interp, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]));
            } else {
              ShpState<SH_CAP> hs;
              m[t] += shp_fwd_state<SH_CAP>(d, gamp, a.shp_tab, interp, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]), hs);
            }
          }
        }
      } else if (cd.kind == K_CORE_SERSIC) {
        if constexpr (XF) {
#pragma unroll
          for (int t = 0; t < T; ++t) m[t] += core_sersic_fwd<float>(d, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]));
        }
      } else if (cd.kind == K_INTERPOL) {
        if constexpr (XF) {
          const InterpDev tb = a.interp[cd.iparam];
          const bool linear = cd.flags & 1u;
#pragma unroll
          for (int t = 0; t < T; ++t) m[t] += interp_fwd<float>(d, tb, linear, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]));
        }
#ifdef GL_HAVE_USER
      } else if (cd.kind == K_USER_LIGHT) {
#pragma unroll
        for (int t = 0; t < T; ++t) m[t] += glu::light_fwd(cd.flags, d, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]));
#endif
      } else if constexpr (T % 2 == 0) {
#pragma unroll
        for (int t = 0; t < T; t += 2) {
          SerStateV<v2f> stv;
          v2f I = sersic_fwd_v<v2f>(d, v2f{light_point(src, cs, bx[t], x[t]), light_point(src, cs, bx[t + 1], x[t + 1])},
                                    v2f{light_point(src, cs, by[t], y[t]), light_point(src, cs, by[t + 1], y[t + 1])}, stv);
          m[t] += I.x;
          m[t + 1] += I.y;
        }
      } else {
#pragma unroll
        for (int t = 0; t < T; ++t) m[t] += sersic_fwd(d, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]));
      }
    }
    bool nanp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      nanp[t] = isnan_(m[t]);
      m[t] = (nanp[t] ? 0.f : m[t]) * a.out_scale;  // NaN -> 0 (tf/simulator.py:140), then x det(T) (:156)
    }
    if (MODE == IMG_FWD) {
      float* row = a.img + (size_t)b * a.img_stride;
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (valid[t]) row[pidx[t]] = m[t];
      continue;
    }
    float gm[T];
    if (MODE == IMG_BWD) {
      const float* row = a.gimg + (size_t)b * a.img_stride;
#pragma unroll
      for (int t = 0; t < T; ++t) gm[t] = (valid[t] && !nanp[t]) ? row[pidx[t]] * a.out_scale : 0.f;
    } else {
      const bool has_err = a.err != nullptr;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        float o = a.obs[pidx[t]];
        float w = a.mask ? a.mask[pidx[t]] : 1.f;
        float e = has_err ? a.err[pidx[t]] : 1.f;
        float c2, nm;
        chi2_terms(m[t], o, w, has_err, e, a.bg2, a.inv_t, c2, nm);
        if (valid[t]) { st[0] += c2; st[1] += nm; }
        if (MODE == LL_GRAD)
          gm[t] = (valid[t] && !nanp[t]) ? chi2_gm(m[t], o, w, has_err, e, a.bg2, a.inv_t) * a.out_scale : 0.f;
      }
    }
    if (MODE == IMG_BWD || MODE == LL_GRAD) {
      float gbx[T], gby[T];
#pragma unroll
      for (int t = 0; t < T; ++t) { gbx[t] = 0.f; gby[t] = 0.f; }
      // ---- phase 3: light VJPs -> parameter gradients and the cotangent of beta ----
      for (int ci = 0; ci < n_light; ++ci) {
        const CompDesc& cd = comps[n_lens + ci];
        const float* d = s_d + cd.d_off;
        const bool src = ci >= n_ll;
        const float cs = light_scale(a, ci);
        if (cd.kind == K_SHAPELETS) {
          if constexpr (SHP && BIG) {
            // runtime-order path: one pixel at a time, every shell n = n1 + n2 of the amplitude gradient reduced over the lane
            // group and added to the LDS columns as soon as it is formed (at most SH_CAPB + 1 values live)
            const bool interp = cd.flags & 1u;
            float acc3[SHPA_AMP] = {0.f, 0.f, 0.f};
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
              float dgx = 0.f, dgy = 0.f;
              (void)shapelets_vjp_shells<float, SH_CAPB>(d, a.shp_tab, a.shp_stride, interp, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]),
                                                         gm[t], acc3, dgx, dgy, [&](int first, int count, float* vals) {
                float tmp[SH_CAPB + 1];
#pragma unroll
                for (int k = 0; k <= SH_CAPB; ++k) tmp[k] = vals[k];
                wave_acc<SH_CAPB + 1>(tmp, ac, cd.a_off + SHPA_AMP + first, count);
              });
              if (src) { gbx[t] += cs * dgx; gby[t] += cs * dgy; }
            }
            wave_acc<SHPA_AMP>(acc3, ac, cd.a_off, SHPA_AMP);
          } else if (SHP) {
            const bool interp = cd.flags & 1u;
            float acc[SHPA_AMP + SH_MAXL];
#pragma unroll
            for (int k = 0; k < SHPA_AMP + SH_MAXL; ++k) acc[k] = 0.f;
            const float* __restrict__ gamp = a.derived + (size_t)b * a.D + cd.d_off + SHP_AMP;
#pragma unroll 1
            for (int t = 0; t < T; ++t) {
              float dgx = 0.f, dgy = 0.f;
              ShpState<SH_CAP> hs;  // bases re-evaluated (the interpreter keeps no per-component state), contractions separable
              (void)shp_fwd_state<SH_CAP>(d, gamp, a.shp_tab, interp, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]), hs);
              shp_vjp_state<SH_CAP>(d, gamp, interp, hs, gm[t], acc, dgx, dgy);
              if (src) { gbx[t] += cs * dgx; gby[t] += cs * dgy; }
            }
            wave_acc<SHPA_AMP + SH_MAXL>(acc, ac, cd.a_off, cd.n_acc);
          }
#ifdef GL_HAVE_USER
        } else if (cd.kind == K_USER_LIGHT) {  // d I / d (x, y, p) from forward-mode duals of the user's body
          float acc[USER_MAXP];
#pragma unroll
          for (int k = 0; k < USER_MAXP; ++k) acc[k] = 0.f;
#pragma unroll
          for (int t = 0; t < T; ++t) {
            float dgx = 0.f, dgy = 0.f;
            glu::light_vjp(cd.flags, d, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]), gm[t], acc, dgx, dgy);
            if (src) { gbx[t] += cs * dgx; gby[t] += cs * dgy; }
          }
          wave_acc<USER_MAXP>(acc, ac, cd.a_off, cd.n_acc);
#endif
        } else if (cd.kind == K_CORE_SERSIC) {
          if constexpr (XF) {
            float acc[CSR_NACC];
#pragma unroll
            for (int k = 0; k < CSR_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              float dgx = 0.f, dgy = 0.f;
              core_sersic_vjp<float>(d, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]), gm[t], acc, dgx, dgy);
              if (src) { gbx[t] += cs * dgx; gby[t] += cs * dgy; }
            }
            wave_acc<CSR_NACC>(acc, ac, cd.a_off);
          }
        } else if (cd.kind == K_INTERPOL) {
          if constexpr (XF) {
            const InterpDev tb = a.interp[cd.iparam];
            const bool linear = cd.flags & 1u;
            float acc[INT_NACC];
#pragma unroll
            for (int k = 0; k < INT_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              float dgx = 0.f, dgy = 0.f;
              interp_vjp<float>(d, tb, linear, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]), gm[t], acc, dgx, dgy);
              if (src) { gbx[t] += cs * dgx; gby[t] += cs * dgy; }
            }
            wave_acc<INT_NACC>(acc, ac, cd.a_off);
          }
        } else {
          float acc[SER_NACC];
          if constexpr (T % 2 == 0) {
            v2f va[SER_NACC];
#pragma unroll
            for (int k = 0; k < SER_NACC; ++k) va[k] = v2f(0.f);
#pragma unroll
            for (int t = 0; t < T; t += 2) {
              SerStateV<v2f> stv;
              (void)sersic_fwd_v<v2f>(d, v2f{light_point(src, cs, bx[t], x[t]), light_point(src, cs, bx[t + 1], x[t + 1])},
                                      v2f{light_point(src, cs, by[t], y[t]), light_point(src, cs, by[t + 1], y[t + 1])}, stv);
              v2f dgx(0.f), dgy(0.f);
              sersic_vjp_v<v2f, true>(d, stv, v2f{gm[t], gm[t + 1]}, va, dgx, dgy);
              if (src) { gbx[t] += cs * dgx.x; gbx[t + 1] += cs * dgx.y; gby[t] += cs * dgy.x; gby[t + 1] += cs * dgy.y; }
            }
#pragma unroll
            for (int k = 0; k < SER_NACC; ++k) acc[k] = va[k].x + va[k].y;
            acc[SERA_INVN] *= (float)kLn2;  // sersic_vjp_v defers this factor
          } else {
#pragma unroll
            for (int k = 0; k < SER_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              float dgx = 0.f, dgy = 0.f;
              sersic_vjp(d, light_point(src, cs, bx[t], x[t]), light_point(src, cs, by[t], y[t]), gm[t], acc, dgx, dgy);
              if (src) { gbx[t] += cs * dgx; gby[t] += cs * dgy; }
            }
          }
          wave_acc<SER_NACC>(acc, ac, cd.a_off);
        }
      }
      // ---- phase 4: lens VJPs with cotangent -g_beta (beta = x - sum alpha) ----
#pragma unroll
      for (int t = 0; t < T; ++t) { gbx[t] = -gbx[t]; gby[t] = -gby[t]; }
      for (int l = 0; l < n_lens; ++l) {
        const CompDesc& cd = comps[l];
        const float* d = s_d + cd.d_off;
        switch (cd.kind) {
          case K_EPL: {
            float acc[EPL_NACC];
#pragma unroll
            for (int k = 0; k < EPL_NACC; ++k) acc[k] = 0.f;
            epl_vjp_T<T>(d, x, y, gbx, gby, acc);
            wave_acc<EPL_NACC>(acc, ac, cd.a_off);
          } break;
          case K_SIE: {
            float acc[SIE_NACC];
#pragma unroll
            for (int k = 0; k < SIE_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) sie_vjp(d, x[t], y[t], gbx[t], gby[t], acc);
            wave_acc<SIE_NACC>(acc, ac, cd.a_off);
          } break;
          case K_NFW: {
            float acc[NFW_NACC];
            if constexpr (T % 2 == 0) {
              v2f va[NFW_NACC];
#pragma unroll
              for (int k = 0; k < NFW_NACC; ++k) va[k] = v2f(0.f);
#pragma unroll
              for (int t = 0; t < T; t += 2)
                nfw_vjp_v(d, s_nfw, v2f{x[t], x[t + 1]}, v2f{y[t], y[t + 1]}, v2f{gbx[t], gbx[t + 1]}, v2f{gby[t], gby[t + 1]}, va);
#pragma unroll
              for (int k = 0; k < NFW_NACC; ++k) acc[k] = va[k].x + va[k].y;
            } else {
#pragma unroll
              for (int k = 0; k < NFW_NACC; ++k) acc[k] = 0.f;
#pragma unroll
              for (int t = 0; t < T; ++t) nfw_vjp(d, x[t], y[t], gbx[t], gby[t], acc);
            }
            wave_acc<NFW_NACC>(acc, ac, cd.a_off);
          } break;
          case K_SHEAR: {
            float acc[SHR_NACC];
            acc[0] = 0.f; acc[1] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) shear_vjp(d, x[t], y[t], gbx[t], gby[t], acc);
            wave_acc<SHR_NACC>(acc, ac, cd.a_off);
          } break;
          case K_SIS: {
            float acc[SIS_NACC];
            acc[0] = 0.f; acc[1] = 0.f; acc[2] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) sis_vjp(d, x[t], y[t], gbx[t], gby[t], acc);
            wave_acc<SIS_NACC>(acc, ac, cd.a_off);
          } break;
#ifdef GL_HAVE_USER
          case K_USER_MASS: {
            float acc[USER_MAXP];
#pragma unroll
            for (int k = 0; k < USER_MAXP; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) glu::mass_vjp(cd.flags, d, x[t], y[t], gbx[t], gby[t], acc);
            wave_acc<USER_MAXP>(acc, ac, cd.a_off, cd.n_acc);
          } break;
#endif
          case K_DPIS:
          case K_DPIE:
          case K_DPIEP: if constexpr (DP) {
            float acc[DP_NACC];
#pragma unroll
            for (int k = 0; k < DP_NACC; ++k) acc[k] = 0.f;
            if (cd.kind == K_DPIE) {
#pragma unroll
              for (int t = 0; t < T; ++t) piemd_vjp<float, true>(d, d + DP_NS, d + DPX_DE, x[t], y[t], gbx[t], gby[t], acc);
            } else {
#pragma unroll
              for (int t = 0; t < T; ++t) piep_vjp<float, true>(d, d + DP_NS, x[t], y[t], gbx[t], gby[t], acc);
            }
            wave_acc<DP_NACC>(acc, ac, cd.a_off);
          } break;
          case K_NFW_ELLIPSE: if constexpr (XF) {
            float acc[NFE_NACC];
#pragma unroll
            for (int k = 0; k < NFE_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) nfw_ell_vjp<float>(d, x[t], y[t], gbx[t], gby[t], acc);
            wave_acc<NFE_NACC>(acc, ac, cd.a_off);
          } break;
          case K_TNFW: if constexpr (XF) {
            float acc[TNF_NACC];
#pragma unroll
            for (int k = 0; k < TNF_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) tnfw_vjp<float>(d, x[t], y[t], gbx[t], gby[t], acc);
            wave_acc<TNF_NACC>(acc, ac, cd.a_off);
          } break;
          case K_INTERPOL_MASS: if constexpr (XF) {
            const InterpMassDev tb = a.interp_mass[cd.iparam];
            float acc[IM_NACC];
#pragma unroll
            for (int k = 0; k < IM_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              float ux = 0.f, uy = 0.f;  // (the cotangent of a grid point: unused)
              interpmass_vjp<float>(d, tb, x[t], y[t], gbx[t], gby[t], acc, ux, uy);
            }
            wave_acc<IM_NACC>(acc, ac, cd.a_off);
          } break;
          case K_MULTIPOLE: if constexpr (XF) {
            float acc[MPL_NACC];
#pragma unroll
            for (int k = 0; k < MPL_NACC; ++k) acc[k] = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              float ux = 0.f, uy = 0.f;  // (the cotangent of a grid point: unused)
              multipole_vjp<float>(d, cd.iparam, x[t], y[t], gbx[t], gby[t], acc, ux, uy);
            }
            wave_acc<MPL_NACC>(acc, ac, cd.a_off);
          } break;
          case K_SERIES: if constexpr (DP) {
            const SeriesDev sv = a.series[cd.flags];
            const float te = d[0], dl = d[1] - sv.r0;
            const size_t stn = (size_t)a.N;
            float acc[2] = {0.f, 0.f};
#pragma unroll
            for (int t = 0; t < T; ++t) {
              const int j = base + t * WG + tid;
              const float* c = sv.coef + (j < p1 ? j : p1 - 1);
              float ax = c[(size_t)sv.order * stn], ay = c[(size_t)(2 * sv.order + 1) * stn], dx = 0.f, dy = 0.f;
              for (int n = sv.order - 1; n >= 0; --n) {  // Horner with derivative
                dx = dx * dl + ax;
                dy = dy * dl + ay;
                ax = ax * dl + c[(size_t)n * stn];
                ay = ay * dl + c[(size_t)(sv.order + 1 + n) * stn];
              }
              acc[0] += gbx[t] * ax + gby[t] * ay;
              acc[1] += te * (gbx[t] * dx + gby[t] * dy);
            }
            wave_acc<2>(acc, ac, cd.a_off);
          } break;
          case K_SCALED: if constexpr (DP) {
            // gradient of the scales = cotangent . (tangents carried by the ray-shooting pass); a second catalogue in
            // the same model re-evaluates its members here
            float sc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < T; t += 2) {
              ScaleTan<v2f> tn = tans[t / 2];
              if (l != a.scaled_first) {
                const CatDev cat = a.cats[cd.iparam];
                tn = ScaleTan<v2f>{v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f), v2f(0.f)};
                v2f dbx(0.f), dby(0.f);
                members_v<v2f, true>(cat.base_kind, cat.n_gal, a.gal_static + (size_t)cat.g_off * DP_NS,
                                     a.gal_dyn + ((size_t)b * a.G + cat.g_off) * GM_ND, v2f{x[t], x[t + 1]},
                                     v2f{y[t], y[t + 1]}, dbx, dby, tn);
              }
              const v2f gx{gbx[t], gbx[t + 1]}, gy{gby[t], gby[t + 1]};
              sc[0] += hsum(gx * tn.tx + gy * tn.ty);
              sc[1] += hsum(gx * tn.cx + gy * tn.cy);
              sc[2] += hsum(gx * tn.ux + gy * tn.uy);
            }
            wave_acc<3>(sc, ac, cd.a_off);
          } break;
        }
      }
    }
  }
  if (MODE == IMG_FWD || MODE == IMG_BASIS) return;
  if (MODE == LL_FWD || MODE == LL_GRAD) wave_acc<2>(st, ac, 0);
  __syncthreads();
  float* out = a.partial + ((size_t)b * gridDim.x + chunk) * a.A;
  for (int k = tid; k < a.A; k += WG) {
    float v = 0.f;
    for (int j = 0; j < a.ncols; ++j) v += s_acc[j * a.Apad + k];
    out[k] = v;
  }
}

}  // namespace glk
