// gl_api_lstsq.hip -- the entry points of the linear-amplitude solve (gl_lstsq_*): basis stack or the stack-free shapelet kernel,
// normal matrices, Cholesky attempt, eigenvalue solve (gl_lstsq.hip.h, gl_shp.hip.h gl_shp_normal_kernel).
#include <algorithm>
#include <cstdio>

#include "gl_host.hip.h"
#include "gl_static.hip.h"
#include "gl_lstsq.hip.h"
#include "gl_shp.hip.h"

using namespace glk;

namespace {
struct LstsqWs {
  float *stack_ss, *stack, *partial, *coeffs;
  float* mats;  // [B][2][D][D | 1]: A and V of the eigen solve for systems above LS_LDS_MAXN unknowns (else null)
  int* todo;    // [B]: 1 = the Cholesky attempt left this system to the eigenvalue solve
  int chunk, n_chunks, Dp;
  int n_chunks_f;  // workgroups per sample of the stack-free kernel (gl_shp_normal_kernel: 512-pixel tiles dealt round-robin)
  size_t bytes;
};
// a kernel that asks for more than 64 KB of dynamic LDS (up to the CU's 160) has to be told once per process
int raise_lds_limit(const void* kernel, bool* raised) {
  if (!*raised) {
    GL_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    *raised = true;
  }
  return GL_OK;
}

// pixel chunks per sample of the normal-matrix kernels: ~`wgs` (2048) workgroups in flight, whole 64-pixel groups per chunk
void lstsq_chunks(long long HW, int B, int wgs, int* chunk, int* n_chunks) {
  long long want = std::max<long long>(1, ((long long)wgs + B - 1) / B);
  long long per = (HW + want - 1) / want;
  per = std::max<long long>(2 * LS_TPP, (per + 2 * LS_TPP - 1) / (2 * LS_TPP) * (2 * LS_TPP));
  *chunk = (int)per;
  *n_chunks = (int)((HW + per - 1) / per);
}

// (behind the call workspace `cw` of the same base)
LstsqWs carve_lstsq(const gl_model* m, int B, void* base, const Workspace& cw) {
  LstsqWs w{};
  size_t off = align_up(cw.bytes, 256);
  const int D = (int)m->lin_cols.size();
  const size_t HWs = (size_t)m->height * m->width, HW = HWs / ((size_t)m->supersample * m->supersample);
  char* p = (char*)base;
  auto take = [&](size_t n) { float* q = (float*)(p + off); off += align_up(n * sizeof(float), 256); return q; };
  w.Dp = (D + 1 + 3) & ~3;
  lstsq_chunks((long long)HW, B, m->lstsq_wgs, &w.chunk, &w.n_chunks);
  w.stack_ss = m->has_post ? take((size_t)B * D * HWs) : nullptr;
  w.stack = take((size_t)B * D * HW);
  // three workgroups per CU there: 1.5 x the workgroup target = four full rounds of the chip at the default (measured: 2048 ->
  // 0.708, 3072 -> 0.694, 4096 -> 0.697, 6144 -> 0.715 ms per C3L solve)
  w.n_chunks_f = (int)std::min<long long>(((long long)HW + 511) / 512, std::max<long long>(1, (3LL * m->lstsq_wgs / 2 + B - 1) / B));
  w.partial = take((size_t)B * std::max(w.n_chunks, w.n_chunks_f) * w.Dp * w.Dp);
  w.coeffs = take((size_t)B * D);
  w.mats = D > LS_LDS_MAXN ? take((size_t)B * 2 * D * (D | 1)) : nullptr;
  w.todo = (int*)take((size_t)B);
  w.bytes = off;
  return w;
}

// what the solve half of the linear-amplitude step needs of a workspace
struct SolveWs {
  float* partial;  // [B][n_chunks][Dp*Dp]
  float* mats;     // [B][2][D][D | 1] above LS_LDS_MAXN unknowns, else null
  int* todo;       // [B]
  int Dp, chunk, n_chunks;
};
// host function pointers of the most recent solve's normal-matrix, Cholesky and eigen kernel (null: the stage did not run)
std::atomic<const void*> g_lstsq_last_fn[3];
#define GL_LS_LAUNCH(slot_, kernel_, ...)                      \
  do {                                                         \
    g_lstsq_last_fn[slot_] = (const void*)&kernel_;            \
    hipLaunchKernelGGL((kernel_), __VA_ARGS__);                \
  } while (0)

// The solve of gl_lstsq_fwd and gl_lstsq_solve_stack: normal matrices of [stack / err | obs / err] per (sample, pixel chunk) --
// unless the stack-free kernel already left them (`have_partials`) --, their sum, the Cholesky attempt, the eigenvalue solve.
int lstsq_solve(const float* stack, const float* obs, const float* err, int B, int D, int HW, const SolveWs& sw,
                bool have_partials, bool chol, float* coeffs, hipStream_t stream) {
  int rc;
  NormalArgs na{};
  na.stack = stack;
  na.obs = obs;
  na.err = err;
  na.D = D;
  na.Dp = sw.Dp;
  na.HW = HW;
  na.chunk = sw.chunk;
  na.n_chunks = sw.n_chunks;
  na.partial = sw.partial;
  if (have_partials) {
    // the partials are already there
  } else if (D + 1 <= LS_SMALL)
    GL_LS_LAUNCH(0, gl_normal_small_kernel<LS_SMALL>, dim3(sw.n_chunks, B), dim3(256), 0, stream, na);
  else if (D + 1 > LS_MAXD) {  // more than five tile rows: super-block pairs (gl_normal_pair_kernel)
    const int vec_ok = (HW % 4 == 0) && ((uintptr_t)obs % 16 == 0) && ((uintptr_t)err % 16 == 0) && ((uintptr_t)stack % 16 == 0);
    const int n_sb = (D + 1 + 16 * LS_SB - 1) / (16 * LS_SB);
    const dim3 grid(sw.n_chunks, B, n_sb * (n_sb + 1) / 2), block(256);
    if (vec_ok) GL_LS_LAUNCH(0, gl_normal_pair_kernel<true>, grid, block, 0, stream, na);
    else GL_LS_LAUNCH(0, gl_normal_pair_kernel<false>, grid, block, 0, stream, na);
  } else {
    // 16-byte loads need every channel row, obs and err on a 16-byte pitch
    const int vec_ok = (HW % 4 == 0) && ((uintptr_t)obs % 16 == 0) && ((uintptr_t)err % 16 == 0) && ((uintptr_t)stack % 16 == 0);
    const dim3 grid(sw.n_chunks, B), block(256);
#define GL_NORMAL_MFMA(NT_)                                                                                  \
  if (vec_ok) GL_LS_LAUNCH(0, (gl_normal_mfma_kernel<NT_, true>), grid, block, 0, stream, na);               \
  else GL_LS_LAUNCH(0, (gl_normal_mfma_kernel<NT_, false>), grid, block, 0, stream, na)
    switch ((D + 1 + 15) / 16) {
      case 1: GL_NORMAL_MFMA(1); break;
      case 2: GL_NORMAL_MFMA(2); break;
      case 3: GL_NORMAL_MFMA(3); break;
      case 4: GL_NORMAL_MFMA(4); break;
      default: GL_NORMAL_MFMA(5); break;
    }
#undef GL_NORMAL_MFMA
  }
  GL_HIP(hipGetLastError());
  int n_sum = sw.n_chunks;
  if (n_sum > 8) {  // many chunks (small batches): reduce them with the whole chip first
    hipLaunchKernelGGL(gl_partial_sum_kernel, dim3((sw.Dp * sw.Dp + 255) / 256, B), dim3(256), 0, stream, sw.partial,
                       sw.n_chunks, sw.Dp * sw.Dp);
    GL_HIP(hipGetLastError());
    n_sum = 1;
  }
  const int* todo = nullptr;
  g_lstsq_last_fn[1] = nullptr;
  if (D <= LS_LDS_MAXN && chol) {  // the inverse when the pseudo-inverse's cut is provably idle (gl_chol_solve_kernel)
    const int nb = D + 1 <= 64 ? 4 : D + 1 <= 80 ? 5 : 8;
    const size_t sm = sizeof(float) * ((size_t)(D + 2) * (16 * nb + 1) + 4);
    static bool chol_raised = false;
    if (sm > 64 * 1024 && (rc = raise_lds_limit((const void*)&gl_chol_solve_kernel<8>, &chol_raised))) return rc;
#define GL_CHOL(NB_) GL_LS_LAUNCH(1, gl_chol_solve_kernel<NB_>, dim3(B), dim3(256), sm, stream, sw.partial, sw.n_chunks, n_sum, D, \
                                  sw.Dp, 1e-6f, coeffs, sw.todo)
    if (nb == 4) GL_CHOL(4); else if (nb == 5) GL_CHOL(5); else GL_CHOL(8);
#undef GL_CHOL
    GL_HIP(hipGetLastError());
    todo = sw.todo;
  }
  if (D <= LS_LDS_MAXN) {  // A and V in LDS: up to 129 KB of the CU's 160 (above 64 KB the kernel has to be told once)
    const size_t sm = sizeof(float) * ((size_t)2 * D * (D | 1) + 8 * D + 8);
    static bool eigh_raised = false;
    if (sm > 64 * 1024 && (rc = raise_lds_limit((const void*)&gl_eigh_solve_kernel<2, false>, &eigh_raised))) return rc;
    GL_LS_LAUNCH(2, (gl_eigh_solve_kernel<2, false>), dim3(B), dim3(64), sm, stream, sw.partial, sw.n_chunks, n_sum, D, sw.Dp,
                 1e-6f, coeffs, (float*)nullptr, todo);
  } else {  // the two matrices in the workspace (L2), the vectors in LDS; four registers hold the tridiagonal
    const size_t sm = sizeof(float) * ((size_t)8 * D + 8);
    GL_LS_LAUNCH(2, (gl_eigh_solve_kernel<4, true>), dim3(B), dim3(64), sm, stream, sw.partial, sw.n_chunks, n_sum, D, sw.Dp,
                 1e-6f, coeffs, sw.mats, todo);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

// the workspace of gl_lstsq_solve_stack: partials, the eigen solve's matrices above LS_LDS_MAXN unknowns, the flags
SolveWs carve_solve_stack(int B, int D, int HW, int wgs, void* base, size_t* bytes) {
  SolveWs w{};
  size_t off = 0;
  char* p = (char*)base;
  auto take = [&](size_t n) { float* q = (float*)(p + off); off += align_up(n * sizeof(float), 256); return q; };
  w.Dp = (D + 1 + 3) & ~3;
  lstsq_chunks((long long)HW, B, wgs, &w.chunk, &w.n_chunks);
  w.partial = take((size_t)B * w.n_chunks * w.Dp * w.Dp);
  w.mats = D > LS_LDS_MAXN ? take((size_t)B * 2 * D * (D | 1)) : nullptr;
  w.todo = (int*)take((size_t)B);
  *bytes = off;
  return w;
}

int check_solve_stack_shape(int B, int D, int HW, int workgroups) {
  if (B <= 0 || B > 65535) return fail(GL_EINVAL, "batch size %d outside [1, 65535]", B);
  if (D <= 0 || HW <= 0 || workgroups <= 0) return fail(GL_EINVAL, "D, HW and workgroups must be positive");
  if (D > LS_MAXN) return fail(GL_EUNSUPPORTED, "%d linear coefficients exceed the %d the solve serves", D, LS_MAXN);
  return GL_OK;
}
}  // namespace

extern "C" {

size_t gl_lstsq_solve_stack_workspace_bytes(int B, int D, int HW, int workgroups) {
  if (check_solve_stack_shape(B, D, HW, workgroups)) return 0;
  size_t bytes = 0;
  carve_solve_stack(B, D, HW, workgroups, nullptr, &bytes);
  return bytes;
}

int gl_lstsq_solve_stack(const float* stack, const float* obs, const float* err, int B, int D, int HW, int workgroups,
                         int cholesky, float* coeffs, int* flags_or_null, float* normal_or_null, void* workspace,
                         size_t workspace_bytes, void* hip_stream) {
  if (!stack || !obs || !err || !coeffs || !workspace) return fail(GL_EINVAL, "null argument");
  if (int rc = check_solve_stack_shape(B, D, HW, workgroups)) return rc;
  size_t bytes = 0;
  const SolveWs sw = carve_solve_stack(B, D, HW, workgroups, workspace, &bytes);
  if (workspace_bytes < bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  if (int rc = lstsq_solve(stack, obs, err, B, D, HW, sw, false, cholesky != 0, coeffs, stream)) return rc;
  if (flags_or_null) {  // no attempt: every system went to the eigenvalue solve
    if (cholesky && D <= LS_LDS_MAXN)
      GL_HIP(hipMemcpyAsync(flags_or_null, sw.todo, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, stream));
    else
      GL_HIP(hipMemsetD32Async((hipDeviceptr_t)flags_or_null, 1, (size_t)B, stream));
  }
  if (normal_or_null) {
    const int DpDp = sw.Dp * sw.Dp;
    // 2..8 chunks: the solve kernels summed the partials themselves; this pass repeats their additions in their order, so the
    // matrix handed out is a re-sum, bitwise equal to the values they consumed, not a copy of them
    if (sw.n_chunks > 1 && sw.n_chunks <= 8) {
      hipLaunchKernelGGL(gl_partial_sum_kernel, dim3((DpDp + 255) / 256, B), dim3(256), 0, stream, sw.partial, sw.n_chunks, DpDp);
      GL_HIP(hipGetLastError());
    }
    GL_HIP(hipMemcpy2DAsync(normal_or_null, sizeof(float) * DpDp, sw.partial, sizeof(float) * (size_t)sw.n_chunks * DpDp,
                            sizeof(float) * DpDp, (size_t)B, hipMemcpyDeviceToDevice, stream));
  }
  return GL_OK;
}

int gl_lstsq_last_kernels(char* normal, char* chol, char* eigen, size_t cap) {
  if (!normal || !chol || !eigen || cap == 0) return fail(GL_EINVAL, "bad argument");
  char* out[3] = {normal, chol, eigen};
  if (!g_lstsq_last_fn[2].load()) return fail(GL_EINVAL, "no linear solve has been launched in this process yet");
  for (int k = 0; k < 3; ++k) {
    const void* fn = g_lstsq_last_fn[k].load();
    const char* name = fn ? hipKernelNameRefByPtr(fn, nullptr) : "";
    if (!name) return fail(GL_ELAUNCH, "hipKernelNameRefByPtr returned no name");
    snprintf(out[k], cap, "%s", name);
  }
  return GL_OK;
}

size_t gl_lstsq_workspace_bytes(const gl_model* m, int B) {
  if (!m || B <= 0) return 0;
  return carve_lstsq(m, B, nullptr, carve(m, B, nullptr, launch_plan(m, B))).bytes;
}

int gl_lstsq_solve_flags(const gl_model* m, int B, size_t* offset_bytes) {
  if (!m || B <= 0 || !offset_bytes) return fail(GL_EINVAL, "bad argument");
  if ((int)m->lin_cols.size() > LS_LDS_MAXN || !m->lstsq_chol)
    return fail(GL_EUNSUPPORTED, "no Cholesky attempt for this model: every system goes through the eigenvalue solve");
  const LstsqWs lw = carve_lstsq(m, B, nullptr, carve(m, B, nullptr, launch_plan(m, B)));
  *offset_bytes = (size_t)((const char*)lw.todo - (const char*)nullptr);
  return GL_OK;
}

int gl_lstsq_fwd(const gl_model* m, const float* params, const float* obs, const float* err, int B, unsigned parts,
                 float* coeffs_or_null, float* stacked_or_null, float* image_or_null, void* workspace,
                 size_t workspace_bytes, void* hip_stream) {
  if (!m) return fail(GL_EINVAL, "model is null");
  if (int rp = refuse_planes(m, "gl_lstsq_fwd")) return rp;
  if (m->has_user && !m->user_fn[IMG_BASIS]) return fail(GL_EUNSUPPORTED, "the basis-stack kernel of this model with user-written profiles was not built");
  const int D = (int)m->lin_cols.size();
  if (D == 0) return fail(GL_EINVAL, "the model has no linear (light amplitude) coefficients");
  if (!params || !workspace) return fail(GL_EINVAL, "params / workspace is null");
  if (B <= 0 || B > 65535) return fail(GL_EINVAL, "batch size %d outside [1, 65535]", B);
  if (int rc = check_ready(m, true, false)) return rc;
  const bool solve = coeffs_or_null || image_or_null;
  if (solve && D > LS_MAXN)  // the basis stack alone (return_stacked) is served at any depth
    return fail(GL_EUNSUPPORTED, "%d linear coefficients exceed the %d the solve serves", D, LS_MAXN);
  if (solve && (!obs || !err)) return fail(GL_EINVAL, "obs / err_map are required to solve for the coefficients");
  if (!solve && !stacked_or_null) return fail(GL_EINVAL, "nothing to compute");
  if (!(parts & (GL_PART_LENS_LIGHT | GL_PART_SOURCE_LIGHT)) || parts > 7u) return fail(GL_EINVAL, "bad parts");
  const LaunchPlan plan = launch_plan(m, B);
  const Workspace w = carve(m, B, workspace, plan);
  LstsqWs lw = carve_lstsq(m, B, workspace, w);
  if (workspace_bytes < lw.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lw.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  const int chunk = plan.chunk, n_chunks = plan.n_chunks;
  int rc;
  const int HW = (m->height / m->supersample) * (m->width / m->supersample);
  // unit amplitudes -> derived constants -> basis stack
  hipLaunchKernelGGL(gl_unit_amplitudes_kernel, dim3((unsigned)(((long long)B * m->P + 255) / 256)), dim3(256), 0,
                     stream, params, m->P, B, m->d_lin_cols, D, w.params);
  GL_HIP(hipGetLastError());
  if ((rc = run_prep(m, w.params, nullptr, B, plan, w, stream))) return rc;
  MainArgs a = base_args(m, w, chunk);
  a.parts = parts | GL_PART_LENS_LIGHT | GL_PART_SOURCE_LIGHT;
  a.n_lin = D;
  if ((rc = run_order(m, B, w, &a, stream))) return rc;
  // One shapelet source as the only light component, no PSF / supersampling / pixel list, the stack not asked for: the normal
  // matrix straight from the bases (gl_shp_normal_kernel), no stack in HBM; a fitted image is rendered from the solved amplitudes
  const bool fused = solve && !stacked_or_null && !m->has_post && !m->d_pix && m->shp_kernel && m->static_id == ST_EPLSHEAR_SHAPELETS &&
                     m->n_ll == 0 && m->comps.back().iparam <= SH_CAP && D == sh_layers(m->comps.back().iparam) &&
                     (a.parts & (GL_PART_DEFLECT | GL_PART_SOURCE_LIGHT)) == (GL_PART_DEFLECT | GL_PART_SOURCE_LIGHT) &&
                     m->lstsq_fused;  // (a scaled source has static_id 0: the stack path, whose bases the interpreter renders at beta_s)
  if (fused) {
    lw.n_chunks = lw.n_chunks_f;
    const bool interp = (m->comps.back().flags & GL_FLAG_SHAPELETS_INTERPOLATE) != 0;
    constexpr int NPS = SH_SQ / 2;
    ShpNormalArgs sn{obs, err, lw.partial, D, lw.Dp};
    MainArgs fa = a;
    // (table mode on a whole image: 8 x 16 blocks of the image as wave-tiles, like gl_shp_kernel)
    fa.blk_w = (interp && m->shp_blocked && m->width % 16 == 0 && m->height % 8 == 0 && (long long)a.N == (long long)m->width * m->height) ? m->width : 0;
    const int nt = (D + 1 + 15) / 16;
    const size_t red = (size_t)(nt * (nt + 1) / 2 * 256 + 8) * sizeof(float);
    const size_t sh = (size_t)((m->D + 3) & ~3) * sizeof(float) +
                      std::max((size_t)4 * shn_wave_floats(NPS) * sizeof(float), red);
    const dim3 grid(lw.n_chunks, B), block(WG);
#define GL_SHPN(NT_, I_)                                                                                        \
  do {                                                                                                          \
    /* (table mode, five tile rows: 17 spilled VGPRs under the 128-register budget of four waves per SIMD since the live-pixel \
       list of round 4 -- three waves there) */                                                                  \
    m->last_main_fn = (const void*)&gl_shp_normal_kernel<NT_, ((I_ && NT_ < 5) ? 4 : 3), L_EplShear, NPS, I_>;              \
    g_lstsq_last_fn[0] = m->last_main_fn.load();                                                                \
    hipLaunchKernelGGL((gl_shp_normal_kernel<NT_, ((I_ && NT_ < 5) ? 4 : 3), L_EplShear, NPS, I_>), grid, block, sh, stream, fa, sn);  \
  } while (0)
    if (nt == 1) { if (interp) GL_SHPN(1, true); else GL_SHPN(1, false); }
    else if (nt == 2) { if (interp) GL_SHPN(2, true); else GL_SHPN(2, false); }
    else if (nt == 3) { if (interp) GL_SHPN(3, true); else GL_SHPN(3, false); }
    else if (nt == 4) { if (interp) GL_SHPN(4, true); else GL_SHPN(4, false); }
    else { if (interp) GL_SHPN(5, true); else GL_SHPN(5, false); }
#undef GL_SHPN
    GL_HIP(hipGetLastError());
  }
  float* target = m->has_post ? lw.stack_ss : lw.stack;
  if (!fused) {
  if (m->d_pix) GL_HIP(hipMemsetAsync(target, 0, sizeof(float) * (size_t)B * D * m->height * m->width, stream));
  a.img = target;
  if ((rc = launch_main<IMG_BASIS>(m, a, B, n_chunks, stream))) return rc;
  if (m->has_post && (rc = post_fwd(m, B * D, lw.stack_ss, lw.stack, stream, 1.f))) return rc;  // no det(T) here (:226-240)
  if (stacked_or_null)
    GL_HIP(hipMemcpyAsync(stacked_or_null, lw.stack, sizeof(float) * (size_t)B * D * HW, hipMemcpyDeviceToDevice, stream));
  }  // !fused
  if (!solve) return GL_OK;
  float* coeffs = coeffs_or_null ? coeffs_or_null : lw.coeffs;
  const SolveWs sw{lw.partial, lw.mats, lw.todo, lw.Dp, lw.chunk, lw.n_chunks};
  if ((rc = lstsq_solve(lw.stack, obs, err, B, D, HW, sw, fused, m->lstsq_chol, coeffs, stream))) return rc;
  if (image_or_null && fused) {
    // image = sum_d coeffs_d basis_d = the ordinary render with the solved amplitudes in their parameter columns (no det(T):
    // the stack carries none, tf/simulator.py:226-240)
    hipLaunchKernelGGL(gl_set_amplitudes_kernel, dim3((unsigned)(((long long)B * m->P + 255) / 256)), dim3(256), 0, stream,
                       params, m->P, B, m->d_lin_cols, D, coeffs, w.params);
    GL_HIP(hipGetLastError());
    if ((rc = run_prep(m, w.params, nullptr, B, plan, w, stream))) return rc;
    MainArgs ia = base_args(m, w, chunk);
    ia.parts = a.parts;
    ia.order = a.order;
    ia.img = image_or_null;
    ia.out_scale = 1.f;
    if ((rc = launch_main<IMG_FWD>(m, ia, B, n_chunks, stream))) return rc;
  } else if (image_or_null) {
    hipLaunchKernelGGL(gl_combine_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, stream, lw.stack, coeffs, D, HW,
                       image_or_null);
    GL_HIP(hipGetLastError());
  }
  return GL_OK;
}

#ifdef GL_EIGH_STAMPS
int gl_debug_eigh_stamps(long long* out) {
  GL_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(glk::g_eigh_stamps), sizeof(long long) * 8));
  return GL_OK;
}
#endif

}  // extern "C"
