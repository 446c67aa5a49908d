// gl_api_pixsrc.hip -- the entry points of the pixelated source reconstruction (gl_pixsrc_*, gl_pixsrc.hip.h).
#include <algorithm>

#include "gl_host.hip.h"
#include "gl_pixsrc.hip.h"

using namespace glk;

namespace {
constexpr size_t PIX_CHUNK_BUDGET = (size_t)256 << 20;  // operator, normal matrices and factors of one chunk of samples
constexpr size_t PIX_PLANE_BUDGET = (size_t)32 << 20;   // basis planes (supersampled and pooled) of one post-processing launch
constexpr int PIX_MAX_L_SLICE = 4;                      // factors held at once per sample
constexpr int PIX_MAX_PLANES = 4096;
struct PixLayout {
  int cb, lch, pc, n_pad;  // samples per chunk, strengths per slice, planes per post-processing launch
  size_t planes_ss, planes_lo, Fw, yw, A0, bvec, M, bytes;
};
PixLayout pix_layout(const gl_model* m, int B, int L, int S, int n_used) {
  PixLayout l{};
  const size_t HsWs = (size_t)m->height * m->width, HW = HsWs / ((size_t)m->supersample * m->supersample);
  l.n_pad = (n_used + PIX_TK - 1) / PIX_TK * PIX_TK;
  l.lch = std::min(L, PIX_MAX_L_SLICE);
  const size_t per_sample = sizeof(float) * ((size_t)S * l.n_pad + l.n_pad + (size_t)S * S * (1 + l.lch) + S);
  l.cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, PIX_CHUNK_BUDGET / per_sample));
  const size_t per_plane = sizeof(float) * ((m->has_post ? HsWs : 0) + HW);
  l.pc = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)l.cb * S, PIX_MAX_PLANES), PIX_PLANE_BUDGET / per_plane));
  l.planes_ss = 0;
  l.planes_lo = l.planes_ss + align_up(m->has_post ? sizeof(float) * (size_t)l.pc * HsWs : 0, 256);
  l.Fw = l.planes_lo + align_up(sizeof(float) * (size_t)l.pc * HW, 256);
  l.yw = l.Fw + align_up(sizeof(float) * (size_t)l.cb * S * l.n_pad, 256);
  l.A0 = l.yw + align_up(sizeof(float) * (size_t)l.cb * l.n_pad, 256);
  l.bvec = l.A0 + align_up(sizeof(float) * (size_t)l.cb * S * S, 256);
  l.M = l.bvec + align_up(sizeof(float) * (size_t)l.cb * S, 256);
  l.bytes = l.M + align_up(sizeof(float) * (size_t)l.cb * l.lch * S * S, 256);
  return l;
}
bool pix_sizes_ok(const gl_model* m, int B, int L, int ny, int nx, int n_used) {
  if (!m || B <= 0 || B > 65535 || L <= 0 || L > 65535 || ny <= 0 || nx <= 0 || (long long)ny * nx > PIX_MAX_S) return false;
  const long long HW = (long long)(m->height / m->supersample) * (m->width / m->supersample);
  return n_used > 0 && n_used <= HW;
}
// what a call reads and writes per sample, whole-batch pointers
struct PixIO {
  const float *beta_x, *beta_y, *obs, *sigma, *lens_light, *pose, *strength;
  float *source, *model;
  double* scal;
  int* ok;
};

// the forward launches of the chunk of samples b0 .. b0 + nb - 1 (gl_pixsrc.hip.h): operator, normal matrix, right-hand side, then
// solve and combine per slice of lch strengths.  Leaves `a` pointing at the chunk (and at its last slice of strengths).
int pix_forward_chunk(const gl_model* m, PixArgs& a, const PixIO& io, int b0, int nb, int L, int lch, int pc, float* planes_ss,
                      float* planes_lo, hipStream_t stream) {
  const int S = a.S, n_used = a.n_used, T = (S + PIX_TK - 1) / PIX_TK;
  a.B = nb;
  a.beta_x = io.beta_x + (size_t)b0 * a.HsWs;
  a.beta_y = io.beta_y + (size_t)b0 * a.HsWs;
  a.pose = io.pose + (size_t)b0 * 3;
  a.sigma = io.sigma + (size_t)b0 * n_used;
  a.obs = io.obs + (size_t)b0 * n_used;
  a.lens_light = io.lens_light ? io.lens_light + (size_t)b0 * a.HW : nullptr;
  // the operator, a launch of basis planes at a time
  for (int p0 = 0; p0 < nb * S; p0 += pc) {
    const int np = std::min(pc, nb * S - p0);
    hipLaunchKernelGGL(gl_pix_planes_kernel, dim3((a.HsWs + PIX_WG - 1) / PIX_WG, np), dim3(PIX_WG), 0, stream, a, p0,
                       m->has_post ? 1.f : m->conversion_factor, planes_ss);
    if (m->has_post)
      if (int rc = post_fwd(m, np, planes_ss, planes_lo, stream, m->conversion_factor)) return rc;
    hipLaunchKernelGGL(gl_pix_gather_kernel, dim3((a.n_pad + PIX_WG - 1) / PIX_WG, np), dim3(PIX_WG), 0, stream, a, p0, planes_lo);
  }
  hipLaunchKernelGGL(gl_pix_rhs_prep_kernel, dim3((a.n_pad + PIX_WG - 1) / PIX_WG, nb), dim3(PIX_WG), 0, stream, a);
  hipLaunchKernelGGL(gl_pix_normal_kernel, dim3(T * (T + 1) / 2, nb), dim3(PIX_WG), 0, stream, a);
  hipLaunchKernelGGL(gl_pix_rhs_kernel, dim3((S + PIX_WG / 64 - 1) / (PIX_WG / 64), nb), dim3(PIX_WG), 0, stream, a);
  for (int l0 = 0; l0 < L; l0 += lch) {
    const int nl = std::min(lch, L - l0);
    const size_t o = (size_t)b0 * L + l0;
    a.L = nl;
    a.strength = io.strength + o;
    a.source = io.source + o * S;
    a.model = io.model + o * a.HW;
    a.scal = io.scal + 3 * o;
    a.ok = io.ok + o;
    hipLaunchKernelGGL(gl_pix_solve_kernel, dim3(nb, nl), dim3(PIX_WG), 0, stream, a);
    hipLaunchKernelGGL(gl_pix_combine_kernel, dim3(nb, nl), dim3(PIX_WG), 0, stream, a);
  }
  return GL_OK;
}

// the gradient call: the forward workspace of one strength per sample, plus Z = M^-1 Fw and rw per sample and the inverse pixel map
struct PixGradLayout {
  int cb, pc, n_pad;  // samples per chunk, planes per post-processing launch
  size_t planes_ss, planes_lo, Fw, yw, A0, bvec, M, Z, rw, inv, bytes;
};
PixGradLayout pix_grad_layout(const gl_model* m, int B, int S, int n_used) {
  PixGradLayout l{};
  const size_t HsWs = (size_t)m->height * m->width, HW = HsWs / ((size_t)m->supersample * m->supersample);
  l.n_pad = (n_used + PIX_TK - 1) / PIX_TK * PIX_TK;
  const size_t per_sample = sizeof(float) * (2 * (size_t)S * l.n_pad + 2 * (size_t)l.n_pad + 2 * (size_t)S * S + S);
  l.cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, PIX_CHUNK_BUDGET / per_sample));
  const size_t per_plane = sizeof(float) * ((m->has_post ? HsWs : 0) + HW);
  l.pc = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)l.cb * S, PIX_MAX_PLANES), PIX_PLANE_BUDGET / per_plane));
  l.planes_ss = 0;
  l.planes_lo = l.planes_ss + align_up(m->has_post ? sizeof(float) * (size_t)l.pc * HsWs : 0, 256);
  l.Fw = l.planes_lo + align_up(sizeof(float) * (size_t)l.pc * HW, 256);
  l.yw = l.Fw + align_up(sizeof(float) * (size_t)l.cb * S * l.n_pad, 256);
  l.A0 = l.yw + align_up(sizeof(float) * (size_t)l.cb * l.n_pad, 256);
  l.bvec = l.A0 + align_up(sizeof(float) * (size_t)l.cb * S * S, 256);
  l.M = l.bvec + align_up(sizeof(float) * (size_t)l.cb * S, 256);
  l.Z = l.M + align_up(sizeof(float) * (size_t)l.cb * S * S, 256);
  l.rw = l.Z + align_up(sizeof(float) * (size_t)l.cb * S * l.n_pad, 256);
  l.inv = l.rw + align_up(sizeof(float) * (size_t)l.cb * l.n_pad, 256);
  l.bytes = l.inv + align_up(sizeof(int) * HW, 256);
  return l;
}
}  // namespace

extern "C" {

size_t gl_pixsrc_workspace_bytes(const gl_model* m, int B, int n_strength, int ny, int nx, int n_used) {
  if (!pix_sizes_ok(m, B, n_strength, ny, nx, n_used)) return 0;
  return pix_layout(m, B, n_strength, ny * nx, n_used).bytes;
}

int gl_pixsrc_layout(const gl_model* m, int B, int n_strength, int ny, int nx, int n_used, int32_t out[4]) {
  if (!out) return fail(GL_EINVAL, "null argument");
  if (!pix_sizes_ok(m, B, n_strength, ny, nx, n_used)) return fail(GL_EINVAL, "gl_pixsrc_layout: bad sizes");
  const PixLayout lay = pix_layout(m, B, n_strength, ny * nx, n_used);
  out[0] = lay.cb; out[1] = lay.lch; out[2] = lay.pc; out[3] = lay.n_pad;
  return GL_OK;
}

int gl_pixsrc_reconstruct(const gl_model* m, const float* beta_x, const float* beta_y, int B, const float* obs, const float* sigma,
                          const float* lens_light, const int* pix, int n_used, int ny, int nx, const float* pose, int regularization,
                          const float* strength, int n_strength, float* source, float* model_image, double* scalars, int* ok,
                          void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !beta_x || !beta_y || !obs || !sigma || !pix || !pose || !strength || !source || !model_image || !scalars || !ok)
    return fail(GL_EINVAL, "null argument");
  if (int rp = refuse_planes(m, "gl_pixsrc_reconstruct")) return rp;
  if (ny <= 0 || nx <= 0) return fail(GL_EINVAL, "source grid %d x %d: both sides must be positive", ny, nx);
  if ((long long)ny * nx > PIX_MAX_S) return fail(GL_EUNSUPPORTED, "source grid %d x %d has more than %d nodes", ny, nx, PIX_MAX_S);
  if (regularization < PIX_REG_IDENTITY || regularization > PIX_REG_CURVATURE) return fail(GL_EINVAL, "unknown regularization %d", regularization);
  if (!pix_sizes_ok(m, B, n_strength, ny, nx, n_used))
    return fail(GL_EINVAL, "bad sizes: B = %d, strengths = %d (both in 1..65535), used pixels = %d (1..H W)", B, n_strength, n_used);
  const int S = ny * nx, L = n_strength;
  const PixLayout lay = pix_layout(m, B, L, S, n_used);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  float* planes_lo = (float*)(base + lay.planes_lo);
  float* planes_ss = m->has_post ? (float*)(base + lay.planes_ss) : planes_lo;
  PixArgs a{};
  a.ny = ny; a.nx = nx; a.S = S;
  a.HsWs = m->height * m->width;
  a.HW = a.HsWs / (m->supersample * m->supersample);
  a.n_used = n_used; a.n_pad = lay.n_pad;
  a.reg = regularization;
  a.L_total = L;
  a.pix = pix;
  a.Fw = (float*)(base + lay.Fw);
  a.yw = (float*)(base + lay.yw);
  a.A0 = (float*)(base + lay.A0);
  a.bvec = (float*)(base + lay.bvec);
  a.M = (float*)(base + lay.M);
  const PixIO io{beta_x, beta_y, obs, sigma, lens_light, pose, strength, source, model_image, scalars, ok};
  for (int b0 = 0; b0 < B; b0 += lay.cb) {
    const int nb = std::min(lay.cb, B - b0);
    if (int rc = pix_forward_chunk(m, a, io, b0, nb, L, lay.lch, lay.pc, planes_ss, planes_lo, stream)) return rc;
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

size_t gl_pixsrc_grad_workspace_bytes(const gl_model* m, int B, int ny, int nx, int n_used) {
  if (!pix_sizes_ok(m, B, 1, ny, nx, n_used)) return 0;
  return pix_grad_layout(m, B, ny * nx, n_used).bytes;
}

int gl_pixsrc_grad_layout(const gl_model* m, int B, int ny, int nx, int n_used, int32_t out[3]) {
  if (!out) return fail(GL_EINVAL, "null argument");
  if (!pix_sizes_ok(m, B, 1, ny, nx, n_used)) return fail(GL_EINVAL, "gl_pixsrc_grad_layout: bad sizes");
  const PixGradLayout lay = pix_grad_layout(m, B, ny * nx, n_used);
  out[0] = lay.cb; out[1] = lay.pc; out[2] = lay.n_pad;
  return GL_OK;
}

int gl_pixsrc_evidence_grad(const gl_model* m, const float* beta_x, const float* beta_y, int B, const float* obs, const float* sigma,
                            const float* lens_light, const int* pix, int n_used, int ny, int nx, const float* pose, int regularization,
                            const float* strength, float* source, float* model_image, double* scalars, int* ok, float* grad_beta,
                            float* grad_image, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !beta_x || !beta_y || !obs || !sigma || !pix || !pose || !strength || !source || !model_image || !scalars || !ok ||
      !grad_beta || !grad_image)
    return fail(GL_EINVAL, "null argument");
  if (B <= 0 || n_used <= 0) return fail(GL_EINVAL, "bad sizes: B = %d, used pixels = %d: both must be positive", B, n_used);
  if (ny <= 0 || nx <= 0) return fail(GL_EINVAL, "source grid %d x %d: both sides must be positive", ny, nx);
  if (int rp = refuse_planes(m, "gl_pixsrc_evidence_grad")) return rp;
  if ((long long)ny * nx > PIX_MAX_S) return fail(GL_EUNSUPPORTED, "source grid %d x %d has more than %d nodes", ny, nx, PIX_MAX_S);
  if (regularization < PIX_REG_IDENTITY || regularization > PIX_REG_CURVATURE) return fail(GL_EINVAL, "unknown regularization %d", regularization);
  if (!pix_sizes_ok(m, B, 1, ny, nx, n_used))
    return fail(GL_EINVAL, "bad sizes: B = %d (1..65535), used pixels = %d (1..H W)", B, n_used);
  const int S = ny * nx;
  const PixGradLayout lay = pix_grad_layout(m, B, S, n_used);
  if (!workspace) return fail(GL_EINVAL, "workspace is null");
  if (workspace_bytes < lay.bytes) return fail(GL_ENOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, lay.bytes);
  hipStream_t stream = (hipStream_t)hip_stream;
  char* base = (char*)workspace;
  float* planes_lo = (float*)(base + lay.planes_lo);
  float* planes_ss = m->has_post ? (float*)(base + lay.planes_ss) : planes_lo;
  PixArgs a{};
  a.ny = ny; a.nx = nx; a.S = S;
  a.HsWs = m->height * m->width;
  a.HW = a.HsWs / (m->supersample * m->supersample);
  a.n_used = n_used; a.n_pad = lay.n_pad;
  a.reg = regularization;
  a.L_total = 1;
  a.pix = pix;
  a.Fw = (float*)(base + lay.Fw);
  a.yw = (float*)(base + lay.yw);
  a.A0 = (float*)(base + lay.A0);
  a.bvec = (float*)(base + lay.bvec);
  a.M = (float*)(base + lay.M);
  float* Z = (float*)(base + lay.Z);
  float* rw = (float*)(base + lay.rw);
  int* inv = (int*)(base + lay.inv);
  const PixIO io{beta_x, beta_y, obs, sigma, lens_light, pose, strength, source, model_image, scalars, ok};
  hipLaunchKernelGGL(gl_pix_inv_fill_kernel, dim3((a.HW + PIX_WG - 1) / PIX_WG), dim3(PIX_WG), 0, stream, a.HW, inv);
  hipLaunchKernelGGL(gl_pix_inv_set_kernel, dim3((n_used + PIX_WG - 1) / PIX_WG), dim3(PIX_WG), 0, stream, pix, n_used, a.HW, inv);
  for (int b0 = 0; b0 < B; b0 += lay.cb) {
    const int nb = std::min(lay.cb, B - b0);
    if (int rc = pix_forward_chunk(m, a, io, b0, nb, 1, 1, lay.pc, planes_ss, planes_lo, stream)) return rc;
    PixGradArgs g{};
    g.Z = Z; g.rw = rw; g.inv = inv;
    g.gbx = grad_beta + (size_t)b0 * a.HsWs;
    g.gby = grad_beta + ((size_t)B + b0) * a.HsWs;
    g.gimg = grad_image + (size_t)b0 * a.HW;
    hipLaunchKernelGGL(gl_pix_resid_kernel, dim3((a.n_pad + PIX_WG - 1) / PIX_WG, nb), dim3(PIX_WG), 0, stream, a, rw);
    hipLaunchKernelGGL(gl_pix_gimage_kernel, dim3((a.HW + PIX_WG - 1) / PIX_WG, nb), dim3(PIX_WG), 0, stream, a, g);
    hipLaunchKernelGGL(gl_pix_zsolve_kernel, dim3((a.n_pad + PIX_ZS_WG - 1) / PIX_ZS_WG, nb), dim3(PIX_ZS_WG), 0, stream, a, Z);
    // dE/dF a launch of planes at a time: scatter -> the model's transpose of PSF + pooling -> contraction with the hat derivatives
    for (int p0 = 0; p0 < nb * S; p0 += lay.pc) {
      const int np = std::min(lay.pc, nb * S - p0);
      hipLaunchKernelGGL(gl_pix_scatter_kernel, dim3((a.HW + PIX_WG - 1) / PIX_WG, np), dim3(PIX_WG), 0, stream, a, g, p0,
                         m->has_post ? 1.f : m->conversion_factor, planes_lo);
      if (m->has_post)
        if (int rc = post_bwd(m, np, planes_lo, planes_ss, stream, m->conversion_factor)) return rc;
      const int b_lo = p0 / S, b_hi = (p0 + np - 1) / S;
      hipLaunchKernelGGL(gl_pix_contract_kernel, dim3((a.HsWs + PIX_WG - 1) / PIX_WG, b_hi - b_lo + 1), dim3(PIX_WG), 0, stream, a, g,
                         b_lo, p0, np, (const float*)planes_ss);
    }
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
