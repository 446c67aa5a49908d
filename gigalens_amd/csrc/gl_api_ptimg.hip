// gl_api_ptimg.hip -- the entry points of the point images in the pixel likelihood (gl_ptimg_*, gl_ptimg.hip.h).
#include "gl_host.hip.h"
#include "gl_ptimg.hip.h"

using namespace glk;

namespace {
struct PtLayout {
  int stride;  // floats of one column plane: the largest box
  size_t box, cols, bytes;
};
PtLayout pt_layout(const gl_model* m, int B, int J) {
  PtLayout l{};
  const int ss = m->supersample;
  l.stride = ((m->psf_h + 3 + ss - 1) / ss + 1) * ((m->psf_w + 3 + ss - 1) / ss + 1);
  l.box = 0;
  l.cols = align_up(sizeof(int) * 4 * (size_t)B * J, 256);
  l.bytes = l.cols + align_up(sizeof(float) * 3 * (size_t)l.stride * B * J, 256);
  return l;
}
// the checks that read no model: they come first, so that they answer without a device
int pt_sizes(const char* what, int B, int J) {
  if (J < 1 || J > PTI_MAX_J) return fail(GL_EINVAL, "%s: %d images per sample (1..%d)", what, J, PTI_MAX_J);
  if (B < 1 || B > 65535) return fail(GL_EINVAL, "%s: B = %d (1..65535)", what, B);
  return GL_OK;
}
// the model's side of a call: its workspace, carved, and the arguments every kernel shares
int pt_args(const gl_model* m, const char* what, const float* x, const float* y, const float* amp, int B, int J, const double* xf,
            void* workspace, size_t workspace_bytes, PtImgArgs* a) {
  if (int rp = refuse_planes(m, what)) return rp;
  if ((size_t)(m->psf_h + 4) * (m->psf_w + 4) > (size_t)PTI_MAX_TAB)
    return fail(GL_EUNSUPPORTED, "%s: a %d x %d PSF does not fit the kernels' table (%d floats with its apron)", what, m->psf_h,
                m->psf_w, PTI_MAX_TAB);
  const PtLayout lay = pt_layout(m, B, J);
  if (workspace_bytes < lay.bytes) return fail(GL_EINVAL, "%s: workspace too small: %zu < %zu bytes", what, workspace_bytes, lay.bytes);
  a->B = B; a->J = J;
  a->ss = m->supersample;
  a->H = m->height / a->ss; a->W = m->width / a->ss;
  a->kh = m->psf_h; a->kw = m->psf_w;
  a->stride = lay.stride;
  a->x0 = xf[0]; a->y0 = xf[1]; a->m00 = xf[2]; a->m01 = xf[3]; a->m10 = xf[4]; a->m11 = xf[5];
  a->tab = m->d_ptimg_tab;
  a->x = x; a->y = y; a->amp = amp;
  a->box = (int*)((char*)workspace + lay.box);
  a->cols = (float*)((char*)workspace + lay.cols);
  return GL_OK;
}
template <bool GRAD>
void pt_columns(const PtImgArgs& a, hipStream_t stream) {
  const size_t lds = sizeof(float) * (size_t)(a.kh + 4) * (a.kw + 4);
  hipLaunchKernelGGL(gl_ptimg_columns_kernel<GRAD>, dim3(a.J, a.B), dim3(PTI_COL_WG), lds, stream, a);
}
}  // namespace

extern "C" {

size_t gl_ptimg_workspace_bytes(const gl_model* m, int B, int n_images) {
  if (!m || B < 1 || B > 65535 || n_images < 1 || n_images > PTI_MAX_J) return 0;
  return pt_layout(m, B, n_images).bytes;
}

int gl_ptimg_render(const gl_model* m, const float* x, const float* y, const float* amplitude, int B, int n_images,
                    const double* transform, float* image, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !x || !y || !amplitude || !transform || !image || !workspace) return fail(GL_EINVAL, "gl_ptimg_render: null argument");
  if (int rc = pt_sizes("gl_ptimg_render", B, n_images)) return rc;
  PtImgArgs a{};
  if (int rc = pt_args(m, "gl_ptimg_render", x, y, amplitude, B, n_images, transform, workspace, workspace_bytes, &a)) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  pt_columns<false>(a, stream);
  hipLaunchKernelGGL(gl_ptimg_render_kernel, dim3((a.H * a.W + PTI_WG - 1) / PTI_WG, B), dim3(PTI_WG), 0, stream, a, image);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_ptimg_render_bwd(const gl_model* m, const float* x, const float* y, const float* amplitude, int B, int n_images,
                        const double* transform, const float* grad_image, float* grad_x, float* grad_y, float* grad_amplitude,
                        void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !x || !y || !amplitude || !transform || !grad_image || !grad_x || !grad_y || !grad_amplitude || !workspace)
    return fail(GL_EINVAL, "gl_ptimg_render_bwd: null argument");
  if (int rc = pt_sizes("gl_ptimg_render_bwd", B, n_images)) return rc;
  PtImgArgs a{};
  if (int rc = pt_args(m, "gl_ptimg_render_bwd", x, y, amplitude, B, n_images, transform, workspace, workspace_bytes, &a)) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  pt_columns<true>(a, stream);
  hipLaunchKernelGGL(gl_ptimg_adjoint_kernel, dim3(B), dim3(PTI_WG), 0, stream, a, grad_image, grad_amplitude, grad_x, grad_y);
  GL_HIP(hipGetLastError());
  return GL_OK;
}

int gl_ptimg_fit(const gl_model* m, const float* x, const float* y, int B, int n_images, const double* transform,
                 const float* extended_image, const float* observed, int observed_batched, const float* weight, int weight_batched,
                 int want_grad, float* amplitude, float* model_image, float* cotangent_image, double* chi2, int* ok, float* grad_x,
                 float* grad_y, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!m || !x || !y || !transform || !extended_image || !observed || !weight || !amplitude || !model_image || !cotangent_image ||
      !chi2 || !ok || !workspace || (want_grad && (!grad_x || !grad_y)))
    return fail(GL_EINVAL, "gl_ptimg_fit: null argument");
  if (int rc = pt_sizes("gl_ptimg_fit", B, n_images)) return rc;
  PtImgArgs a{};
  if (int rc = pt_args(m, "gl_ptimg_fit", x, y, amplitude, B, n_images, transform, workspace, workspace_bytes, &a)) return rc;
  PtFitArgs f{};
  const int HW = a.H * a.W;
  f.ext = extended_image;
  f.obs = observed; f.obs_stride = observed_batched ? HW : 0;
  f.weight = weight; f.weight_stride = weight_batched ? HW : 0;
  f.amp = amplitude; f.model = model_image; f.cot = cotangent_image; f.chi2 = chi2; f.ok = ok;
  f.gx = grad_x; f.gy = grad_y;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (want_grad) {
    pt_columns<true>(a, stream);
    hipLaunchKernelGGL(gl_ptimg_solve_kernel, dim3(B), dim3(PTI_WG), 0, stream, a, f);
    hipLaunchKernelGGL(gl_ptimg_residual_kernel<true>, dim3(B), dim3(PTI_WG), 0, stream, a, f);
  } else {
    pt_columns<false>(a, stream);
    hipLaunchKernelGGL(gl_ptimg_solve_kernel, dim3(B), dim3(PTI_WG), 0, stream, a, f);
    hipLaunchKernelGGL(gl_ptimg_residual_kernel<false>, dim3(B), dim3(PTI_WG), 0, stream, a, f);
  }
  GL_HIP(hipGetLastError());
  return GL_OK;
}

}  // extern "C"
