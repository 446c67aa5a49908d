// gl_imgplane.hip.h -- the image-plane position likelihood of image families with its exact gradient (gl_imgplane_loglike;
// LensSimulator.image_plane_log_like_and_grad; beyond the reference, whose position term is the source-plane linearisation).
//
// Family f has J_f observed images theta^obs_j with one isotropic error sigma_j each and a deflection scale c_f:
//   beta(theta) = theta - c_f sum alpha(theta) ,  A(theta) = I - c_f H(theta)   (H with the dPIS excess, as img_lens_eval forms it).
// Its source beta_f is given, or the barycentre (1/J_f) sum_k beta(theta^obs_k).  The predicted image of observed image j is the
// root of beta(theta) = beta_f that Newton reaches from theta^obs_j -- the iteration of gl_img_newton_kernel with its polishing
// step, the step length limited to cap_j -- and is LOST when Newton has not converged after max_iter steps, the point is not
// finite, |theta_pred - theta^obs_j| > cap_j, or u_j below is not finite.  With r_j = theta_pred_j - theta^obs_j:
//   chi2_j = min(|r_j|^2, cap_j^2)/sigma_j^2  (a lost image sits at the cap) ,  log_like = -1/2 sum chi2_j - sum log(2 pi sigma_j^2) .
// Gradient by the implicit function theorem, nothing is differentiated through the iterations:  u_j = J(theta_pred_j)^-T r_j/sigma_j^2
// (0 for a lost image),
//   d log_like / d p = sum_j u_j . d beta/d p at theta_pred_j  -  (sum_{j in f} u_j) . d beta_f/d p .
// J = d beta / d theta = I - c_f d alpha / d theta is the derivative of the deflection ALONE: the reference's analytic dPIS Hessian adds
// a convergence excess that no deflection has (lens_kappa_excess), so A steers the Newton steps as it does in the solver -- the root
// does not depend on it -- while only J makes the gradient the derivative of the value.  Without a dPIS, J = A bit for bit.
//   I1  (image, sample): a lane each, the images of all families concatenated, sample fastest: the source (the barycentre is formed
//       by every lane of the family itself, J_f float evaluations in image order: siblings see the same bits without talking),
//       Newton on Dual<float,2>, then theta_pred (NaN when lost) into the point list, chi2_j, the lost flag and u_j
//   I2  (point, sample): the point list [n_pts][B] -- the predicted points I1 wrote, then the observed ones broadcast over the samples
//       when the source is the barycentre -- gets its cotangents on theta - sum alpha, [2][n_pts][B]: c_f u_j at a predicted point,
//       -(c_f/J_f) sum_{j in f} u_j (in image order) at an observed one
//   I3  (sample): one wave adds chi2_j, the norm and the lost flags, lane-strided then the tree, in float64; the first image of a
//       family writes -sum_{j in f} u_j as the gradient on an explicit source
// followed by V1 and V2 of gl_lens_vjp.hip.h on the list.  No atomics, no LDS of their own: every sum has a fixed order, two calls
// give identical bits and a sample reads nothing of another one.
// Included by gl_api_points.hip alone (not part of the run-time compile of user-written point kernels).
#pragma once
#include "gl_images.hip.h"
#include "gl_lens_vjp.hip.h"

namespace glk {

constexpr int IMGP_MAX_FAMILY = 64;  // images in one family: every lane of a family walks all of them for the barycentre

struct ImgPlaneArgs {
  const float* tab;      // [5][J] x, y, sigma, cap, deflection scale of every observed image
  const int* fam;        // [3][J] family, first image and image count of the family of every image
  const float* source;   // [2][B][F] explicit sources, or null: the barycentre of the back-traced observed images
  int J, F, max_iter;
  float tol;
  float* pts;       // [2][n_pts][B] the point list of the VJP: x then y (I1 fills the first J points)
  float* u;         // [2][J][B]
  float* chi2_j;    // [J][B]
  int* lost;        // [J][B]
  float* cot;       // [2][n_pts][B] or null: no gradient wanted
  long long n_pts;  // J (explicit sources) or 2 J
};

// beta and the Hessian of one point with the dPIS convergence excess kept apart: h is the derivative of the deflection, the Hessian
// of the maps is h + ex on f_xx and f_yy.  Always a
// function call, the device of crit_eval_cat in gl_critical.hip.h: inline, the Newton state beside the largest lens template (and
// the catalogue member loop in the switch of lens_point) does not fit the 256 VGPRs -- even the build without catalogues spilled 8.
static __device__ __attribute__((noinline)) void imgp_eval(const PosArgs& a, int b, float px, float py, float c, float& bx, float& by,
                                                           float* h, float& ex) {
  bx = px;
  by = py;
  h[0] = h[1] = h[2] = h[3] = ex = 0.f;
  lens_jets(a, b, px, py, [&](const CompDesc&, const float*, const Jet2& ax, const Jet2& ay, float e) {
    ex += e;
    bx -= ax.v;
    by -= ay.v;
    h[0] += ax.d[0]; h[1] += ax.d[1]; h[2] += ay.d[0]; h[3] += ay.d[1];
  });
  lens_rescale(c, px, py, bx, by, h);
  if (c != 1.f) ex *= c;
}

// beta alone (the back-traced observed images of the barycentre), always a function call: it stays out of the Newton loop's budget
static __device__ __attribute__((noinline)) float2 imgp_beta(const PosArgs& a, int b, float px, float py, float c) {
  float bx = px, by = py;
  lens_deflections(a, b, px, py, [&](const CompDesc&, const float*, float ax, float ay) {
    bx -= ax;
    by -= ay;
  });
  lens_rescale(c, px, py, bx, by);
  return float2{bx, by};
}

// grid: ceil(J B / 64) workgroups of one wave; lane = (image, sample), sample fastest
__global__ void __launch_bounds__(VJP_WG) gl_imgp_newton_kernel(PosArgs a, ImgPlaneArgs g) {
  const long long i = (long long)blockIdx.x * VJP_WG + threadIdx.x, total = (long long)g.J * a.B;
  const bool live = i < total;
  const int j = live ? (int)(i / a.B) : 0, b = live ? (int)(i - (long long)j * a.B) : 0;
  const float ox = g.tab[j], oy = g.tab[g.J + j], sg = g.tab[2 * g.J + j], cap = g.tab[3 * g.J + j], c = g.tab[4 * g.J + j];
  const int f = g.fam[j], first = g.fam[g.J + j], count = g.fam[2 * g.J + j];
  float sx = 0.f, sy = 0.f;
  if (live) {
    if (g.source) {
      sx = g.source[(size_t)b * g.F + f];
      sy = g.source[(size_t)a.B * g.F + (size_t)b * g.F + f];
    } else {
      for (int k = first; k < first + count; ++k) {
        const float2 bk = imgp_beta(a, b, g.tab[k], g.tab[g.J + k], c);
        sx += bk.x;
        sy += bk.y;
      }
      sx /= (float)count;
      sy /= (float)count;
    }
  }
  const float tol2 = g.tol * g.tol;
  // The iteration of gl_img_newton_kernel with one evaluation per pass: pass n evaluates the candidate (nx, ny) -- the observed
  // image at n = 0 --, which becomes the current point unless the pass is the polishing step (kept when its residual is not larger).
  // Steps until converged or max_iter of them are taken, then the one polishing step: at most max_iter + 2 passes, and the loop
  // ends when no lane of the wave is still iterating.
  float x = ox, y = oy, r_x = 0.f, r_y = 0.f, r2 = 0.f, h[4] = {0.f, 0.f, 0.f, 0.f}, ex = 0.f;
  float nx = ox, ny = oy;
  bool conv = false, ok = false, done = !live;
  for (int n = 0; n <= g.max_iter + 1; ++n) {
    if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
    if (done) continue;
    float nbx, nby, nh[4], nex;
    imgp_eval(a, b, nx, ny, c, nbx, nby, nh, nex);
    const float nr_x = sx - nbx, nr_y = sy - nby, nr2 = nr_x * nr_x + nr_y * nr_y;
    if (conv) {  // the polishing step
      if (nr2 <= r2) { x = nx; y = ny; ex = nex; for (int k = 0; k < 4; ++k) h[k] = nh[k]; }
      ok = true;
      done = true;
      continue;
    }
    x = nx; y = ny; r_x = nr_x; r_y = nr_y; r2 = nr2; ex = nex;
    for (int k = 0; k < 4; ++k) h[k] = nh[k];
    conv = r2 <= tol2;
    if (!conv && n == g.max_iter) { done = true; continue; }
    const float a00 = 1.f - (h[0] + ex), a01 = -h[1], a10 = -h[2], a11 = 1.f - (h[3] + ex);  // A: the excess included
    const float det = a00 * a11 - a01 * a10;
    float dx = (a11 * r_x - a01 * r_y) / det, dy = (a00 * r_y - a10 * r_x) / det;
    const float len = sqrtf(dx * dx + dy * dy);
    if (!(len <= cap)) {  // (also NaN)
      if (!isfinite(len)) { ok = conv; done = true; continue; }
      dx *= cap / len;
      dy *= cap / len;
    }
    nx = x + dx;
    ny = y + dy;
  }
  if (!live) return;
  const float a00 = 1.f - h[0], a01 = -h[1], a10 = -h[2], a11 = 1.f - h[3];
  const float det = a00 * a11 - a01 * a10;
  const float d_x = x - ox, d_y = y - oy, d2 = d_x * d_x + d_y * d_y, s2 = sg * sg;
  // u = J^-T r / sigma^2 (the derivative of the deflection alone)
  const float ux = ((a11 * d_x - a10 * d_y) / det) / s2, uy = ((a00 * d_y - a01 * d_x) / det) / s2;
  const bool lost = !(ok && isfinite(x) && isfinite(y) && d2 <= cap * cap && isfinite(ux) && isfinite(uy));
  const float nan = __builtin_nanf("");
  const long long st = g.n_pts * a.B, sj = total;
  g.pts[i] = lost ? nan : x;
  g.pts[st + i] = lost ? nan : y;
  g.chi2_j[i] = (lost ? cap * cap : fminf(d2, cap * cap)) / s2;
  g.lost[i] = lost ? 1 : 0;
  g.u[i] = lost ? 0.f : ux;
  g.u[sj + i] = lost ? 0.f : uy;
}

// grid: ceil(n_pts B / 64) workgroups of one wave; lane = (point, sample), sample fastest
__global__ void __launch_bounds__(VJP_WG) gl_imgp_cot_kernel(ImgPlaneArgs g, int B) {
  const long long i = (long long)blockIdx.x * VJP_WG + threadIdx.x, st = g.n_pts * B, sj = (long long)g.J * B;
  if (i >= st) return;
  const int pt = (int)(i / B), b = (int)(i - (long long)pt * B);
  if (pt < g.J) {  // a predicted point (x, y: I1)
    const float c = g.tab[4 * g.J + pt];
    g.cot[i] = c * g.u[i];
    g.cot[st + i] = c * g.u[sj + i];
    return;
  }
  const int k = pt - g.J;  // an observed point of a family with a barycentre source
  const int first = g.fam[g.J + k], count = g.fam[2 * g.J + k];
  float su_x = 0.f, su_y = 0.f;
  for (int j = first; j < first + count; ++j) {
    su_x += g.u[(long long)j * B + b];
    su_y += g.u[sj + (long long)j * B + b];
  }
  const float w = -g.tab[4 * g.J + k] / (float)count;
  g.pts[i] = g.tab[k];
  g.pts[st + i] = g.tab[g.J + k];
  g.cot[i] = w * su_x;
  g.cot[st + i] = w * su_y;
}

__device__ inline double imgp_wave_sum(double v) {
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// grid: B workgroups of one wave
__global__ void __launch_bounds__(VJP_WG) gl_imgp_sum_kernel(ImgPlaneArgs g, int B, float* __restrict__ ll, float* __restrict__ chi2,
                                                            int* __restrict__ n_lost, float* __restrict__ grad_source) {
  const int b = blockIdx.x;
  const long long sj = (long long)g.J * B;
  double c = 0.0, n = 0.0;
  int lost = 0;
  for (int j = threadIdx.x; j < g.J; j += VJP_WG) {
    const float sg = g.tab[2 * g.J + j];
    c += (double)g.chi2_j[(long long)j * B + b];
    n += (double)logf(6.283185307179586f * sg * sg);
    lost += g.lost[(long long)j * B + b];
    if (grad_source && g.fam[g.J + j] == j) {  // the first image of its family
      const int count = g.fam[2 * g.J + j], f = g.fam[j];
      float su_x = 0.f, su_y = 0.f;
      for (int k = j; k < j + count; ++k) {
        su_x += g.u[(long long)k * B + b];
        su_y += g.u[sj + (long long)k * B + b];
      }
      grad_source[(size_t)b * g.F + f] = -su_x;
      grad_source[(size_t)B * g.F + (size_t)b * g.F + f] = -su_y;
    }
  }
  c = imgp_wave_sum(c);
  n = imgp_wave_sum(n);
  for (int off = 32; off; off >>= 1) lost += __shfl_down(lost, off, 64);
  if (threadIdx.x == 0) {
    ll[b] = (float)(-0.5 * c - n);
    chi2[b] = (float)c;
    n_lost[b] = lost;
  }
}

}  // namespace glk
