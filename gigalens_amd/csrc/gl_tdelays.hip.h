// gl_tdelays.hip.h -- time-delay likelihood of the image families (beyond the reference, which has no such term).  Family f has
// observed images theta_j with beta_j = theta_j - sum alpha(theta_j), as the image-position likelihood traces them; its source is
// the barycentre  mean beta  over ALL its images, the one P2 compares against.  Images with a measured arrival time t_j (days,
// relative to any zero) and error s_j enter with weight w_j = 1 / s_j^2 (a NaN time: no measurement).  With the Fermat potential
//   phi_j = 1/2 |theta_j - mean beta|^2 - psi(theta_j)        (psi: lens_potential_point, gl_potential.hip.h; arcsec^2)
// and the w-weighted means  phi_bar, t_bar  over the measured images,  phi~ = phi - phi_bar,  t~ = t - t_bar,
//   lambda_f = the family's given scale (days / arcsec^2: D_dt c^-1 arcsec^2)   or, profiled out,   sum w t~ phi~ / sum w phi~^2
//   r_j = t~_j - lambda_f phi~_j ,  chi2_f = sum w r^2 ,  ll_f = -1/2 (chi2_f + sum log(2 pi s_j^2)) ,  T_f = t_bar - lambda_f phi_bar .
// T_f (the zero of the family's clock) minimises chi2_f, and so does a profiled lambda_f: the gradient is the partial derivative at
// fixed (lambda_f, T_f),
//   a_j = d ll / d phi_j = lambda_f w_j r_j ,   d ll / d mean beta = -sum a_j (theta_j - mean beta)   (1 / n_f of it to every image),
//   direct part  d ll / d p = -sum a_j d psi(theta_j; p) / d p .
// Only delay differences are constrained.  The term adds nothing to d ll / d det.
//
// Two kernels on the stream of the position likelihood:
//   gl_pos_tdelay_kernel       one thread per (sample, family), the thread that owns the same elements of w_fam and w_adj in P2 and
//                              in the flux kernel: alone it writes ll / chi2 and adj = (adj_x, adj_y, 0); `accumulate` (after P2
//                              and / or the flux kernel) it adds.  a_j goes to a scratch table [B][J] (0 for an image without a time).
//                              It traces beta_j and psi(theta_j) itself, on float64 (tdelay_trace_wide below: why).
//   gl_pos_tdelay_grad_kernel  after P3, before P4: one thread per (sample, image, lens-parameter column) adds -a_j d psi / d p to
//                              w_g, psi on Dual<float, 1> with the one direction seeded.  a_j == 0 exactly: nothing is touched.
// No atomics, a fixed order of operations: two calls give identical bits.  The delay tables and the scratch are kernel arguments of
// their own: PosArgs keeps the layout the run-time compiled point programs of user-written lenses were built against.
#pragma once
#include "gl_positions.hip.h"
#include "gl_potential.hip.h"

namespace glk {

// beta and psi of sample b at the image (x, y), summed over the lenses, in float64.  The term lives on DIFFERENCES of the Fermat
// potential between the images of a family, a tenth of psi and less, times a lambda_f of order 100 days / arcsec^2 against
// errors of a day or less: float32 rounding of psi (2e-7 arcsec^2) and of beta (1e-7 arcsec, which shifts phi_j by theta_j times
// that) is 2e-5 days of residual and moves a profiled lambda_f by 1e-6 -- and far more where a profile's float32 form cancels
// (the bracket of tnfw_g: 1e-5 of the deflection and of psi).  This path is tiny (a few images per thread), so the thread traces
// its family's images again with the profile templates on double instead of reading P1's float32 beta.  A function of its own:
// its registers are not held across the family's sums.
static __device__ __attribute__((noinline)) void tdelay_trace_wide(const PosArgs& a, int b, float xf, float yf, double& bx, double& by,
                                                                   double& psi) {
  const double x = (double)xf, y = (double)yf;
  bx = x;
  by = y;
  psi = 0.;
  for (int l = 0; l < a.n_lens; ++l) {
    const CompDesc cd = a.comps[l];
    double p[POS_MAXP];
    for (int k = 0; k < POS_MAXP; ++k) p[k] = k < cd.n_par ? (double)a.params[(size_t)b * a.P + cd.p_off + k] : 0.;
    double ax, ay;
    lens_point<double>(a, cd, p, x, y, ax, ay);
    bx -= ax;
    by -= ay;
    psi += lens_potential_point<double>(a, cd, p, x, y);
  }
}

// delay, delay_err [J] in the concatenated image order of the position tables, fam_scale [F] (lambda_f, NaN: profiled);
// aj [B][J]; scale, offset [B][F] (lambda_f, T_f) and model_delay [B][J] (lambda_f phi_j + T_f) or null
__global__ void __launch_bounds__(64) gl_pos_tdelay_kernel(PosArgs a, const float* __restrict__ delay, const float* __restrict__ delay_err,
                                                           const float* __restrict__ lam_given, int accumulate, float* __restrict__ aj,
                                                           float* __restrict__ scale, float* __restrict__ offset,
                                                           float* __restrict__ model_delay) {
  int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.B * a.F) return;
  int b = i / a.F, f = i - b * a.F;
  const int j0 = a.fam_off[f], j1 = a.fam_off[f + 1], nf = j1 - j0;
  float* tab = aj + (size_t)b * a.J;  // (psi_j - psi of the family's first image until the last pass writes a_j)
  const float two_pi = 6.283185307179586f;
  // pass 0: every image of the family traced in float64 -- the barycentre of ALL images, psi_j relative to the first image's
  // (a float32 slot holds the difference to 3e-8)
  double mbx = 0., mby = 0., psi0 = 0.;
  for (int j = j0; j < j1; ++j) {
    double bx, by, psi;
    tdelay_trace_wide(a, b, a.px[j], a.py[j], bx, by, psi);
    mbx += bx;
    mby += by;
    if (j == j0) psi0 = psi;
    tab[j] = (float)(psi - psi0);
  }
  mbx /= (double)nf;
  mby /= (double)nf;
  auto fermat = [&](int j) {
    const double dx = (double)a.px[j] - mbx, dy = (double)a.py[j] - mby;
    return 0.5 * (dx * dx + dy * dy) - ((double)tab[j] + psi0);
  };
  // pass 1: the weighted means.  All sums of this thread run in float64: the residuals then sum to zero under their weights as T_f
  // demands, and what the images' d psi / d p have in common (all of it for a distant catalogue member) cannot leak into the
  // gradient through a remainder.
  double sw = 0., swp = 0., swt = 0.;
  float norm = 0.f;
  int n = 0;
  for (int j = j0; j < j1; ++j) {
    const float t = delay[j];
    if (t != t) continue;
    const float s = delay_err[j];
    const double wt = 1. / ((double)s * (double)s);
    sw += wt;
    swp += wt * fermat(j);
    swt += wt * (double)t;
    norm += logf(two_pi * s * s);
    ++n;
  }
  const double pbar = swp / sw, tbar = swt / sw;  // (a family without delays: 0 / 0, the NaN its optional outputs report)
  double lam = (double)lam_given[f];
  if (lam != lam) {
    double stp = 0., spp = 0.;
    for (int j = j0; j < j1; ++j) {
      const float t = delay[j];
      if (t != t) continue;
      const float s = delay_err[j];
      const double wt = 1. / ((double)s * (double)s), pc = fermat(j) - pbar;
      stp += wt * ((double)t - tbar) * pc;
      spp += wt * pc * pc;
    }
    lam = stp / spp;
  }
  if (!n) lam = (double)__builtin_nanf("");
  if (scale) scale[(size_t)b * a.F + f] = (float)lam;
  if (offset) offset[(size_t)b * a.F + f] = (float)(tbar - lam * pbar);
  if (model_delay)
    for (int j = j0; j < j1; ++j) model_delay[(size_t)b * a.J + j] = (float)(tbar + lam * (fermat(j) - pbar));
  // pass 3: residuals, chi2, a_j and the adjoint of the barycentre
  double chi2d = 0., gxd = 0., gyd = 0.;
  for (int j = j0; j < j1; ++j) {
    const float t = delay[j];
    float aw = 0.f;
    if (t == t) {
      const float s = delay_err[j];
      const double wt = 1. / ((double)s * (double)s);
      const double r = ((double)t - tbar) - lam * (fermat(j) - pbar);
      chi2d += wt * r * r;
      const double ad = lam * wt * r;
      gxd -= ad * ((double)a.px[j] - mbx);
      gyd -= ad * ((double)a.py[j] - mby);
      aw = (float)ad;
    }
    tab[j] = aw;
  }
  const float chi2 = (float)chi2d;
  float gx = (float)gxd, gy = (float)gyd;
  float* fam = a.w_fam + ((size_t)b * a.F + f) * 2;
  const float ll = n ? -0.5f * (chi2 + norm) : 0.f;
  if (!accumulate) {
    fam[0] = ll;
    fam[1] = chi2;
  } else if (n) {  // (a family without delays keeps the bits of the kernels before)
    fam[0] += ll;
    fam[1] += chi2;
  }
  if (!a.grad) return;
  gx /= (float)nf;
  gy /= (float)nf;
  for (int j = j0; j < j1; ++j) {
    float* o = a.w_adj + ((size_t)b * a.J + j) * 3;
    if (!accumulate) {
      o[0] = gx;
      o[1] = gy;
      o[2] = 0.f;
    } else if (n) {
      o[0] += gx;
      o[1] += gy;
    }
  }
}

// d psi / d (the seeded parameter) of lens cd.  Outlined: the TNFW quadrature on duals stays in registers as a function of its own.
// The TNFW runs on Dual<double, 1>: the adjoints a_j of a family sum to zero, so what the images' d psi / d p have in common
// cancels, and the float32 bracket of tnfw_g leaves d psi / d r_trunc (a column of small scale) too few digits for that.
template <class R1> static __device__ __attribute__((noinline)) float tdelay_dpsi(const PosArgs& a, const CompDesc& cd, const R1* p, float x, float y) {
  if (cd.kind == glp::K_TNFW) {
    using W = gld::Dual<double, 1>;
    W pw[5], d[glp::TNF_ND];
    for (int m = 0; m < 5; ++m) {
      pw[m].v = (double)p[m].v;
      pw[m].d[0] = (double)p[m].d[0];
    }
    glp::tnfw_prep<W>(pw, d);
    return (float)glp::tnfw_pot<W>(d, W((double)x), W((double)y)).d[0];
  }
  return lens_potential_point<R1>(a, cd, p, R1(x), R1(y)).d[0];
}

__global__ void __launch_bounds__(64) gl_pos_tdelay_grad_kernel(PosArgs a, const float* __restrict__ aj, int lens_params) {
  int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.B * a.J * lens_params) return;
  const int col = i % lens_params, bj = i / lens_params;
  const int b = bj / a.J, j = bj - b * a.J;
  const float aw = aj[(size_t)b * a.J + j];
  if (aw == 0.f) return;  // (no measured time: P3's bits stay)
  int l = 0;  // (lens_seeded_column, spelled out as in gl_pos_p3_kernel, for the same reason)
  while (l + 1 < a.n_lens && col >= a.comps[l + 1].p_off) ++l;
  const CompDesc cd = a.comps[l];
  const int k = col - cd.p_off;
  using R1 = gld::Dual<float, 1>;
  R1 p[POS_MAXP];
  for (int m = 0; m < POS_MAXP; ++m) {
    R1 v(m < cd.n_par ? a.params[(size_t)b * a.P + cd.p_off + m] : 0.f);
    if (m == k) v.d[0] = 1.f;
    p[m] = v;
  }
  a.w_g[((size_t)b * a.J + j) * a.P + col] -= aw * tdelay_dpsi<R1>(a, cd, p, a.px[j], a.py[j]);
}

}  // namespace glk
