// gl_multiplane_fermat.hip.h -- arrival times on lens planes (gl_multiplane.hip.h): the multi-plane Fermat potential
//   T(theta; beta_s) = sum_{i<Ks} [ g_si |theta_i - theta_next(i)|^2 / 2 - v_i psi_i(theta_i) ]        (gl_mp_delay.h)
// of rays that leave the observer at given points theta (the images gl_multiplane_image_positions returned, or any points) towards
// sources that each sit on a plane of their own (gl_multiplane_fermat; LensSimulator.time_delays(source_redshifts=...) and
// fermat_potential(source_redshift=...)).  An evaluation, not a search: every lens is evaluated wherever the ray meets its plane
// (MpSkipNone's rule), and whatever is not finite propagates to the result.
//
// One kernel, one thread per (sample, source, point) in the order of the arrays [B][n_src][M] -- the point index runs fastest,
// so a wave reads and writes consecutive addresses; the lens list is the model's, the same for every lane.  The thread walks the
// lenses in plane order as mp_trace does and adds psi of a lens where its deflection is evaluated, at the ray's position on the
// lens's plane.  Everything is on double (tdelay_trace_wide of gl_tdelays.hip.h: the same reasons): delays are differences of T a
// tenth of its terms and less, and the weights turn 1e-6 arcsec^2 into tens of days.  The 3 MP_MAXK running sums are registers
// (MpDelayState: constant indices only); the kernel has no private segment.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_mp_delay.h"
#include "gl_multiplane.hip.h"
#include "gl_potential.hip.h"

namespace glk {

constexpr int MP_FERMAT_WG = 64;

struct MpFermatArgs {
  const float* x;       // [B][n_src][M] points; NaN = no point (the solver's padding)
  const float* y;
  const float* src_x;   // [B][n_src]
  const float* src_y;
  const double* geom;   // [n_src][K] g_si, 0 from the first plane at or behind the source on
  const double* pot;    // [K] v_i
  int n_src, M, K;
  double* out;          // [B][n_src][M]
};

__global__ void __launch_bounds__(MP_FERMAT_WG) gl_mp_fermat_kernel(PosArgs a, MpArgs mp, MpFermatArgs q) {
  const long long i = (long long)blockIdx.x * MP_FERMAT_WG + threadIdx.x;
  const long long SM = (long long)q.n_src * q.M;
  if (i >= SM * a.B) return;
  const int b = (int)(i / SM);
  const long long bs = i / q.M;  // (sample, source)
  const int s = (int)(bs - (long long)b * q.n_src);
  const double tx = (double)q.x[i], ty = (double)q.y[i];
  glp::MpDelayState<MP_MAXK> st;
  for (int t = 0; t < a.n_lens; ++t) {
    const int l = mp.order[t], pl = mp.plane[l];
    const CompDesc cd = a.comps[l];
    double x = tx, y = ty;
    st.to_plane(pl, mp.scale, x, y);
    double p[POS_MAXP];
#pragma unroll
    for (int k = 0; k < POS_MAXP; ++k) p[k] = k < cd.n_par ? (double)a.params[(size_t)b * a.P + cd.p_off + k] : 0.;
    double ax, ay;
    lens_point<double, false>(a, cd, p, x, y, ax, ay);
    st.add(pl, ax, ay, lens_potential_point<double, false>(a, cd, p, x, y));
  }
  const double T = st.arrival(mp.scale, tx, ty, (double)q.src_x[bs], (double)q.src_y[bs], q.geom + (size_t)s * q.K, q.pot, q.K,
                              nullptr);
  q.out[i] = isfinite(T) ? T : (double)__builtin_nanf("");  // (inf of either sign is no arrival time)
}

}  // namespace glk
