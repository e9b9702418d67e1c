// The Matern-3/2 covariance of the two plain fp64 paths (oi_nystrom.hip; the
// dense path's oi_predict.hip, oi_sample.hip and oi_grad.hip, which also share
// stage_tile below) as SGPkernel writes it (GPR_CS2S3.py, GPR:83-93).  Every
// expression keeps numpy's operation order; no FMA contraction.  The main
// engine (oi_kernels.hip, -ffp-contract=fast) and SVGP (another algebraic
// form) have their own code and do not use this file.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

constexpr double SQRT3 = 1.7320508075688772;  // np.sqrt(3.)

// np.sqrt(3.) * x / ell: the scaled coordinate whose 3-D distance is Q
__device__ inline double matern_scale(double x, double ell) { return (SQRT3 * x) / ell; }
// np.sqrt(3.) * (x / ell): the per-dimension q_d of dK (Nystrom gradient)
__device__ inline double matern_scale_q(double x, double ell) { return SQRT3 * (x / ell); }

// Q from the differences of two scaled rows (scipy pdist / cdist 'euclidean')
__device__ inline double matern_dist(double d0, double d1, double d2) {
  return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

// sf2 (1 + Q) exp(-Q)
__device__ inline double matern32(double sf2, double d0, double d1, double d2) {
  const double Q = matern_dist(d0, d1, d2);
  return sf2 * ((1.0 + Q) * exp(-Q));
}

// c_k = np.sqrt(3.) / ell_k: the derivative of a scaled coordinate
__device__ inline double matern_c(double ell) { return SQRT3 / ell; }

// The covariance and its derivatives from Q and e = exp(-Q), computed once per
// pair (oi_grad.hip).  matern32_qe is matern32's own expression, so its values
// are matern32's bit for bit.  With c_k = np.sqrt(3.) / ell_k and d = the
// scaled a minus the scaled b:
//   d k / d a_k        = -sf2 e d_k c_k   matern32_d1(sf2, e, -d_k, c_k)
//   d k / d b_l        = +sf2 e d_l c_l   matern32_d1(sf2, e, d_l, c_l)
//   d2 k / d a_k d b_l = sf2 e c_k c_l ((k == l) - d_k d_l / Q), the quotient 0 at Q = 0
// No division by Q in the first derivatives, so they are +0 at Q = 0 (the
// caller forms -d_k as the scaled b minus the scaled a, never as a negation).
__device__ inline double matern32_qe(double sf2, double Q, double e) { return sf2 * ((1.0 + Q) * e); }
__device__ inline double matern32_d1(double sf2, double e, double d, double c) { return (sf2 * e) * (d * c); }
__device__ inline double matern32_d2(double sf2, double e, double Q, double dk, double dl, double ck, double cl,
                                     bool same) {
  const double r = Q > 0.0 ? (dk * dl) / Q : 0.0;
  return ((sf2 * e) * (ck * cl)) * ((same ? 1.0 : 0.0) - r);
}
// Entry (k, l), k, l = 0..3, of the 4 x 4 joint covariance of u = (f, df/dx,
// df/dy, df/dt) at a with u at b: d[q] = scaled a - scaled b, nd[q] = scaled b
// - scaled a (its exact negative), c[q] = c_q
__device__ inline double matern32_joint(double sf2, double Q, double e, const double (&d)[3], const double (&nd)[3],
                                        const double (&c)[3], int k, int l) {
  if (k == 0 && l == 0) return matern32_qe(sf2, Q, e);
  if (l == 0) return matern32_d1(sf2, e, nd[k - 1], c[k - 1]);
  if (k == 0) return matern32_d1(sf2, e, d[l - 1], c[l - 1]);
  return matern32_d2(sf2, e, Q, d[k - 1], d[l - 1], c[k - 1], c[l - 1], k == l);
}

// scaled rows of the tile's 64 rows (si) and 64 columns (sj) into LDS, zero beyond n
__device__ inline void stage_tile(const double* __restrict__ s, int n, int it, int jt,
                                  double (*si)[64], double (*sj)[64]) {
  const int t = threadIdx.x;
  if (t < 128) {
    const int a = t < 64 ? it * 64 + t : jt * 64 + (t - 64);
    for (int d = 0; d < 3; ++d) (t < 64 ? si : sj)[d][t & 63] = a < n ? s[(size_t)a * 3 + d] : 0.0;
  }
  __syncthreads();
}
