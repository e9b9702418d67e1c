// The Matern-3/2 covariance of the two plain fp64 paths (oi_nystrom.hip; the
// dense path's oi_predict.hip and oi_sample.hip, which also share stage_tile
// below) as SGPkernel writes it (GPR_CS2S3.py, GPR:83-93).  Every
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
