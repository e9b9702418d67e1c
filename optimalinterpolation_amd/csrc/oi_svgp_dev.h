// Device helpers shared by the SVGP kernels: training (oi_svgp.hip) and the
// prediction / ELBO entry points on trained parameters (oi_svgp_predict.hip).
// Both files are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int MMAX = 64;      // inducing points per cell
constexpr double SQRT3 = 1.7320508075688772;
constexpr double JITTER = 1e-6;
constexpr double LIK_LOWER = 1e-6;
constexpr double LOG2PI = 1.8378770664093453;

__device__ inline double softplus(double x) {  // np.logaddexp(0, x)
  return fmax(x, 0.0) + log1p(exp(-fabs(x)));
}

// GPflow Matern32 pieces for one pair of 3-vectors (already divided by ls):
// r2 = |a|^2 + |b|^2 - 2 a.b clamped at 0 (GPflow's square_distance),
// r = sqrt(max(r2, 1e-36)); returns k/var = (1 + sqrt3 r) e, writes e
__device__ inline double m32(const double* a, const double* b, double& e) {
  const double sa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  const double sb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  double r2 = (sa + sb) - 2.0 * ab;
  r2 = r2 > 0.0 ? r2 : 0.0;
  const double r = sqrt(r2 > 1e-36 ? r2 : 1e-36);
  e = exp(-SQRT3 * r);
  return (1.0 + SQRT3 * r) * e;
}

// L = chol(W) for the symmetric M x M matrix W (row-major, LDS; its lower
// triangle is overwritten).  Right-looking, one barrier per column: in step j
// every thread reads column j of W (final for this step) and scales it on the
// fly by 1/sqrt(a_jj) (as LAPACK dpotf2 does), writing L's column j and the
// trailing lower triangle.  Returns false if a pivot is not positive.
// (A one-wave variant with lane-owned rows and no block barriers measured 3x
// slower: each of its ~M^2/2 shuffle + LDS read-modify-write steps is exposed
// latency.)
__device__ bool chol_lds(double* W, double* L, int M, int* flag) {
  const int nt = (int)blockDim.x;
  for (int e = threadIdx.x; e < M * M; e += nt) L[e] = 0.0;
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  for (int j = 0; j < M; ++j) {
    const double d = W[j * M + j];
    const double ljj = sqrt(d), rj = 1.0 / ljj;
    if (threadIdx.x == 0 && !(d > 0.0)) *flag = 1;
    const int rem = M - j - 1;
    for (int e = threadIdx.x; e < rem * rem + rem + 1; e += nt) {
      if (e < rem * rem) {  // W[i][k] -= l_ij l_kj, j < k <= i
        const int i = j + 1 + e / rem, k = j + 1 + e % rem;
        if (k <= i) W[i * M + k] -= (W[i * M + j] * rj) * (W[k * M + j] * rj);
      } else {  // column j of L
        const int i = j + (e - rem * rem);
        L[i * M + j] = i == j ? ljj : W[i * M + j] * rj;
      }
    }
    __syncthreads();
  }
  return *flag == 0;
}

// parameter vector layout (oracle Params.flat): ls_raw[3], var_raw, lik_raw, c,
// Z[M*3], q_mu[M], tril(S) row-major [M(M+1)/2]
__device__ inline int tri_index(int i, int j) { return i * (i + 1) / 2 + j; }  // i >= j

}  // namespace
