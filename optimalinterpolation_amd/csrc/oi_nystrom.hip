// Nystrom-approximated GP of the reference notebook (GP_example.ipynb, code
// cell 1 -- abbreviated NB1): Nystroem, SMLII(approx=True, M) and
// GPR(approx=True, M) for a ragged batch of cells.
//
// Per cell, with n observations, M inducing rows sel (NB1 Nystroem draws them
// with np.random.seed(20); the caller passes them), Matern-3/2 kernel:
//
//   Kmm = K(x_sel, x_sel)            Knm = K(x, x_sel)            (kernels below)
//   s, u = eigh(Kmm); s[s<=0] = 1e-12; st = n s / M               (oila::eigh)
//   ut = sqrt(M/n) Knm u / s;  C = Vi ut = ut / sn2                (oila::gemm + kernel)
//   B = diag(1/st) + ut' C;  L = chol(B)                           (oila::gemm + cholesky)
//
// NB1 then forms alpha = L'^-1 L^-1 C' and Ki = Vi - C alpha (n x n).  Here
// the same quantities come from W' = C L^-T (n x M: a right-looking block
// triangular solve with the Cholesky's diagonal-block inverses):
//   C alpha = W'W,  A = Ki r = r/sn2 - W'(W r),  k*'Ki k* = |k*|^2/sn2 - |W k*|^2
// and, because D B D = H / sn2 for D = diag(sqrt(st)) and NB1's
// H = sn2 I + (sqrt(st) ut)'(sqrt(st) ut),
//   slogdet(H) = M log sn2 + sum log st + 2 sum log diag(L)
// -- no second Cholesky.  Only the objective needs the n x n Ki = Vi - W'W
// (one n x n x M GEMM), its lower triangle swept once by the fused kernel k_nys_grad, which
// regenerates K and dK_d from the 3-D inputs in registers and reduces
// (Ki - A A') against them, so the n x n x 3 dK array the notebook
// materialises never exists:
//   nlZ = r.A/2 + slogdet(H)/2 + n log(2 pi)/2
//   dnlZ_d = sum((Ki - A A') * dK_d)/2, dnlZ_3 = sum(Q * 2K)/2, dnlZ_4 = sn2 tr(Q)
//   (exact K, dK: NB1 SMLII quirks kept)
//   predict: fs = mean + k*.A;  sd = sqrt(sf2 - k*'Ki k*);  prior sd = sqrt(sf2)
//   predict at nt targets (oi_nystrom_predict_multi): after the same set-up,
//   cov = Kxs - (Kxsx'Kxsx/sn2 - V'V), V = W Kxsx, by one fused MFMA kernel per
//   cell (k_nys_cov_mfma); the nt x nt err is never formed
//
// Every dense step -- the eigendecomposition, the Cholesky, the products --
// is a hand-written gfx950 kernel of oi_linalg.hip (no LAPACK / rocSOLVER /
// rocBLAS): the eigensolver is one workgroup per matrix for the Householder
// tridiagonalisation and the tridiagonal eigenpairs, batched MFMA products for
// the orthogonalisation and the back-transform.  A Runner evaluates a chunk
// of cells phase by phase on one stream; independent Runners (the groups of a
// fit, oi_nystrom_fit.hip) overlap on streams of their own.  Per-cell status
// comes back in one copy at the end.  The host declarations are in
// oi_nystrom.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "oi_gemm.h"
#include "oi_host.h"
#include "oi_linalg.h"
#include "oi_matern.h"
#include "oi_nystrom.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------- kernels --

// scaled coordinates as SGPkernel forms them (GPR:83, :93):
//   sc = np.sqrt(3.) * x / ell      (the 3-D distance Q)
//   sq = np.sqrt(3.) * (x / ell)    (the per-dimension q_d of dK)
__global__ void k_nys_scale(const double* __restrict__ x, int64_t n, double l0, double l1,
                            double l2, double* __restrict__ sc, double* __restrict__ sq) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double ell[3] = {l0, l1, l2};
  for (int d = 0; d < 3; ++d) {
    const double v = x[i * 3 + d];
    sc[i * 3 + d] = matern_scale(v, ell[d]);
    if (sq) sq[i * 3 + d] = matern_scale_q(v, ell[d]);
  }
}

__device__ inline double dist3(const double* a, const double* b) {
  return matern_dist(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
}

// out[i + ld j] = sf2 (1 + Q) exp(-Q), Q = |sa[ia[i]] - sb[ib[j]]| (column-major)
__global__ void k_nys_cross(const double* __restrict__ sa, const int64_t* __restrict__ ia,
                            int64_t na, const double* __restrict__ sb,
                            const int64_t* __restrict__ ib, double sf2, double* __restrict__ out,
                            int64_t ld) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.y;
  if (i >= na) return;
  const int64_t ra = ia ? ia[i] : i, rb = ib ? ib[j] : j;
  const double* a = sa + ra * 3;
  const double* b = sb + rb * 3;
  out[i + ld * j] = matern32(sf2, a[0] - b[0], a[1] - b[1], a[2] - b[2]);
}

// s[s <= 0] = 1e-12; st = n * s / M  for the M real eigenvalues; st = 1 on a
// padded tail (so the pad contributes log 1 = 0 to the batched log-determinant)
__global__ void k_nys_eigpost(double* __restrict__ s, int64_t M, int64_t Mp, int64_t n,
                              double* __restrict__ st) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Mp) return;
  if (k >= M) {
    st[k] = 1.0;
    return;
  }
  double v = s[k];
  if (v <= 0.0) v = 1e-12;
  s[k] = v;
  st[k] = ((double)n * v) / (double)M;
}

// ut = sqrt(M/n) * U1 / s  (column k divided by s[k]);  C = ut / sn2 (= Vi ut)
// (ut may alias U1: each element is read before it is written, by one thread)
__global__ void k_nys_ut(const double* U1, int64_t n, int64_t M,
                         const double* __restrict__ s, double c, double isn2,
                         double* ut, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * M) return;
  const int64_t k = e / n;
  const double u = (c * U1[e]) / s[k];
  ut[e] = u;
  C[e] = isn2 * u;
}

// A = r / sn2 (Vi r; the W'(W r) part is subtracted by a gemv)
__global__ void k_nys_vi(const double* __restrict__ r, int64_t n, double isn2,
                         double* __restrict__ A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[i] = isn2 * r[i];
}

// A[i + ld i] = d + A[i + ld i]  (d = dv[i] if dv, else 1/dv-free scalar; inv => 1/dv[i])
__global__ void k_nys_diag(double* __restrict__ A, int64_t m, int64_t ld,
                           const double* __restrict__ dv, int inv, double d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double a = dv ? (inv ? 1.0 / dv[i] : dv[i]) : d;
  A[i + ld * i] = a + A[i + ld * i];
}

template <int NV>
__device__ inline void block_sum(double (&v)[NV], double* red) {
  // 256 threads: wave reduction then the 4 wave partials in fixed order
  for (int q = 0; q < NV; ++q)
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
    for (int q = 0; q < NV; ++q) red[w * NV + q] = v[q];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < NV; ++q) v[q] = ((red[q] + red[NV + q]) + red[2 * NV + q]) + red[3 * NV + q];
}

// out[0] = a . b   (one 256-thread block, fixed order)
__global__ void __launch_bounds__(256) k_nys_dot(const double* __restrict__ a,
                                                 const double* __restrict__ b, int64_t n,
                                                 double* __restrict__ out) {
  __shared__ double red[4];
  double v[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n; i += 256) v[0] += a[i] * b[i];
  block_sum<1>(v, red);
  if (threadIdx.x == 0) out[0] = v[0];
}

// per matrix b of a strided batch of Cholesky factors:
//   res[b * NRES_ + 1] = sum_k log L_b[k + M k] + (sum_k log st_b[k]) / 2
// (slogdet(H)/2 minus M log(sn2)/2; one block per matrix)
__global__ void __launch_bounds__(256) k_nys_logdet(const double* __restrict__ L, int64_t M,
                                                    int64_t ld, int64_t strideL,
                                                    const double* __restrict__ st,
                                                    int64_t strideS, double* __restrict__ res,
                                                    int64_t strideR) {
  __shared__ double red[8];
  const int64_t b = blockIdx.x;
  L += b * strideL;
  st += b * strideS;
  double v[2] = {0.0, 0.0};
  for (int64_t i = threadIdx.x; i < M; i += 256) {
    v[0] += log(L[i + ld * i]);
    v[1] += log(st[i]);
  }
  block_sum<2>(v, red);
  if (threadIdx.x == 0) res[b * strideR + 1] = v[0] + v[1] / 2.0;
}

// pad the M x M matrix in the top-left of an Mp x Mp column-major buffer to a
// block-diagonal diag(A, d I): rows / columns M..Mp-1 zero except d on the
// diagonal.  Householder tridiagonalisation and Cholesky never mix the two
// blocks (the reflectors' entries in the pad rows are exactly 0), so the
// leading block's factors and eigenpairs are those of A itself.
__global__ void k_nys_pad(double* __restrict__ A, int64_t M, int64_t Mp, double d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i >= Mp || (i < M && j < M)) return;
  A[i + Mp * j] = i == j ? d : 0.0;
}

// The objective's n x n pass (NB1 SMLII, approx branch): the five sums
// sum Q dK_0, sum Q dK_1, sum Q dK_2, sum Q (2 K), tr Q over Q = Ki - A A',
// K = sf2 (1+D) e^-D, dK_d = sf2 q_d^2 e^-D regenerated from the scaled
// inputs (no n x n x 3 array).  Q and dK are symmetric and Ki is stored as its
// lower triangle only (syrk), so the sweep covers 64 x 64 tiles on or below
// the diagonal, weighting i > j by 2; one partial row of 5 per tile (zeros
// above the diagonal), Ki read once, coalesced along its columns.
__global__ void __launch_bounds__(256) k_nys_grad(const double* __restrict__ Ki,
                                                  const double* __restrict__ A,
                                                  const double* __restrict__ sc,
                                                  const double* __restrict__ sq, int64_t n,
                                                  double sf2, double* __restrict__ part) {
  __shared__ double red[4 * 5];
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (blockIdx.x >= blockIdx.y) {
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const int64_t j0 = (int64_t)blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i < n) {
      const double ci[3] = {sc[i * 3], sc[i * 3 + 1], sc[i * 3 + 2]};
      const double qi[3] = {sq[i * 3], sq[i * 3 + 1], sq[i * 3 + 2]};
      const double Ai = A[i];
      int64_t jend = j0 + 16 < n ? j0 + 16 : n;
      jend = jend < i + 1 ? jend : i + 1;  // j <= i
      for (int64_t j = j0; j < jend; ++j) {
        const double Q = Ki[i + n * j] - Ai * A[j];
        const double D = dist3(ci, sc + j * 3);
        const double e = exp(-D);
        const double K = sf2 * ((1.0 + D) * e);
        const double w = j == i ? 1.0 : 2.0;
        for (int d = 0; d < 3; ++d) {
          // SGPkernel's q_d = pdist of one coordinate = sqrt(t*t) = |t| exactly
          // (binary64, round-to-nearest), so q_d^2 = fl(t*t): no sqrt needed
          const double t = qi[d] - sq[j * 3 + d];
          v[d] += w * (Q * (sf2 * ((t * t) * e)));
        }
        v[3] += w * (Q * (2.0 * K));
        if (j == i) v[4] += Q;
      }
    }
  }
  block_sum<5>(v, red);
  if (threadIdx.x == 0) {
    const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int q = 0; q < 5; ++q) part[b * 5 + q] = v[q];
  }
}

// out[q] = sum_b part[b*5 + q]  (fixed order)
__global__ void __launch_bounds__(256) k_nys_partsum(const double* __restrict__ part,
                                                     int64_t nb, double* __restrict__ out) {
  __shared__ double red[4 * 5];
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < nb; b += 256)
    for (int q = 0; q < 5; ++q) v[q] += part[b * 5 + q];
  block_sum<5>(v, red);
  if (threadIdx.x == 0)
    for (int q = 0; q < 5; ++q) out[q] = v[q];
}

// W' (n x M, column-major) -> 64 x 64 k-major tiles Wp[kt][it] (element
// kk*64 + mm = W'[64 it + mm][64 kt + kk], zero beyond n / M): the operand
// layout of the MFMA tile GEMM core (oi_gemm.h)
__global__ void __launch_bounds__(256) k_nys_pack(const double* __restrict__ Wt, int64_t n,
                                                  int64_t M, int Tn, double* __restrict__ Wp) {
  const int it = blockIdx.x % Tn, kt = blockIdx.x / Tn;
  double* dst = Wp + (size_t)blockIdx.x * 4096;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int64_t a = (int64_t)it * 64 + (e & 63), k = (int64_t)kt * 64 + (e >> 6);
    dst[e] = (a < n && k < M) ? Wt[a + n * k] : 0.0;
  }
}

// The objective's n x n pass without materialising Ki: per lower 64 x 64 tile
// (i >= j) the MFMA core forms (W'W)_ij = sum_k Wp[k][i]^T Wp[k][j] in
// registers, then Ki = [a == b]/sn2 - (W'W)_ab, Q = Ki - A_a A_b and the five
// sums against K, dK regenerated from the scaled inputs (as k_nys_grad),
// off-diagonal entries weighted 2.  One partial row of 5 per tile.
__global__ void __launch_bounds__(256) k_nys_grad_mfma(const double* __restrict__ Wp, int Tn,
                                                       int Tk, const double* __restrict__ A,
                                                       const double* __restrict__ sc,
                                                       const double* __restrict__ sq, int64_t n,
                                                       double sf2, double isn2,
                                                       double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[GEMM1_LDS];
  const int tile = blockIdx.x;
  int i = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= tile) ++i;
  while (i * (i + 1) / 2 > tile) --i;
  const int j = tile - i * (i + 1) / 2;
  Quad acc;
  quad_zero(acc);
  gemm1_kmajor<false>(acc, lds, 4 * Tk, 0u, [=](int p, const double*& a, const double*& b) {
    a = Wp + ((size_t)p * Tn + i) * 4096;
    b = Wp + ((size_t)p * Tn + j) * 4096;
  });
  double* cQ = lds;            // [3][128] scaled inputs (distance), rows i | columns j
  double* cq = lds + 3 * 128;  // [3][128] per-dimension scaled inputs
  double* al = lds + 6 * 128;  // [128] A
  double* red = lds + 7 * 128;
  const int t = threadIdx.x;
  if (t < 128) {
    const int64_t a = t < 64 ? (int64_t)i * 64 + t : (int64_t)j * 64 + (t - 64);
    for (int d = 0; d < 3; ++d) {
      cQ[d * 128 + t] = a < n ? sc[3 * a + d] : 0.0;
      cq[d * 128 + t] = a < n ? sq[3 * a + d] : 0.0;
    }
    al[t] = a < n ? A[a] : 0.0;
  }
  __syncthreads();
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int mb = 0; mb < 2; ++mb)
    for (int nb = 0; nb < 2; ++nb)
      for (int r = 0; r < 4; ++r) {
        const int m = acc1_row(mb, r), nn = acc1_col(nb);
        const int64_t a = (int64_t)i * 64 + m, b = (int64_t)j * 64 + nn;
        if (a >= n || b >= n || (i == j && m < nn)) continue;
        const double x = acc.c[mb][nb][r];
        const double Ki = a == b ? isn2 - x : -x;
        const double Q = Ki - al[m] * al[64 + nn];
        const double d0 = cQ[m] - cQ[64 + nn], d1 = cQ[128 + m] - cQ[128 + 64 + nn],
                     d2 = cQ[256 + m] - cQ[256 + 64 + nn];
        const double D = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double e = exp(-D);
        const double K = sf2 * ((1.0 + D) * e);
        const double w = a == b ? 1.0 : 2.0;
        for (int d = 0; d < 3; ++d) {
          const double tt = cq[d * 128 + m] - cq[d * 128 + 64 + nn];
          v[d] += w * (Q * (sf2 * ((tt * tt) * e)));
        }
        v[3] += w * (Q * (2.0 * K));
        if (a == b) v[4] += Q;
      }
  block_sum<5>(v, red);
  if (t == 0)
    for (int q = 0; q < 5; ++q) part[(size_t)tile * 5 + q] = v[q];
}

// ---- prediction at many targets per cell (oi_nystrom_predict_multi) ----
// NB1 GPR(approx=True) with xs of size nt x 3:
//   Kxsx = SGPkernel(x, xs=xs) (n x nt), Kxs = SGPkernel(xs) (nt x nt)
//   err = Kxsx' Ki Kxsx = Kxsx'Kxsx / sn2 - V'V,  V = W Kxsx (M x nt)
//   fs = mean + Kxsx' A,  cov = Kxs - err,  sd = sqrt(diag(cov))

// out[a + nt k] = sf2 (1 + Q) exp(-Q), Q = |sc[k] - ts[a]|: Kxsx' (nt x n,
// column-major), from the scaled observations sc and scaled targets ts
__global__ void k_nys_cross_t(const double* __restrict__ ts, int64_t nt,
                              const double* __restrict__ sc, int64_t n, double sf2,
                              double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nt * n) return;
  const int64_t a = e % nt, k = e / nt;
  const double* o = sc + k * 3;
  const double* b = ts + a * 3;
  out[e] = matern32(sf2, o[0] - b[0], o[1] - b[1], o[2] - b[2]);
}

// fs[a] = mean + sum_k KxT[a + nt k] A[k]  (one 256-thread block per target:
// the order of k_nys_dot, the same for every target of every call)
__global__ void __launch_bounds__(256) k_nys_fs(const double* __restrict__ KxT, int64_t nt,
                                                int64_t n, const double* __restrict__ A,
                                                double mean, double* __restrict__ fs) {
  __shared__ double red[4];
  const int64_t a = blockIdx.x;
  double v[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n; i += 256) v[0] += KxT[a + nt * i] * A[i];
  block_sum<1>(v, red);
  if (threadIdx.x == 0) fs[a] = mean + v[0];
}

// The posterior covariance without err as a matrix: per lower 64 x 64 tile
// (i >= j) of the nt x nt output the MFMA core accumulates
//   acc1 = (Kxsx'Kxsx)_ij over the n rows   (Kp: k_nys_pack of Kxsx', nch1 chunks of 16)
//   acc2 = (V'V)_ij       over the M rows   (Vp: k_nys_pack of V',    nch2 chunks of 16)
// and the epilogue forms cov(a, b) = Kxs(a, b) - (acc1 / sn2 - acc2), Kxs
// regenerated from the scaled targets (diagonal sf2 exactly), stores it at
// (a, b) and (b, a) of the row-major nt x nt output -- in a diagonal tile from
// the entries with a >= b -- and the diagonal into var.  cov may be null: the
// grid is then the Tt diagonal tiles (blockIdx.x = i = j) and only var is
// written, by the same arithmetic.
__global__ void __launch_bounds__(256) k_nys_cov_mfma(const double* __restrict__ Kp, int nch1,
                                                      const double* __restrict__ Vp, int nch2,
                                                      int Tt, const double* __restrict__ ts,
                                                      int64_t nt, double sf2, double sn2,
                                                      double* __restrict__ cov,
                                                      double* __restrict__ var) {
  __shared__ __attribute__((aligned(16))) double lds[GEMM1_LDS];
  int i = blockIdx.x, j = blockIdx.x;
  if (cov) {
    const int tile = blockIdx.x;
    i = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= tile) ++i;
    while (i * (i + 1) / 2 > tile) --i;
    j = tile - i * (i + 1) / 2;
  }
  Quad acc1, acc2;
  quad_zero(acc1);
  quad_zero(acc2);
  gemm1_kmajor<false>(acc1, lds, nch1, 0u, [=](int p, const double*& a, const double*& b) {
    a = Kp + ((size_t)p * Tt + i) * 4096;
    b = Kp + ((size_t)p * Tt + j) * 4096;
  });
  gemm1_kmajor<false>(acc2, lds, nch2, 0u, [=](int p, const double*& a, const double*& b) {
    a = Vp + ((size_t)p * Tt + i) * 4096;
    b = Vp + ((size_t)p * Tt + j) * 4096;
  });
  double* cs = lds;  // [3][128] scaled targets, rows i | columns j
  const int t = threadIdx.x;
  if (t < 128) {
    const int64_t a = t < 64 ? (int64_t)i * 64 + t : (int64_t)j * 64 + (t - 64);
    for (int d = 0; d < 3; ++d) cs[d * 128 + t] = a < nt ? ts[3 * a + d] : 0.0;
  }
  __syncthreads();
  for (int mb = 0; mb < 2; ++mb)
    for (int nb = 0; nb < 2; ++nb)
      for (int r = 0; r < 4; ++r) {
        const int m = acc1_row(mb, r), nn = acc1_col(nb);
        const int64_t a = (int64_t)i * 64 + m, b = (int64_t)j * 64 + nn;
        if (a >= nt || b >= nt || (i == j && m < nn)) continue;
        const double err = acc1.c[mb][nb][r] / sn2 - acc2.c[mb][nb][r];
        const double kxs = a == b ? sf2
                                  : matern32(sf2, cs[m] - cs[64 + nn], cs[128 + m] - cs[128 + 64 + nn],
                                             cs[256 + m] - cs[256 + 64 + nn]);
        const double c = kxs - err;
        if (cov) {
          cov[(size_t)a * nt + b] = c;
          if (a != b) cov[(size_t)b * nt + a] = c;
        }
        if (a == b) var[a] = c;
      }
}

}  // namespace

// ------------------------------------------------------------------- host --

namespace oi_nys {

// nys_eigh = the Householder tridiagonalisation; the eigensolver's other phases
// are timed as their own stages
const char* const kStage[S_COUNT] = {"nys_build",  "nys_eigh",   "nys_eigh_vectors", "nys_eigh_orth",
                                     "nys_eigh_back", "nys_panels", "nys_ki_gemm", "nys_apply",
                                     "nys_logdet", "nys_grad",   "nys_predict", "nys_predict_multi"};

int check_batch(Batch& b) {
  if (b.ncell < 0) return oi_set_last_error(OI_E_ARG, "negative ncell");
  if (b.ncell == 0) return 0;
  if (!b.sel || !b.xyt || !b.y) return oi_set_last_error(OI_E_ARG, "null pointer");
  if (int rc = oi_check_offs(b.offs, b.ncell, 1, "offs")) return rc;
  if (int rc = oi_check_offs(b.soffs, b.ncell, 0, "soffs")) return rc;
  for (int64_t c = 0; c < b.ncell; ++c) {
    const int64_t n = b.offs[c + 1] - b.offs[c], M = b.soffs[c + 1] - b.soffs[c];
    if (M < 1 || M > n) return oi_set_last_error(OI_E_ARG, "each cell needs 1 <= M <= n");
    for (int64_t k = b.soffs[c]; k < b.soffs[c + 1]; ++k)
      if (b.sel[k] < 0 || b.sel[k] >= n)
        return oi_set_last_error(OI_E_ARG, "inducing index out of range");
    b.nmax = n > b.nmax ? n : b.nmax;
    b.mmax = M > b.mmax ? M : b.mmax;
  }
  if (b.nmax > INT32_MAX / 2) return oi_set_last_error(OI_E_ARG, "cell too large");
  return 0;
}

// the LINEAR hypers of ncell cells (5 each)
int check_hypers(const double* hyp, int64_t ncell) {
  for (int64_t q = 0; q < ncell * 5; ++q)
    if (!(hyp[q] > 0.0)) return oi_set_last_error(OI_E_ARG, "hypers must be > 0");
  return 0;
}

BatchDev::BatchDev(const Batch& b, const double* xs, bool device_inputs, hipStream_t st) {
  const int64_t N = b.offs[b.ncell], S = b.soffs[b.ncell];
  const double* dx = b.xyt;
  const double* dy = b.y;
  if (!device_inputs) {
    hx.alloc_async(N * 3 * 8, st);
    hy.alloc_async(N * 8, st);
    HC(hipMemcpyAsync(hx.p, b.xyt, N * 3 * 8, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(hy.p, b.y, N * 8, hipMemcpyHostToDevice, st));
    dx = hx.as<double>();
    dy = hy.as<double>();
  }
  dsel.alloc_async(S * 8, st);
  HC(hipMemcpyAsync(dsel.p, b.sel, S * 8, hipMemcpyHostToDevice, st));
  if (xs) {
    dxs.alloc_async(b.ncell * 3 * 8, st);
    HC(hipMemcpyAsync(dxs.p, xs, b.ncell * 3 * 8, hipMemcpyHostToDevice, st));
  }
  HC(hipStreamSynchronize(st));  // host arrays may go away once submit returns
  rows.resize(b.ncell);
  for (int64_t c = 0; c < b.ncell; ++c)
    rows[c] = CellSrc{dx + b.offs[c] * 3, dy + b.offs[c], dsel.as<int64_t>() + b.soffs[c],
                      xs ? dxs.as<double>() + c * 3 : nullptr, b.offs[c + 1] - b.offs[c],
                      b.soffs[c + 1] - b.soffs[c]};
}

Runner::Runner(const std::vector<CellSrc>* tab, int64_t nmax, int64_t mmax, int64_t cap, const oi_options& o, bool obj,
               bool pred, bool own_stream)
    : tab_(tab), cap_(cap), st_((hipStream_t)o.stream), obj_(obj), pred_(pred) {
  if (own_stream) {
    own_.create();
    st_ = own_.s;
  }
  hres_.reserve(cap * NRES * 8);
  hinfo_.reserve(cap * NINFO * sizeof(int32_t));
  hr_ = hres_.as<double>();
  hi_ = hinfo_.as<int32_t>();
  la_.bind(st_);
  sg_.on = o.profile != 0;
  sg_.st = st_;
  const int64_t fd = Fixed::doubles(nmax, mmax, cap, obj, pred, kn_.fused);
  fixed_.alloc((size_t)fd * 8);
  Carver cf{fixed_.as<double>()};
  fx_.layout(cf, nmax, mmax, cap, obj, pred, kn_.fused);
  if (cf.off > fd) throw HipErr{"Runner: fixed workspace layout exceeds its estimate"};
  // the slot arrays: chunk <= 64 cells and <= 1/4 of the HBM that is free now
  // that the fixed part exists
  const int64_t Mpmax = Mp(mmax);
  const size_t per = (size_t)Slots::doubles(1, nmax, Mpmax, 1) * 8;
  size_t fr = 0, tot = 0;
  HC(hipMemGetInfo(&fr, &tot));
  chunk_ = std::min<int64_t>(std::min<int64_t>(64, cap), std::max<int64_t>(1, (int64_t)(fr / 4 / per)));
  const int64_t sd = Slots::doubles(chunk_, nmax, Mpmax);
  slots_.alloc((size_t)sd * 8);
  Carver cs{slots_.as<double>()};
  sl_.layout(cs, chunk_, nmax, Mpmax);
  if (cs.off > sd) throw HipErr{"Runner: slot workspace layout exceeds its estimate"};
}
Runner::~Runner() {  // the members (buffers first, the stream last) go after the stream's work
  if (own_.s) (void)hipStreamSynchronize(own_.s);
}

void Runner::run(const std::vector<int64_t>& cells, const double* hyp, double mean, CellOut* out) {
  mean_ = mean;
  enqueue(cells, hyp);
  collect(out);
}
void Runner::run_all(int64_t ncell, const double* hyp, double mean, CellOut* out) {
  std::vector<int64_t> cells(ncell);
  for (int64_t c = 0; c < ncell; ++c) cells[c] = c;
  run(cells, hyp, mean, out);
}

void Runner::enqueue(const std::vector<int64_t>& cells, const double* hyp) {
  const int64_t nc = (int64_t)cells.size();
  ncq_ = nc;
  if (!nc) return;
  if (nc > cap_) throw HipErr{"Runner: more cells than its capacity"};
  cellv_ = cells;
  hypv_.assign(hyp, hyp + nc * 5);
  // positions sorted by M (equal-M cells adjacent for the batched factorisations)
  order_.resize(nc);
  for (int64_t k = 0; k < nc; ++k) order_[k] = k;
  std::stable_sort(order_.begin(), order_.end(), [&](int64_t a, int64_t c) {
    return Mof(cells[a]) < Mof(cells[c]);
  });
  HC(hipMemsetAsync(fx_.res, 0, nc * NRES * 8, st_));
  HC(hipMemsetAsync(fx_.info, 0, nc * NINFO * sizeof(int32_t), st_));
  for (int64_t p0 = 0; p0 < nc; p0 += chunk_) {
    const int64_t p1 = std::min(nc, p0 + chunk_);
    for (int64_t p = p0; p < p1; ++p) phase1(p, p - p0);
    batched(p0, p1, 0);
    batched3(p0, p1);
    batched(p0, p1, 1);
    for (int64_t p = p0; p < p1; ++p) phase5(p, p - p0);
  }
  HC(hipMemcpyAsync(hr_, fx_.res, nc * NRES * 8, hipMemcpyDeviceToHost, st_));
  HC(hipMemcpyAsync(hi_, fx_.info, nc * NINFO * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
}

void Runner::collect(CellOut* out) {
  const int64_t nc = ncq_;
  if (!nc) return;
  HC(hipStreamSynchronize(st_));
  sg_.flush();
  la_.reset();  // every launch that read the staged descriptors has completed
  const double inf = INFINITY, nan = NAN;
  for (int64_t p = 0; p < nc; ++p) {
    const int64_t k = order_[p], c = cellv_[k];
    const int64_t n = (*tab_)[c].n, M = Mof(c);
    const double sf2 = hypv_[k * 5 + 3], sn2 = hypv_[k * 5 + 4];
    const double* rr = hr_ + p * NRES;
    const int32_t* ii = hi_ + p * NINFO;
    const bool bad = ii[0] != 0 || ii[1] != 0;  // NB1's LinAlgError (eigh / cholesky)
    CellOut& r = out[k];
    r.status = bad ? 1 : 0;
    if (obj_) {
      if (bad) {
        r.nlz = inf;
        for (int q = 0; q < 5; ++q) r.grad[q] = inf;
      } else {
        // det = slogdet(H)/2 = (M log sn2 + sum log st + 2 sum log diag L) / 2
        const double det = (double)M * std::log(sn2) / 2.0 + rr[1];
        r.nlz = (rr[0] / 2.0 + det) + (double)n * std::log(2.0 * M_PI) / 2.0;
        r.grad[0] = rr[2] / 2.0;
        r.grad[1] = rr[3] / 2.0;
        r.grad[2] = rr[4] / 2.0;
        r.grad[3] = rr[5] / 2.0;
        r.grad[4] = sn2 * rr[6];
      }
    }
    if (pred_) {
      const double err = rr[8] / sn2 - rr[9];  // k*'Ki k* = |k*|^2/sn2 - |W k*|^2
      r.fs = bad ? nan : mean_ + rr[7];
      r.sd = bad ? nan : std::sqrt(sf2 - err);
      r.sprior = std::sqrt(sf2);
    }
  }
}

// which = 0: s, u = eigh(Kmm) (oila::eigh; u overwrites Kmm); 1: L = chol(B)
// (oila::cholesky, in place, with the diagonal-block inverses kept for the
// triangular solve) -- one batched call per run of slots with equal padded
// size, on the main stream
void Runner::batched(int64_t p0, int64_t p1, int which) {
  for (int64_t g0 = p0; g0 < p1;) {
    const int64_t M = Mp(Mof(cellv_[order_[g0]]));  // padded size of the group
    int64_t g1 = g0 + 1;
    while (g1 < p1 && Mp(Mof(cellv_[order_[g1]])) == M) ++g1;
    const int iM = (int)M, cnt = (int)(g1 - g0);
    const int64_t s0 = g0 - p0;
    const double dM = (double)M;
    if (which == 0) {
      std::vector<oila::Eigh> es;
      for (int q = 0; q < cnt; ++q)
        es.push_back(oila::Eigh{sl_.Kmm.slot(s0 + q), sl_.eval.slot(s0 + q), sl_.EW.slot(s0 + q), iM, iM,
                                fx_.info + (g0 + q) * NINFO + 0});
      // algorithmic flops per phase: tridiagonalisation 4/3 M^3, tridiagonal
      // eigenpairs O(M^2), BCGS2 2 M^3, back-transform 2 M^3
      const double m3 = dM * dM * dM * cnt;
      const int kind[4] = {S_EIGH, S_EIGH_VEC, S_EIGH_ORTH, S_EIGH_BACK};
      const double fl[4] = {4.0 / 3.0 * m3, 0.0, 2.0 * m3, 2.0 * m3};
      oila::eigh(la_, st_, es, [&](int k) {
        if (k > 0) sg_.end();
        if (k < 4) sg_.begin(kind[k], fl[k], 0.0);
      });
    } else {
      // L = chol(B); half log-determinants; then W' = C L^-T by a block
      // triangular solve with the kept diagonal-block inverses
      sg_.begin(S_PANEL, dM * dM * dM / 3 * cnt, 0.0);
      std::vector<oila::Chol> cs;
      for (int q = 0; q < cnt; ++q)
        cs.push_back(oila::Chol{sl_.B.slot(s0 + q), sl_.Dinv.slot(s0 + q), fx_.info + (g0 + q) * NINFO + 1, iM, iM});
      oila::cholesky(la_, st_, cs);
      // the pad block is the identity: log 1 = 0 and st is 1 there (see batched3)
      hipLaunchKernelGGL(k_nys_logdet, dim3(cnt), dim3(256), 0, st_, sl_.B.slot(s0), M, M, sl_.B.stride,
                         sl_.stl.slot(s0), sl_.stl.stride, fx_.res + g0 * NRES, (int64_t)NRES);
      KCHK();
      // W' = C L^-T in place on each slot's C (n x M, leading dimension n): one
      // batched right-looking block solve for the whole group
      std::vector<oila::TrsmRLT> ts;
      for (int q = 0; q < cnt; ++q) {
        const CellRefs R = refs(g0 + q, s0 + q);
        ts.push_back(oila::TrsmRLT{R.C, R.B, R.dinv, R.in, R.iM, R.in, R.iMp});
      }
      oila::trsm_right_lt(la_, st_, ts);
      sg_.end();
    }
    g0 = g1;
  }
}

Runner::CellRefs Runner::refs(int64_t p, int64_t slot) {
  CellRefs R;
  R.k = order_[p];
  R.c = cellv_[R.k];
  R.n = (*tab_)[R.c].n;
  R.M = Mof(R.c);
  R.Mp = Mp(R.M);
  R.in = (int)R.n;
  R.iM = (int)R.M;
  R.iMp = (int)R.Mp;
  R.dn = (double)R.n;
  R.dM = (double)R.M;
  R.x = (*tab_)[R.c].x;
  R.r = (*tab_)[R.c].y;
  R.sl = (*tab_)[R.c].sel;
  R.hp = hypv_.data() + R.k * 5;
  R.sc = sl_.sc.slot(slot);
  R.sq = sl_.sq.slot(slot);
  R.Kmm = sl_.Kmm.slot(slot);
  R.s = sl_.eval.slot(slot);
  R.stl = sl_.stl.slot(slot);
  R.C = sl_.C.slot(slot);
  R.B = sl_.B.slot(slot);
  R.rs = fx_.res + p * NRES;
  R.dinv = sl_.Dinv.slot(slot);
  return R;
}

// phase 3 for a whole chunk: s clamp, st; Knm = SGPkernel(x, xs=x[sel]);
// U1 = Knm u; ut, C = Vi ut; B = diag(1/st) + ut' C -- the per-cell elementwise
// kernels, and each of the two n x M products as ONE batched oila::gemm over
// the chunk's cells (per-cell launches of ~1 000 64 x 64 tiles left the
// chip under-filled in the last wave of tiles)
void Runner::batched3(int64_t p0, int64_t p1) {
  hipStream_t st = st_;
  double fl = 0.0, by = 0.0;
  for (int64_t p = p0; p < p1; ++p) {
    const CellRefs R = refs(p, p - p0);
    fl += 4 * R.dn * R.dM * R.dM;
    by += 8.0 * R.dn * R.dM;
  }
  sg_.begin(S_PANEL, fl, by);
  std::vector<oila::Gemm> g1, g2;
  for (int64_t p = p0; p < p1; ++p) {
    const CellRefs R = refs(p, p - p0);
    double* Knm = sl_.Knm.slot(p - p0);
    double* U1 = sl_.U1.slot(p - p0);
    hipLaunchKernelGGL(k_nys_eigpost, dim3(blocks(R.Mp, 256)), dim3(256), 0, st, R.s, R.M, R.Mp,
                       R.n, R.stl);
    KCHK();
    hipLaunchKernelGGL(k_nys_cross, dim3(blocks(R.n, 256), (unsigned)R.M), dim3(256), 0, st, R.sc,
                       nullptr, R.n, R.sc, R.sl, R.hp[3], Knm, R.n);
    KCHK();
    g1.push_back(oila::Gemm{Knm, R.Kmm, U1, R.in, R.iM, R.iM, R.in, R.iMp, R.in, 1.0, 0.0, 0});  // U1 = Knm u
    g2.push_back(oila::Gemm{U1, R.C, R.B, R.iM, R.iM, R.in, R.in, R.in, R.iMp, 1.0, 0.0, 0});    // B = ut' C
  }
  oila::gemm(la_, st, false, false, g1);
  for (int64_t p = p0; p < p1; ++p) {  // ut (in place of U1) and C
    const CellRefs R = refs(p, p - p0);
    double* U1 = sl_.U1.slot(p - p0);
    hipLaunchKernelGGL(k_nys_ut, dim3(blocks(R.n * R.M, 256)), dim3(256), 0, st, U1, R.n, R.M, R.s,
                       std::sqrt(R.dM / R.dn), 1.0 / R.hp[4], U1, R.C);
    KCHK();
  }
  oila::gemm(la_, st, true, false, g2);
  for (int64_t p = p0; p < p1; ++p) {  // B += diag(1/st), pad block
    const CellRefs R = refs(p, p - p0);
    hipLaunchKernelGGL(k_nys_diag, dim3(blocks(R.M, 256)), dim3(256), 0, st, R.B, R.M, R.Mp, R.stl, 1,
                       0.0);
    KCHK();
    if (R.Mp > R.M) {
      hipLaunchKernelGGL(k_nys_pad, dim3(blocks(R.Mp, 256), (unsigned)R.Mp), dim3(256), 0, st, R.B,
                         R.M, R.Mp, 1.0);
      KCHK();
    }
  }
  sg_.end();
}

// scaled inputs, Kmm (NB1 Nystroem: SGPkernel(x[sel]))
void Runner::phase1(int64_t p, int64_t slot) {
  const CellRefs R = refs(p, slot);
  hipStream_t st = st_;
  sg_.begin(S_BUILD, 0.0, 8.0 * R.dM * R.dM);
  hipLaunchKernelGGL(k_nys_scale, dim3(blocks(R.n, 256)), dim3(256), 0, st, R.x, R.n, R.hp[0],
                     R.hp[1], R.hp[2], R.sc, obj_ ? R.sq : nullptr);
  KCHK();
  hipLaunchKernelGGL(k_nys_cross, dim3(blocks(R.M, 256), (unsigned)R.M), dim3(256), 0, st, R.sc,
                     R.sl, R.M, R.sc, R.sl, R.hp[3], R.Kmm, R.Mp);
  KCHK();
  if (R.Mp > R.M) {
    // pad eigenvalue above every eigenvalue of K_mm (<= trace = M sf2), so the
    // M real eigenpairs stay first in syevd's ascending order
    hipLaunchKernelGGL(k_nys_pad, dim3(blocks(R.Mp, 256), (unsigned)R.Mp), dim3(256), 0, st,
                       R.Kmm, R.M, R.Mp, 2.0 * R.dM * R.hp[3] + 1.0);
    KCHK();
  }
  sg_.end();
}

// W' = C L^-T;  A = r/sn2 - W'(W r);  objective (Ki, fused pass);  predict
void Runner::phase5(int64_t p, int64_t slot) {
  const CellRefs R = refs(p, slot);
  hipStream_t st = st_;
  const double sf2 = R.hp[3], isn2 = 1.0 / R.hp[4];
  const double dn = R.dn, dM = R.dM;
  double* Wt = R.C;  // n x M: W' = C L^-T, formed in place by batched()
  double* Av = fx_.Av;
  double* tv = fx_.tv;
  StageTimer& sg = sg_;
  sg.begin(S_APPLY, 2.0 * dM * dM * dn + 4.0 * dn * dM, 16.0 * dn * dM);
  hipLaunchKernelGGL(k_nys_vi, dim3(blocks(R.n, 256)), dim3(256), 0, st, R.r, R.n, isn2, Av);
  KCHK();
  oila::gemv(la_, st, true, {oila::Gemv{Wt, R.r, tv, R.in, R.iM, R.in, 1.0, 0.0}});     // tv = W r
  oila::gemv(la_, st, false, {oila::Gemv{Wt, tv, Av, R.in, R.iM, R.in, -1.0, 1.0}});   // A -= W' tv
  sg.end();
  if (obj_) {
    double* Ki = fx_.Ki;
    sg.begin(S_LOGDET, 2.0 * dn, 16.0 * dn);
    hipLaunchKernelGGL(k_nys_dot, dim3(1), dim3(256), 0, st, R.r, Av, R.n, R.rs + 0);
    KCHK();
    sg.end();
    if (kn_.fused) {
      // (W'W) tiles on the MFMA core, reduced against K, dK in the same kernel
      const int Tn = (int)blocks(R.n, 64), Tk = (int)blocks(R.M, 64);
      const int ntri = Tn * (Tn + 1) / 2;
      sg.begin(S_KI, dn * dn * dM, 8.0 * dn * dM);
      hipLaunchKernelGGL(k_nys_pack, dim3((unsigned)(Tn * Tk)), dim3(256), 0, st, Wt, R.n, R.M,
                         Tn, fx_.Wp);
      KCHK();
      sg.end();
      sg.begin(S_GRAD, dn * dn * dM, 0.0);
      hipLaunchKernelGGL(k_nys_grad_mfma, dim3((unsigned)ntri), dim3(256), 0, st, fx_.Wp, Tn, Tk, Av, R.sc,
                         R.sq, R.n, sf2, isn2, fx_.part);
      KCHK();
      hipLaunchKernelGGL(k_nys_partsum, dim3(1), dim3(256), 0, st, fx_.part, (int64_t)ntri, R.rs + 2);
      KCHK();
      sg.end();
    } else {
      // Ki = Vi - W'W (OI_NYS_FUSED=0 only: one full oila::gemm product; the
      // sweep below reads the lower half)
      sg.begin(S_KI, 2.0 * dn * dn * dM, 8.0 * dn * dn);
      oila::gemm(la_, st, false, true, {oila::Gemm{Wt, Wt, Ki, R.in, R.in, R.iM, R.in, R.in, R.in, -1.0, 0.0, 0}});
      hipLaunchKernelGGL(k_nys_diag, dim3(blocks(R.n, 256)), dim3(256), 0, st, Ki, R.n, R.n, nullptr,
                         0, isn2);
      KCHK();
      sg.end();
      // the lower triangle of Ki read once (~4 n^2 bytes); inputs and A cache-resident
      sg.begin(S_GRAD, 0.0, 4.0 * dn * dn);
      const unsigned nt = blocks(R.n, 64);
      hipLaunchKernelGGL(k_nys_grad, dim3(nt, nt), dim3(256), 0, st, Ki, Av, R.sc, R.sq, R.n, sf2, fx_.part);
      KCHK();
      hipLaunchKernelGGL(k_nys_partsum, dim3(1), dim3(256), 0, st, fx_.part, (int64_t)nt * nt, R.rs + 2);
      KCHK();
      sg.end();
    }
  }
  if (pred_) {
    // k* = SGPkernel(x, xs=xs); fs = mean + k*.A; k*'Ki k* = |k*|^2/sn2 - |W k*|^2
    sg.begin(S_PRED, 2.0 * dn * dM, 8.0 * dn * dM);
    double* ks = fx_.ks;
    double* kv = fx_.kv;
    hipLaunchKernelGGL(k_nys_scale, dim3(1), dim3(64), 0, st, (*tab_)[R.c].xs,
                       (int64_t)1, R.hp[0], R.hp[1], R.hp[2], fx_.xsc, nullptr);
    KCHK();
    hipLaunchKernelGGL(k_nys_cross, dim3(blocks(R.n, 256), 1), dim3(256), 0, st, R.sc, nullptr,
                       R.n, fx_.xsc, nullptr, sf2, ks, R.n);
    KCHK();
    hipLaunchKernelGGL(k_nys_dot, dim3(1), dim3(256), 0, st, ks, Av, R.n, R.rs + 7);
    KCHK();
    hipLaunchKernelGGL(k_nys_dot, dim3(1), dim3(256), 0, st, ks, ks, R.n, R.rs + 8);
    KCHK();
    oila::gemv(la_, st, true, {oila::Gemv{Wt, ks, kv, R.in, R.iM, R.in, 1.0, 0.0}});  // kv = W k*
    hipLaunchKernelGGL(k_nys_dot, dim3(1), dim3(256), 0, st, kv, kv, R.M, R.rs + 9);
    KCHK();
    sg.end();
  }
  if (multi_) predict_multi(R, Wt, Av);
}

// the cell's nt targets: Kxsx' (nt x n), fs, V' = Kxsx' W' (nt x M), then the
// fused covariance kernel on the packed operands (k_nys_cov_mfma)
void Runner::predict_multi(const CellRefs& R, const double* Wt, const double* Av) {
  const MultiDev& m = *multi_;
  const int64_t t0 = m.toffs[R.c], nt = m.toffs[R.c + 1] - t0;
  if (nt == 0) return;
  hipStream_t st = st_;
  const double dn = R.dn, dM = R.dM, dt = (double)nt;
  const int Tt = (int)blocks(nt, 64), Tkn = (int)blocks(R.n, 64), Tkm = (int)blocks(R.M, 64);
  sg_.begin(S_PREDM, 2.0 * dt * dn * dM + dt * dt * (dn + dM) + 2.0 * dt * dn,
            8.0 * (2.0 * dt * dn + 2.0 * dt * dM + dn * dM + (m.cov ? dt * dt : dt)));
  hipLaunchKernelGGL(k_nys_scale, dim3(blocks(nt, 256)), dim3(256), 0, st, m.xs + t0 * 3, nt, R.hp[0],
                     R.hp[1], R.hp[2], m.ts, nullptr);
  KCHK();
  hipLaunchKernelGGL(k_nys_cross_t, dim3(blocks(nt * R.n, 256)), dim3(256), 0, st, m.ts, nt, R.sc, R.n,
                     R.hp[3], m.KxT);
  KCHK();
  hipLaunchKernelGGL(k_nys_fs, dim3((unsigned)nt), dim3(256), 0, st, m.KxT, nt, R.n, Av, mean_,
                     m.fs + t0);
  KCHK();
  oila::gemm(la_, st, false, false,
             {oila::Gemm{m.KxT, Wt, m.VT, (int)nt, R.iM, R.in, (int)nt, R.in, (int)nt, 1.0, 0.0, 0}});  // V' = Kxsx' W'
  hipLaunchKernelGGL(k_nys_pack, dim3((unsigned)(Tt * Tkn)), dim3(256), 0, st, m.KxT, nt, R.n, Tt, m.Kp);
  KCHK();
  hipLaunchKernelGGL(k_nys_pack, dim3((unsigned)(Tt * Tkm)), dim3(256), 0, st, m.VT, nt, R.M, Tt, m.Vp);
  KCHK();
  double* cov = m.cov ? m.cov + m.coffs[R.c] : nullptr;
  hipLaunchKernelGGL(k_nys_cov_mfma, dim3((unsigned)(cov ? Tt * (Tt + 1) / 2 : Tt)), dim3(256), 0, st,
                     m.Kp, (int)blocks(R.n, 16), m.Vp, (int)blocks(R.M, 16), Tt, m.ts, nt, R.hp[3],
                     R.hp[4], cov, m.var + t0);
  KCHK();
  sg_.end();
}

}  // namespace oi_nys

using namespace oi_nys;

extern "C" int oi_nystrom_batch(const double* xyt, const double* y, const int64_t* offs,
                                int64_t ncell, const int64_t* sel, const int64_t* soffs,
                                const double* hyp, const double* xs, double mean, double* nlz,
                                double* grad, double* pred, int32_t* status,
                                const oi_options* opts) {
  Batch b{xyt, y, offs, ncell, sel, soffs};
  if (int rc = check_batch(b)) return rc;
  if (ncell == 0) return 0;
  if (!hyp || !status) return oi_set_last_error(OI_E_ARG, "null pointer");
  if ((nlz == nullptr) != (grad == nullptr))
    return oi_set_last_error(OI_E_ARG, "nlz and grad go together");
  const bool want_obj = nlz != nullptr, want_pred = pred != nullptr;
  if (want_pred && !xs) return oi_set_last_error(OI_E_ARG, "pred needs xs");
  if (int rc = check_hypers(hyp, ncell)) return rc;
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    BatchDev bd(b, want_pred ? xs : nullptr, o.device_inputs != 0, (hipStream_t)o.stream);
    Runner R(&bd.rows, b.nmax, b.mmax, ncell, o, want_obj, want_pred);
    std::vector<CellOut> out(ncell);
    R.run_all(ncell, hyp, mean, out.data());
    for (int64_t c = 0; c < ncell; ++c) {
      status[c] = out[c].status;
      if (want_obj) {
        nlz[c] = out[c].nlz;
        for (int q = 0; q < 5; ++q) grad[c * 5 + q] = out[c].grad[q];
      }
      if (want_pred) {
        pred[c * 3 + 0] = out[c].fs;
        pred[c * 3 + 1] = out[c].sd;
        pred[c * 3 + 2] = out[c].sprior;
      }
    }
    return 0;
  });
}

// one cell's scratch, and its covariance as it lies among the call's (not rounded)
int64_t oi_nystrom_multi_cell_doubles(int64_t n, int64_t M, int64_t nt, bool cov) {
  MultiDev::Scratch s;
  s.grow(n, M, nt);
  return MultiDev::doubles(0, -1, s) + (cov ? nt * nt : 0);
}

// Test hook (declared in no header, touches no device): a Runner's workspaces
// in doubles.  which 0: Fixed for cap cells (flags: 1 objective, 2 predict,
// 4 fused); 1: Slots for ch slots as allocated; 2: one slot unrounded, what
// sizes a chunk.  -1 for anything else.
extern "C" int64_t oi_test_nystrom_runner_doubles(int32_t which, int64_t nmax, int64_t mmax, int64_t cap_or_ch,
                                                  int32_t padq, int32_t flags) {
  if (nmax < 0 || mmax < 0 || mmax > INT32_MAX / 2 || cap_or_ch < 0 || padq < 0) return -1;
  switch (which) {
    case 0: return Fixed::doubles(nmax, mmax, cap_or_ch, flags & 1, flags & 2, flags & 4);
    case 1: return Slots::doubles(cap_or_ch, nmax, padded(mmax, padq));
    case 2: return Slots::doubles(1, nmax, padded(mmax, padq), 1);
  }
  return -1;
}

extern "C" int oi_nystrom_predict_multi(const double* xyt, const double* y, const int64_t* offs,
                                        int64_t ncell, const int64_t* sel, const int64_t* soffs,
                                        const double* hyp, const double* xs, const int64_t* toffs,
                                        double mean, double* fs, double* sd, double* cov,
                                        int32_t* status, const oi_options* opts) {
  Batch b{xyt, y, offs, ncell, sel, soffs};
  if (int rc = check_batch(b)) return rc;
  if (ncell == 0) return 0;
  if (int rc = oi_check_offs(toffs, ncell, 0, "toffs")) return rc;
  if (!hyp) return oi_set_last_error(OI_E_ARG, "null hyp");
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  const int64_t T = toffs[ncell];
  if (T > 0 && (!xs || !fs || !sd)) return oi_set_last_error(OI_E_ARG, "null xs / fs / sd");
  if (int rc = check_hypers(hyp, ncell)) return rc;
  // oila's operands take 32-bit byte offsets: Kxsx and cov stay below 2 GiB each
  constexpr int64_t LIM = 0x7FFFFFF0 / 8;
  std::vector<int64_t> coffs(ncell + 1, 0);
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t n = offs[c + 1] - offs[c], nt = toffs[c + 1] - toffs[c];
    if (nt * n >= LIM || nt * nt >= LIM)
      return oi_set_last_error(OI_E_ARG, "cell too large (Kxsx or cov reaches 2 GiB)");
    coffs[c + 1] = coffs[c] + nt * nt;
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    hipStream_t st = (hipStream_t)o.stream;
    const bool want_cov = cov != nullptr;
    // one cell's scratch (n x nt, M x nt and their tiles), the call's targets and outputs
    const int64_t budget = oi_workspace_budget(o);
    MultiDev::Scratch big;  // each scratch array at its largest
    for (int64_t c = 0; c < ncell; ++c) {
      const int64_t n = offs[c + 1] - offs[c], M = soffs[c + 1] - soffs[c], nt = toffs[c + 1] - toffs[c];
      if (oi_nystrom_multi_cell_doubles(n, M, nt, want_cov) > budget)
        throw NoMem{"a cell's Nystrom prediction workspace does not fit pool_bytes"};
      big.grow(n, M, nt);
    }
    const int64_t covd = want_cov ? coffs[ncell] : -1;
    const int64_t total = MultiDev::doubles(T, covd, big);
    if (total > budget)
      throw NoMem{"the call's targets and covariances do not fit pool_bytes: pass fewer cells per call"};
    DevBuf ws((size_t)total * 8);
    Carver cv{static_cast<double*>(ws.p)};
    MultiDev md;
    md.toffs = toffs;
    md.coffs = coffs.data();
    md.layout(cv, T, covd, big, xs, st);
    if (cv.off > total) throw HipErr{"oi_nystrom_predict_multi: workspace layout exceeds its estimate"};
    BatchDev bd(b, nullptr, o.device_inputs != 0, st);
    std::vector<CellOut> out(ncell);
    {
      Runner R(&bd.rows, b.nmax, b.mmax, ncell, o, false, false);
      R.set_multi(&md);
      R.run_all(ncell, hyp, mean, out.data());
    }
    // nothing was written so far: every output in one go, once all cells are done
    if (T > 0) {
      HC(hipMemcpyAsync(fs, md.fs, T * 8, hipMemcpyDeviceToHost, st));
      HC(hipMemcpyAsync(sd, md.var, T * 8, hipMemcpyDeviceToHost, st));
      if (want_cov) HC(hipMemcpyAsync(cov, md.cov, coffs[ncell] * 8, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
    }
    for (int64_t c = 0; c < ncell; ++c) {
      status[c] = out[c].status;
      const bool bad = out[c].status != 0;  // NB1's LinAlgError
      for (int64_t a = toffs[c]; a < toffs[c + 1]; ++a) {
        if (bad) fs[a] = NAN;
        sd[a] = bad ? NAN : std::sqrt(sd[a]);  // the returned diagonal's root, NaN below 0 as np.sqrt
      }
      if (bad && want_cov)
        for (int64_t e = coffs[c]; e < coffs[c + 1]; ++e) cov[e] = NAN;
    }
    return 0;
  });
}
