// Posterior of the field and of its gradient per cell at given hypers:
// oi_gpr_predict_grad (include/oi_ext.h).  For target t the joint vector is
// u_t = (f, df/dx, df/dy, df/dt)(xs_t), component k = 0..3; with C (4 nt x n,
// row 4 t + k the covariance of u_t,k with the observations) and P (4 nt x
// 4 nt, the joint prior), both from oi_matern.h's derivative expressions,
//
//   L = chol(K + sn2 I);  zt = L^-1 (z - mean);  V = L^-1 C'
//   E[u] = (mean, 0, 0, 0) per target + V' zt;   Cov[u] = P - V'V
//
// The path runs on oi_dense.h's Front with four rows of X per target: X is
// (4 nt + 1) x n with leading dimension 4 nt + 1, row 4 t + k as C's and the
// last row the residual z - mean.  Rows 4 t are oi_gpr_predict_multi's rows t
// bit for bit (matern32_qe), every row goes through the one solve on its own,
// and k_pg_reduce keeps k_pm_reduce's summation order, so fs and sd are that
// entry's bit for bit.
//
//   k_pg_xgen    X, one thread per (target, observation) pair: Q and e once,
//                its four rows written side by side; one per residual
//   oila::cholesky, then ONE oila::trsm_right_lt over all 4 nt + 1 rows
//   k_pg_reduce  one pass over the solved X: a 256-thread block takes 64 rows =
//                16 targets, lane = row, so a target's four components sit in
//                four adjacent lanes and exchange their values inside the quad;
//                grad, gsd, fs, sd, blk, status
//   with cov:    k_pg_prior (lower 64-tiles of P through LDS), oila::gemm
//                (cov -= X[:4 nt] X[:4 nt]', lower tiles), k_pg_mirror
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/oi_ext.h"
#include "oi_dense.h"
#include "oi_matern.h"

#pragma clang fp contract(off)

using namespace oi_dense;

namespace {

constexpr int RPT = 4;  // rows of X per target

struct GCell {
  const double* xsc;    // nt x 3 scaled targets
  const double* X;      // (4 nt + 1) x n, solved
  double* grad;         // nt x 3
  double* gsd;          // nt x 3
  double* blk;          // nt x 16
  double* cov;          // 4 nt x 4 nt (leading dimension 4 nt) or null
  double* fs;           // nt
  double* sd;           // nt
  const int32_t* info;  // the cell's Cholesky
  int32_t* status;      // 1
  int n, nt;
  double l0, l1, l2, sf2, mean;
};

// Column i of X: rows 4 t .. 4 t + 3 = the covariance of u_t with observation
// i (a = xs_t, b = x_i; the differences are k_pm_xgen's, observation minus
// target, which is -d), row 4 nt = z_i - mean
__global__ void __launch_bounds__(256) k_pg_xgen(const PCell* __restrict__ cs) {
  const PCell c = cs[blockIdx.y];
  const int units = c.nt + 1, rows = RPT * c.nt + 1;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)units * c.n) return;
  const int t = (int)(e % units);
  const int64_t i = e / units;
  double* X = c.X + (size_t)rows * i + (size_t)RPT * t;
  if (t == c.nt) {
    X[0] = c.z[i] - c.mean;
    return;
  }
  const double* a = c.sc + i * 3;
  const double* b = c.xsc + (size_t)t * 3;
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  const double Q = matern_dist(d0, d1, d2), ex = exp(-Q);
  X[0] = matern32_qe(c.sf2, Q, ex);
  X[1] = matern32_d1(c.sf2, ex, d0, matern_c(c.l0));
  X[2] = matern32_d1(c.sf2, ex, d1, matern_c(c.l1));
  X[3] = matern32_d1(c.sf2, ex, d2, matern_c(c.l2));
}
// one thread per pair and per residual element: at most (ntmax + 1) nmax in a cell
void launch_xgen(const PCell* dc, int64_t nmax, int64_t ntmax, unsigned nc, hipStream_t st) {
  hipLaunchKernelGGL(k_pg_xgen, dim3(blocks((ntmax + 1) * nmax, 256), nc), dim3(256), 0, st, dc);
}

// One pass over the solved X (rows r = 64 blockIdx.x + lane = 4 t + k; wave w
// takes the columns i = w, w + 4, ...; the four wave partials are added in
// wave order, as k_pm_reduce's): a = X_r . X_4nt and b_j = X_r . X_(4t+j),
// whose factors come from the lanes of r's quad, so that b_j of lane k and b_k
// of lane j are sums of the same products in the same order:
//   mean of u_t,k = (k == 0 ? mean : 0) + a,  blk_t[k][j] = P_t[k][j] - b_j,
//   sd_t = sqrt(blk_t[0][0]), gsd_t,k = sqrt(blk_t[k][k]) (no clamping)
// with P_t = diag(sf2, sf2 c_x^2, sf2 c_y^2, sf2 c_t^2) as k_pg_prior forms it
// at Q = 0; the block that holds row 4 nt writes the status.
__global__ void __launch_bounds__(256) k_pg_reduce(const GCell* __restrict__ cs) {
  __shared__ double ra[4][64], rb[4][4][64];
  const GCell c = cs[blockIdx.y];
  const int last = RPT * c.nt, rows = last + 1, r0 = blockIdx.x * 64;
  if (r0 >= rows) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = r0 + lane, q0 = lane & ~3;
  const bool live = r < last;
  double a = 0.0, b[4] = {0.0, 0.0, 0.0, 0.0};
  const double* Xr = c.X + (live ? r : 0);
  const double* Xz = c.X + last;
  for (int i = w; i < c.n; i += 4) {  // uniform over the wave
    const size_t o = (size_t)rows * i;
    const double v = live ? Xr[o] : 0.0, zt = Xz[o];
    a += v * zt;
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] += v * __shfl(v, q0 + j, 64);
  }
  ra[w][lane] = a;
#pragma unroll
  for (int j = 0; j < 4; ++j) rb[j][w][lane] = b[j];
  __syncthreads();
  const bool bad = *c.info != 0;
  if (w == 0 && live) {
    const int t = r >> 2, k = r & 3;
    a = ((ra[0][lane] + ra[1][lane]) + ra[2][lane]) + ra[3][lane];
    double pk = matern32_qe(c.sf2, 0.0, 1.0);  // the value's prior variance, sf2 exactly
    if (k > 0) {                               // a derivative's, sf2 c_k^2
      const double ck = matern_c(k == 1 ? c.l0 : k == 2 ? c.l1 : c.l2);
      pk = matern32_d2(c.sf2, 1.0, 0.0, 0.0, 0.0, ck, ck, true);
    }
    double vk = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double s = ((rb[j][0][lane] + rb[j][1][lane]) + rb[j][2][lane]) + rb[j][3][lane];
      const double p = (j == k ? pk : 0.0) - s;
      if (j == k) vk = p;
      c.blk[(size_t)t * 16 + k * 4 + j] = bad ? NAN : p;
    }
    if (k == 0) {
      c.fs[t] = bad ? NAN : c.mean + a;
      c.sd[t] = bad ? NAN : sqrt(vk);
    } else {
      c.grad[(size_t)t * 3 + (k - 1)] = bad ? NAN : a;
      c.gsd[(size_t)t * 3 + (k - 1)] = bad ? NAN : sqrt(vk);
    }
  }
  if (last >= r0 && last < r0 + 64 && threadIdx.x == 0) *c.status = bad ? 1 : 0;
}

// 64 x 64 tile (it, jt), it >= jt, of P into cov (whole diagonal tiles: the
// product that follows updates them whole): 16 x 16 pairs of targets, one per
// thread, Q and e once per pair and its 4 x 4 block from matern32_joint (a =
// the row's target, b = the column's); at Q = 0 the block is the diagonal
// (sf2, sf2 c_x^2, sf2 c_y^2, sf2 c_t^2) and +0 elsewhere
__global__ void __launch_bounds__(256) k_pg_prior(const GCell* __restrict__ cs) {
  __shared__ double si[3][16], sj[3][16];
  const GCell c = cs[blockIdx.z];
  const int it = blockIdx.x, jt = blockIdx.y;
  if (!c.cov || it < jt || it * 16 >= c.nt) return;
  const int th = threadIdx.x;
  if (th < 96) {
    const int side = th / 48, d = (th % 48) / 16, u = th & 15, t = (side ? jt : it) * 16 + u;
    (side ? sj : si)[d][u] = t < c.nt ? c.xsc[(size_t)t * 3 + d] : 0.0;
  }
  __syncthreads();
  const int ui = th & 15, uj = th >> 4, ti = it * 16 + ui, tj = jt * 16 + uj;
  if (ti >= c.nt || tj >= c.nt) return;
  double d[3], nd[3];
  for (int q = 0; q < 3; ++q) {
    d[q] = si[q][ui] - sj[q][uj];
    nd[q] = sj[q][uj] - si[q][ui];
  }
  const double cc[3] = {matern_c(c.l0), matern_c(c.l1), matern_c(c.l2)};
  const double Q = matern_dist(d[0], d[1], d[2]), ex = exp(-Q);
  const size_t m = (size_t)RPT * c.nt;
  double* out = c.cov + (size_t)RPT * ti + m * ((size_t)RPT * tj);
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k + m * l] = matern32_joint(c.sf2, Q, ex, d, nd, cc, k, l);
}

// k_pm_mirror for the order 4 nt: tile (it, jt), it >= jt, of cov, the entries
// below the diagonal copied to their mirror positions (exactly symmetric, so
// row-major and column-major coincide); NaN everywhere for a failed cell
__global__ void __launch_bounds__(256) k_pg_mirror(const GCell* __restrict__ cs) {
  __shared__ double T[64 * 65];
  const GCell c = cs[blockIdx.z];
  const int it = blockIdx.x, jt = blockIdx.y, m = RPT * c.nt;
  if (!c.cov || it < jt || it * 64 >= m) return;
  const bool bad = *c.info != 0;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int mm = e & 63, nn = e >> 6, i = it * 64 + mm, j = jt * 64 + nn;
    double v = 0.0;
    if (i < m && j < m) {
      double* p = c.cov + i + (size_t)m * j;
      if (bad) *p = NAN;
      v = *p;
    }
    T[nn * 65 + mm] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int mm = e & 63, nn = e >> 6, jj = jt * 64 + mm, ii = it * 64 + nn;
    if (ii < m && jj < ii) c.cov[jj + (size_t)m * ii] = T[mm * 65 + nn];
  }
}

enum { G_GEN, G_CHOL, G_SOLVE, G_REDUCE, G_COV, G_COUNT };
const char* kGradStage[G_COUNT] = {"pg_generate", "pg_cholesky", "pg_solve", "pg_reduce", "pg_cov"};

constexpr int64_t GRAD_SLACK = CHUNK_SLACK + 3 * 32;  // three more chunk-wide arrays

// What the gradient adds to oi_gpr_predict_multi's layout, chunk-wide with the
// cells' parts back to back in the ABI's own layout: grad and gsd, 3 tt each,
// and blk, 16 tt (always: k_pg_reduce takes gsd from it)
struct GradChunk {
  double *grad, *gsd, *blk;
};
GradChunk grad_chunk(Carver& cv, int64_t tt) {
  GradChunk k;
  k.grad = cv.take(3 * tt);
  k.gsd = cv.take(3 * tt);
  k.blk = cv.take(16 * tt);
  return k;
}
int64_t grad_cell_doubles(int64_t n, int64_t nt, bool cov, bool host_inputs) {
  Carver share{nullptr, 0, 1};
  grad_chunk(share, nt);
  return dense_cell_doubles(n, nt, cov, host_inputs, false, RPT) + share.off;
}

}  // namespace

extern "C" int oi_gpr_predict_grad(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                                   const double* xs, const int64_t* toffs, double mean, const double* hyp,
                                   double* grad, double* gsd, double* fs, double* sd, double* blk, double* cov,
                                   int32_t* status, const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (int rc = oi_check_offs(toffs, ncell, 0, "toffs")) return rc;
  if (ncell == 0) return 0;
  const char* missing = toffs[ncell] > 0 && (!xs || !grad || !gsd) ? "null xs / grad / gsd" : nullptr;
  if (int rc = dense_check(xyt, z, offs, toffs, ncell, hyp, status, missing,
                           {.X = true, .cov = cov != nullptr, .nsamp = -1, .rpt = RPT}))
    return rc;
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    const bool want_cov = cov != nullptr;
    Front fr(o, xyt, z, offs, hyp, mean, false, kGradStage, G_COUNT, RPT, launch_xgen);
    const std::vector<int64_t> cuts = fr.plan(ncell, GRAD_SLACK, "gradient", [&](int64_t c) {
      return grad_cell_doubles(offs[c + 1] - offs[c], toffs[c + 1] - toffs[c], want_cov, fr.in.host);
    });
    hipStream_t st = fr.st;
    std::vector<GCell> gcells;
    std::vector<oila::Gemm> syrk;
    int64_t covoff = 0;  // cell c's covariance starts at sum_{k<c} 16 nt_k^2
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, t0 = toffs[c0], tt = toffs[c1] - t0;
      int64_t cc = 0;
      for (int64_t c = c0; c < c1; ++c) cc += RPT * RPT * (toffs[c + 1] - toffs[c]) * (toffs[c + 1] - toffs[c]);
      fr.begin(c0, c1, xs + t0 * 3, tt, want_cov ? cc : -1);
      const DenseChunk& k = fr.k;
      const GradChunk gk = grad_chunk(fr.cv, tt);
      gcells.clear();
      syrk.clear();
      int64_t co = 0;
      double fl_cov = 0.0, by_red = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const int64_t nt = toffs[c + 1] - toffs[c], tq = toffs[c] - t0;
        DenseCell a;
        PCell& p = fr.add(c, nt, tq, a);
        p.cov = nullptr;  // the order differs: the GCell carries it
        const int m = (int)(RPT * nt);
        gcells.push_back(GCell{a.xsc, p.X, gk.grad + tq * 3, gk.gsd + tq * 3, gk.blk + tq * 16,
                               want_cov ? k.cov + co : nullptr, p.fs, p.sd, p.info, p.status, p.n, p.nt, p.l0, p.l1,
                               p.l2, p.sf2, p.mean});
        if (want_cov && nt > 0)  // cov <- P - X[:4 nt] X[:4 nt]' on the lower tiles
          syrk.push_back(oila::Gemm{p.X, p.X, gcells.back().cov, m, m, p.n, m + 1, m + 1, m, -1.0, 1.0, 1});
        co += (int64_t)m * m;
        const double dn = (double)p.n, dm = (double)m;
        fl_cov += dm * dm * dn;
        by_red += 8.0 * (dm + 1.0) * dn;
      }
      fr.factor("oi_gpr_predict_grad", G_GEN, G_CHOL, G_SOLVE);
      const GCell* dg = fr.la.put(gcells);
      const unsigned gz = (unsigned)nc, Tt = blocks(RPT * fr.ntmax, 64);
      fr.sg.begin(G_REDUCE, 2.5 * by_red / 4.0, by_red);
      hipLaunchKernelGGL(k_pg_reduce, dim3(blocks(RPT * fr.ntmax + 1, 64), gz), dim3(256), 0, st, dg);
      KCHK();
      fr.sg.end();
      if (want_cov && fr.ntmax > 0) {
        fr.sg.begin(G_COV, fl_cov, 8.0 * (double)cc);
        hipLaunchKernelGGL(k_pg_prior, dim3(Tt, Tt, gz), dim3(256), 0, st, dg);
        KCHK();
        oila::gemm(fr.la, st, false, true, syrk);
        hipLaunchKernelGGL(k_pg_mirror, dim3(Tt, Tt, gz), dim3(256), 0, st, dg);
        KCHK();
        fr.sg.end();
      }
      if (tt > 0) {
        HC(hipMemcpyAsync(grad + t0 * 3, gk.grad, tt * 24, hipMemcpyDeviceToHost, st));
        HC(hipMemcpyAsync(gsd + t0 * 3, gk.gsd, tt * 24, hipMemcpyDeviceToHost, st));
        if (fs) HC(hipMemcpyAsync(fs + t0, k.mu, tt * 8, hipMemcpyDeviceToHost, st));
        if (sd) HC(hipMemcpyAsync(sd + t0, k.sd, tt * 8, hipMemcpyDeviceToHost, st));
        if (blk) HC(hipMemcpyAsync(blk + t0 * 16, gk.blk, tt * 128, hipMemcpyDeviceToHost, st));
      }
      if (want_cov && cc > 0) HC(hipMemcpyAsync(cov + covoff, k.cov, cc * 8, hipMemcpyDeviceToHost, st));
      covoff += cc;
      fr.finish(status);
    }
    return 0;
  });
}

// Test hook (in no header): the workspace the chunk planner counts for one
// cell of oi_gpr_predict_grad; flags as oi_test_cell_doubles (1 cov, 2 host
// inputs); touches no device
extern "C" int64_t oi_test_grad_cell_doubles(int64_t n, int64_t nt, int32_t flags) {
  return grad_cell_doubles(n, nt, (flags & 1) != 0, (flags & 2) != 0);
}
