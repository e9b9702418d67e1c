// Prediction at many targets per cell with the full posterior covariance:
// the reference notebook's GPR(x, y, xs, ...) (GP_example.ipynb, code cell 1)
// with xs of size ns x 3 -- the arithmetic of GPR3D's predict step
// (GPR_CS2S3.py, GPR:173-182) with ns columns instead of one:
//
//   L = chol(K + sn2 I);  A = L^-T L^-1 (z - mean);  v = L^-1 Kxsx
//   fs = mean + Kxsx' A;  sd = sqrt(diag(Kxs - v'v));  cov = Kxs - v'v
//   lZ = -(z - mean).A/2 - sum log L_ii - n log(2 pi)/2
//
// A plain n x n path on oi_linalg.hip, apart from the main engine (whose
// kernels and bitwise-pinned results it does not touch).  Per chunk of cells
// -- as many as the workspace budget holds, cells of any n and nt together --
// every step is one launch (or one oila call) over the chunk, driven by an
// array of per-cell descriptors (PCell):
//
//   k_pm_scale   sc = (sqrt(3) x) / ell for the inputs and the targets
//   k_pm_kgen    lower 64-tiles of K + sn2 I, column-major, padded to Np = a
//                multiple of 64 with an identity (the upper triangle is never
//                generated or read)
//   k_pm_xgen    X = [Kxsx' ; (z - mean)'], (nt + 1) x n, column-major
//   oila::cholesky, then ONE oila::trsm_right_lt on X: X <- X L^-T, whose
//                first nt rows are v' and whose last row is zt' = (L^-1 r)'
//                -- the residual rides with the targets through one solve
//   k_pm_reduce  fs_t = mean + X_t . X_nt, sd_t = sqrt(sf2 - X_t . X_t),
//                lZ = -zt.zt/2 - sum log L_ii - n log(2 pi)/2, status
//   with cov:    k_pm_kxs (lower tiles of Kxs into the output), oila::gemm
//                (cov -= X[:nt] X[:nt]', lower tiles), k_pm_mirror (lower ->
//                full symmetric; NaN for a failed cell)
//
// All reductions run in a fixed order that depends on the cell alone, so a
// cell's results do not depend on its batch mates or on the chunking.
//
// Front, the part of a chunk up to the solved X, and the layout and checks of
// oi_dense.h are defined here too: oi_cv.hip (leave-one-out, leave-group-out),
// oi_sample.hip (posterior draws) and oi_grad.hip (the gradient's posterior,
// four rows of X per target from its own generator) run on them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "oi_dense.h"
#include "oi_matern.h"

#pragma clang fp contract(off)

namespace oi_dense {
namespace {

// ---------------------------------------------------------------- kernels --

// sc = np.sqrt(3.) * x / ell (SGPkernel, GPR:83) for inputs and targets
__global__ void __launch_bounds__(256) k_pm_scale(const PCell* __restrict__ cs) {
  const PCell c = cs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.n + c.nt) return;
  const double* src = i < c.n ? c.x + (size_t)i * 3 : c.xs + (size_t)(i - c.n) * 3;
  double* dst = i < c.n ? c.sc + (size_t)i * 3 : c.xsc + (size_t)(i - c.n) * 3;
  dst[0] = matern_scale(src[0], c.l0);
  dst[1] = matern_scale(src[1], c.l1);
  dst[2] = matern_scale(src[2], c.l2);
}

// 64 x 64 tile (it, jt), it >= jt, of K + sn2 I (GPR:175 np.linalg.cholesky's
// argument): entries with row >= column only; identity on the pad n..Np-1.
// Thread t: row t & 63, 16 columns from 16 (t >> 6) (stores coalesced along
// the column-major rows).
__global__ void __launch_bounds__(256) k_pm_kgen(const PCell* __restrict__ cs) {
  __shared__ double si[3][64], sj[3][64];
  const PCell c = cs[blockIdx.z];
  const int it = blockIdx.x, jt = blockIdx.y;
  if (it < jt || it * 64 >= c.Np) return;
  stage_tile(c.sc, c.n, it, jt, si, sj);
  const int m = threadIdx.x & 63, i = it * 64 + m;
  for (int q = 0; q < 16; ++q) {
    const int nn = (threadIdx.x >> 6) * 16 + q, j = jt * 64 + nn;
    if (i < j) continue;
    double v;
    if (i < c.n) {  // j <= i < n
      v = matern32(c.sf2, si[0][m] - sj[0][nn], si[1][m] - sj[1][nn], si[2][m] - sj[2][nn]);
      if (i == j) v = v + c.sn2;
    } else {
      v = i == j ? 1.0 : 0.0;
    }
    c.K[i + (size_t)c.Np * j] = v;
  }
}

// X[t + (nt + 1) i] = K(xs_t, x_i) for t < nt;  X[nt + (nt + 1) i] = z_i - mean
__global__ void __launch_bounds__(256) k_pm_xgen(const PCell* __restrict__ cs) {
  const PCell c = cs[blockIdx.y];
  const int rows = c.nt + 1;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)rows * c.n) return;
  const int t = (int)(e % rows);
  const int64_t i = e / rows;
  const double* a = c.sc + i * 3;
  double v;
  if (t < c.nt) {
    const double* b = c.xsc + (size_t)t * 3;
    v = matern32(c.sf2, a[0] - b[0], a[1] - b[1], a[2] - b[2]);
  } else {
    v = c.z[i] - c.mean;
  }
  c.X[e] = v;
}

// 64 x 64 tile (it, jt), it >= jt, of Kxs = SGPkernel(xs) into cov (whole
// diagonal tiles: the product that follows updates them whole); the diagonal
// is sf2 (1 + 0) exp(-0) = sf2 exactly
__global__ void __launch_bounds__(256) k_pm_kxs(const PCell* __restrict__ cs) {
  __shared__ double si[3][64], sj[3][64];
  const PCell c = cs[blockIdx.z];
  const int it = blockIdx.x, jt = blockIdx.y;
  if (!c.cov || it < jt || it * 64 >= c.nt) return;
  stage_tile(c.xsc, c.nt, it, jt, si, sj);
  const int m = threadIdx.x & 63, i = it * 64 + m;
  if (i >= c.nt) return;
  for (int q = 0; q < 16; ++q) {
    const int nn = (threadIdx.x >> 6) * 16 + q, j = jt * 64 + nn;
    if (j >= c.nt) continue;
    c.cov[i + (size_t)c.nt * j] =
        matern32(c.sf2, si[0][m] - sj[0][nn], si[1][m] - sj[1][nn], si[2][m] - sj[2][nn]);
  }
}

// Tile (it, jt), it >= jt, of cov: copy the entries below the diagonal to
// their mirror positions (the result is exactly symmetric, so row-major and
// column-major coincide); a failed cell gets NaN everywhere (GPR:187-191).
__global__ void __launch_bounds__(256) k_pm_mirror(const PCell* __restrict__ cs) {
  __shared__ double T[64 * 65];
  const PCell c = cs[blockIdx.z];
  const int it = blockIdx.x, jt = blockIdx.y;
  if (!c.cov || it < jt || it * 64 >= c.nt) return;
  const bool bad = *c.info != 0;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int m = e & 63, nn = e >> 6, i = it * 64 + m, j = jt * 64 + nn;
    double v = 0.0;
    if (i < c.nt && j < c.nt) {
      double* p = c.cov + i + (size_t)c.nt * j;
      if (bad) *p = NAN;
      v = *p;
    }
    T[nn * 65 + m] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int m = e & 63, nn = e >> 6, jj = jt * 64 + m, ii = it * 64 + nn;
    if (ii < c.nt && jj < ii) c.cov[jj + (size_t)c.nt * ii] = T[m * 65 + nn];
  }
}

// One pass over the solved X (rows t = 64 blockIdx.x + lane; wave w takes the
// columns i = w, w + 4, ...; the four wave partials are added in wave order):
//   fs_t = mean + X_t . X_nt (GPR:180), sd_t = sqrt(sf2 - X_t . X_t) (GPR:181,
//   no clamping: NaN for a negative argument, as np.sqrt)
// and, in the block that holds row nt (zt),
//   lZ = -zt.zt/2 - sum log L_ii - n log(2 pi)/2 (GPR:179), status.
__global__ void __launch_bounds__(256) k_pm_reduce(const PCell* __restrict__ cs) {
  __shared__ double ra[4][64], rb[4][64], red[4];
  const PCell c = cs[blockIdx.y];
  const int rows = c.nt + 1, r0 = blockIdx.x * 64;
  if (r0 >= rows) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = r0 + lane;
  double a = 0.0, b = 0.0;
  if (t < rows) {
    const double* Xt = c.X + t;
    const double* Xz = c.X + c.nt;
    for (int i = w; i < c.n; i += 4) {
      const size_t o = (size_t)rows * i;
      const double v = Xt[o], zt = Xz[o];
      a += v * zt;
      b += v * v;
    }
  }
  ra[w][lane] = a;
  rb[w][lane] = b;
  __syncthreads();
  const bool bad = *c.info != 0;
  if (w == 0 && t < c.nt) {
    a = ((ra[0][lane] + ra[1][lane]) + ra[2][lane]) + ra[3][lane];
    b = ((rb[0][lane] + rb[1][lane]) + rb[2][lane]) + rb[3][lane];
    c.fs[t] = bad ? NAN : c.mean + a;
    c.sd[t] = bad ? NAN : sqrt(c.sf2 - b);
  }
  if (c.nt >= r0 && c.nt < r0 + 64) {  // uniform over the block
    double v = 0.0;
    for (int i = threadIdx.x; i < c.n; i += 256) v += log(c.K[i + (size_t)c.Np * i]);
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int l = c.nt - r0;
      const double ld = ((red[0] + red[1]) + red[2]) + red[3];
      const double zz = ((ra[0][l] + ra[1][l]) + ra[2][l]) + ra[3][l];
      *c.lz = bad ? NAN : ((-zz / 2.0) - ld) - ((double)c.n * LOG2PI) / 2.0;
      *c.status = bad ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------------- host --

// opts.profile: HIP events around each stage of each chunk, summed per stage
// into oi_profile_json
enum { S_GEN, S_CHOL, S_SOLVE, S_REDUCE, S_COV, S_COUNT };
const char* kStage[S_COUNT] = {"pm_generate", "pm_cholesky", "pm_solve", "pm_reduce", "pm_cov"};

}  // namespace

DenseChunk dense_chunk(Carver& cv, const DenseIn& in, int64_t n0, int64_t nn, const double* xs, int64_t tt,
                       int64_t no, int64_t nc, int64_t cc) {
  DenseChunk k{in.xyt ? in.xyt + n0 * 3 : nullptr, in.z ? in.z + n0 : nullptr};
  if (in.host) {
    k.x = stage_host(cv, k.x, nn * 3, in.st);
    k.z = stage_host(cv, k.z, nn, in.st);
  }
  k.xs = stage_host(cv, xs, tt * 3, in.st);
  k.mu = cv.take(no);
  k.sd = cv.take(no);
  k.lz = cv.take(nc);
  k.flag = reinterpret_cast<int32_t*>(cv.take(nc));
  if (k.flag) HC(hipMemsetAsync(k.flag, 0, nc * 8, in.st));
  k.cov = cc >= 0 ? cv.take(cc) : nullptr;
  return k;
}
DenseCell dense_cell(Carver& cv, int64_t n, int64_t nt, bool loo, int64_t rpt) {
  const int64_t Np = up(n, 64);
  DenseCell a;
  a.sc = cv.take(3 * n);
  a.xsc = cv.take(3 * nt);
  a.K = cv.take(Np * Np);
  a.dinv = cv.take(Np * 64);
  a.wdt = loo ? cv.take(Np * 64) : nullptr;
  a.X = cv.take((rpt * nt + 1) * n);
  a.part = loo ? cv.take(Np / 64) : nullptr;
  return a;
}
int64_t dense_cell_doubles(int64_t n, int64_t nt, bool cov, bool host_inputs, bool loo, int64_t rpt) {
  Carver own, share{nullptr, 0, 1};
  dense_cell(own, n, nt, loo, rpt);
  dense_chunk(share, DenseIn{nullptr, nullptr, host_inputs, nullptr}, 0, n, nullptr, nt, loo ? n : nt, 1,
              cov ? (rpt * nt) * (rpt * nt) : -1);
  return own.off + share.off;
}

int dense_check(const double* xyt, const double* z, const int64_t* offs, const int64_t* toffs, int64_t ncell,
                const double* hyp, const int32_t* status, const char* missing, const DenseLimits& lim) {
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (!hyp) return oi_set_last_error(OI_E_ARG, "null hyp");
  if (offs[ncell] > 0 && (!xyt || !z)) return oi_set_last_error(OI_E_ARG, "null xyt / z");
  if (missing) return oi_set_last_error(OI_E_ARG, missing);
  constexpr int64_t LIM = 0x7FFFFFF0 / 8;  // oila's operands take 32-bit byte offsets
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t n = offs[c + 1] - offs[c], nt = toffs ? toffs[c + 1] - toffs[c] : 0, Np = up(n, 64),
                  Ntp = up(nt, 64);
    const int64_t rows = lim.rpt * nt;
    if (Np * Np >= LIM || (lim.X && (rows + 1 >= LIM || (rows + 1) * n >= LIM)) ||
        (lim.cov && rows * rows >= LIM) ||
        (lim.C && Ntp * Ntp >= LIM) || (lim.nsamp > 0 && nt >= LIM / lim.nsamp)) {
      std::vector<const char*> names{"K"};
      if (lim.X) names.push_back("X");
      if (lim.cov) names.push_back("cov");
      if (lim.C) names.push_back("C");
      if (lim.nsamp >= 0) names.push_back("nt * nsamp");
      std::string msg = "cell too large (";  // "K", "K, X or cov", "K, X, C or nt * nsamp"
      for (size_t q = 0; q < names.size(); ++q)
        msg += std::string(q == 0 ? "" : q + 1 < names.size() ? ", " : " or ") + names[q];
      return oi_set_last_error(OI_E_ARG, (msg + " reaches 2 GiB)").c_str());
    }
  }
  return 0;
}

Front::Front(const oi_options& o, const double* xyt, const double* z, const int64_t* offs, const double* hyp,
             double mean, bool loo, const char* const* stages, int count, int64_t rpt, XGen xgen)
    : o(o), in{xyt, z, o.device_inputs == 0, (hipStream_t)o.stream}, offs(offs), hyp(hyp), mean(mean), loo(loo),
      rpt(rpt), xgen(xgen), sg(stages, count) {
  la.bind(st);
  sg.on = o.profile != 0;
  sg.st = st;
}
void Front::begin(int64_t c0_, int64_t c1, const double* xs, int64_t tt, int64_t cc) {
  c0 = c0_;
  nc = c1 - c0;
  const int64_t nn = offs[c1] - offs[c0];
  cv = Carver{static_cast<double*>(ws.p)};
  k = dense_chunk(cv, in, offs[c0], nn, xs, tt, loo ? nn : tt, nc, cc);
  cells.clear();
  chol.clear();
  trsm.clear();
  nmax = ntmax = pts = xel = 0;
  fl_chol = fl_solve = by_gen = 0.0;
}
PCell& Front::add(int64_t c, int64_t nt, int64_t toff, DenseCell& a) {
  const int64_t r0 = offs[c] - offs[c0], n = offs[c + 1] - offs[c], q = c - c0;
  const double* h = hyp + c * 5;
  const int rows = (int)(rpt * nt + 1);  // of X
  a = dense_cell(cv, n, nt, loo, rpt);
  const PCell p{.x = k.x ? k.x + r0 * 3 : nullptr, .z = k.z ? k.z + r0 : nullptr, .xs = k.xs + toff * 3, .sc = a.sc,
                .xsc = a.xsc, .K = a.K, .X = a.X, .fs = k.mu + toff, .sd = k.sd + toff, .lz = k.lz + q,
                .info = k.flag + q, .status = k.flag + nc + q, .n = (int)n, .nt = (int)nt, .Np = (int)up(n, 64),
                .l0 = h[0], .l1 = h[1], .l2 = h[2], .sf2 = h[3], .sn2 = h[4], .mean = mean};
  if (n > 0) {
    chol.push_back(oila::Chol{p.K, a.dinv, p.info, p.Np, p.Np});
    trsm.push_back(oila::TrsmRLT{p.X, p.K, a.dinv, rows, p.n, rows, p.Np});
  }
  nmax = std::max(nmax, n);
  ntmax = std::max(ntmax, nt);
  pts = std::max(pts, n + nt);
  xel = std::max(xel, (int64_t)rows * n);
  const double dn = (double)n, dt = (double)(rows - 1);
  fl_chol += dn * dn * dn / 3.0;
  fl_solve += (dt + 1.0) * dn * dn;
  by_gen += 8.0 * (dn * dn / 2.0 + (dt + 1.0) * dn);
  cells.push_back(p);
  return cells.back();
}
const PCell* Front::factor(const char* entry, int s_gen, int s_chol, int s_solve) {
  if (cv.off > biggest) throw HipErr{std::string(entry) + ": workspace layout exceeds its estimate"};
  const PCell* dc = la.put(cells);
  const unsigned gz = (unsigned)nc, Tn = blocks(nmax, 64);
  sg.begin(s_gen, 0.0, by_gen);
  if (pts > 0) {
    hipLaunchKernelGGL(k_pm_scale, dim3(blocks(pts, 256), gz), dim3(256), 0, st, dc);
    KCHK();
  }
  if (nmax > 0) {
    hipLaunchKernelGGL(k_pm_kgen, dim3(Tn, Tn, gz), dim3(256), 0, st, dc);
    KCHK();
    if (xgen) {
      xgen(dc, nmax, ntmax, gz, st);
    } else {
      hipLaunchKernelGGL(k_pm_xgen, dim3(blocks(xel, 256), gz), dim3(256), 0, st, dc);
    }
    KCHK();
  }
  sg.end();
  sg.begin(s_chol, fl_chol, 0.0);
  oila::cholesky(la, st, chol);
  sg.end();
  sg.begin(s_solve, fl_solve, 0.0);
  oila::trsm_right_lt(la, st, trsm);
  sg.end();
  return dc;
}
void Front::reduce(int stage, double by_red, const PCell* dc) {
  sg.begin(stage, by_red / 2.0, by_red);
  hipLaunchKernelGGL(k_pm_reduce, dim3(blocks(ntmax + 1, 64), (unsigned)nc), dim3(256), 0, st, dc);
  KCHK();
  sg.end();
}
void Front::finish(int32_t* status) {
  HC(hipMemcpyAsync(status + c0, k.flag + nc, nc * 4, hipMemcpyDeviceToHost, st));
  HC(hipStreamSynchronize(st));
  sg.flush();
  la.reset();
}

}  // namespace oi_dense

using namespace oi_dense;

extern "C" int oi_gpr_predict_multi(const double* xyt, const double* z, const int64_t* offs,
                                    int64_t ncell, const double* xs, const int64_t* toffs,
                                    double mean, const double* hyp, double* fs, double* sd,
                                    double* lz, double* cov, int32_t* status,
                                    const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (int rc = oi_check_offs(toffs, ncell, 0, "toffs")) return rc;
  if (ncell == 0) return 0;
  const char* missing = toffs[ncell] > 0 && (!xs || !fs || !sd) ? "null xs / fs / sd" : nullptr;
  if (int rc = dense_check(xyt, z, offs, toffs, ncell, hyp, status, missing, {.X = true, .cov = true, .nsamp = -1}))
    return rc;
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    const bool want_cov = cov != nullptr;
    Front fr(o, xyt, z, offs, hyp, mean, false, kStage, S_COUNT);
    const std::vector<int64_t> cuts = fr.plan(ncell, CHUNK_SLACK, "prediction", [&](int64_t c) {
      return dense_cell_doubles(offs[c + 1] - offs[c], toffs[c + 1] - toffs[c], want_cov, fr.in.host, false);
    });
    hipStream_t st = fr.st;
    std::vector<oila::Gemm> syrk;
    int64_t covoff = 0;  // cell c's covariance starts at sum_{k<c} nt_k^2
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, t0 = toffs[c0], tt = toffs[c1] - t0;
      int64_t cc = 0;
      for (int64_t c = c0; c < c1; ++c) cc += (toffs[c + 1] - toffs[c]) * (toffs[c + 1] - toffs[c]);
      fr.begin(c0, c1, xs + t0 * 3, tt, want_cov ? cc : -1);
      const DenseChunk& k = fr.k;
      syrk.clear();
      int64_t co = 0;
      double fl_cov = 0.0, by_red = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const int64_t nt = toffs[c + 1] - toffs[c];
        DenseCell a;
        PCell& p = fr.add(c, nt, toffs[c] - t0, a);
        p.cov = want_cov ? k.cov + co : nullptr;
        if (want_cov && nt > 0)  // cov <- Kxs - X[:nt] X[:nt]' on the lower tiles
          syrk.push_back(oila::Gemm{p.X, p.X, p.cov, p.nt, p.nt, p.n, p.nt + 1, p.nt + 1, p.nt, -1.0, 1.0, 1});
        co += nt * nt;
        const double dn = (double)p.n, dt = (double)nt;
        fl_cov += dt * dt * dn;
        by_red += 8.0 * (dt + 1.0) * dn;
      }
      const PCell* dc = fr.factor("oi_gpr_predict_multi", S_GEN, S_CHOL, S_SOLVE);
      const unsigned gz = (unsigned)nc, Tt = blocks(fr.ntmax, 64);
      fr.reduce(S_REDUCE, by_red, dc);
      if (want_cov && fr.ntmax > 0) {
        fr.sg.begin(S_COV, fl_cov, 8.0 * (double)cc);
        hipLaunchKernelGGL(k_pm_kxs, dim3(Tt, Tt, gz), dim3(256), 0, st, dc);
        KCHK();
        oila::gemm(fr.la, st, false, true, syrk);
        hipLaunchKernelGGL(k_pm_mirror, dim3(Tt, Tt, gz), dim3(256), 0, st, dc);
        KCHK();
        fr.sg.end();
      }
      if (tt > 0) {
        HC(hipMemcpyAsync(fs + t0, k.mu, tt * 8, hipMemcpyDeviceToHost, st));
        HC(hipMemcpyAsync(sd + t0, k.sd, tt * 8, hipMemcpyDeviceToHost, st));
      }
      if (lz) HC(hipMemcpyAsync(lz + c0, k.lz, nc * 8, hipMemcpyDeviceToHost, st));
      if (want_cov && cc > 0) HC(hipMemcpyAsync(cov + covoff, k.cov, cc * 8, hipMemcpyDeviceToHost, st));
      covoff += cc;
      fr.finish(status);
    }
    return 0;
  });
}

// Test hook (not in oi.h): what the chunk planner counts for one cell of path
// 0 oi_gpr_predict_multi, 1 oi_gpr_loo, 2 oi_svgp_predict / oi_svgp_elbo,
// 3 oi_nystrom_predict_multi; flags 1 cov, 2 host inputs, 4 ELBO; -1: no such path
extern "C" int64_t oi_test_cell_doubles(int32_t path, int64_t n, int64_t nt, int64_t M, int32_t flags) {
  const bool cov = flags & 1, host = flags & 2, elbo = flags & 4;
  switch (path) {
    case 0: return dense_cell_doubles(n, nt, cov, host, false);
    case 1: return dense_cell_doubles(n, 0, false, host, true);
    case 2: return oi_svgp_cell_doubles((int)M, n, cov, host, elbo);
    case 3: return oi_nystrom_multi_cell_doubles(n, M, nt, cov);
  }
  return -1;
}
