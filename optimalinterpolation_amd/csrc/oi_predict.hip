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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "oi_host.h"
#include "oi_linalg.h"
#include "oi_matern.h"

#pragma clang fp contract(off)

namespace {

constexpr double LOG2PI = 1.8378770664093453;  // np.log(2 * np.pi)

// One cell of a chunk (device pointers; the row of the descriptor array that
// every kernel below indexes with its block's cell coordinate).
struct PCell {
  const double* x;   // n x 3 inputs
  const double* z;   // n observations
  const double* xs;  // nt x 3 targets
  double* sc;        // n x 3 scaled inputs
  double* xsc;       // nt x 3 scaled targets
  double* K;         // Np x Np: K + sn2 I, then its Cholesky factor (lower)
  double* X;         // (nt + 1) x n, leading dimension nt + 1
  double* cov;       // nt x nt (leading dimension nt) or null
  double* fs;        // nt
  double* sd;        // nt
  double* lz;        // 1
  int32_t* info;     // the Cholesky's info
  int32_t* status;   // 1
  int n, nt, Np;
  double l0, l1, l2, sf2, sn2, mean;
};

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

// Workspace of one cell in doubles.  Per-cell arrays are rounded to 32 doubles
// (256 bytes); the chunk-wide arrays (inputs, targets, outputs, cov, flags)
// are the cells' parts back to back, so their share is not rounded.
//   scaled inputs / targets 3 (n + nt), K Np^2, the factor's diagonal-block
//   inverses 64 Np, X (nt + 1) n, cov nt^2, fs + sd 2 nt, targets 3 nt,
//   inputs 4 n (host inputs only), lZ + flags 2
int64_t cell_doubles(int64_t n, int64_t nt, bool cov, bool host_inputs) {
  const int64_t Np = up(n, 64);
  int64_t d = up(3 * n, 32) + up(3 * nt, 32) + Np * Np + Np * 64 + up((nt + 1) * n, 32);
  d += (cov ? nt * nt : 0) + 2 * nt + 3 * nt + (host_inputs ? 4 * n : 0) + 2;
  return d;
}
constexpr int64_t CHUNK_SLACK = 8 * 32;  // rounding of the chunk-wide arrays (doubles)
constexpr int64_t CHUNK_CELLS = 4096;    // cells per chunk at most (launch grids, descriptor arrays)

}  // namespace

extern "C" int oi_gpr_predict_multi(const double* xyt, const double* z, const int64_t* offs,
                                    int64_t ncell, const double* xs, const int64_t* toffs,
                                    double mean, const double* hyp, double* fs, double* sd,
                                    double* lz, double* cov, int32_t* status,
                                    const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (int rc = oi_check_offs(toffs, ncell, 0, "toffs")) return rc;
  if (ncell == 0) return 0;
  const int64_t N = offs[ncell], T = toffs[ncell];
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (!hyp) return oi_set_last_error(OI_E_ARG, "null hyp");
  if (N > 0 && (!xyt || !z)) return oi_set_last_error(OI_E_ARG, "null xyt / z");
  if (T > 0 && (!xs || !fs || !sd)) return oi_set_last_error(OI_E_ARG, "null xs / fs / sd");
  // oila's operands take 32-bit byte offsets: K, X and cov stay below 2 GiB each
  constexpr int64_t LIM = 0x7FFFFFF0 / 8;
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t n = offs[c + 1] - offs[c], nt = toffs[c + 1] - toffs[c], Np = up(n, 64);
    if (Np * Np >= LIM || (nt + 1) * n >= LIM || nt * nt >= LIM)
      return oi_set_last_error(OI_E_ARG, "cell too large (K, X or cov reaches 2 GiB)");
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    const bool host_in = o.device_inputs == 0, want_cov = cov != nullptr;
    hipStream_t st = (hipStream_t)o.stream;
    const auto [cuts, biggest] = plan_chunks(ncell, o, CHUNK_SLACK, CHUNK_CELLS, "prediction", [&](int64_t c) {
      return cell_doubles(offs[c + 1] - offs[c], toffs[c + 1] - toffs[c], want_cov, host_in);
    });
    DevBuf ws((size_t)biggest * 8);
    oila::Stager la;
    la.bind(st);
    StageTimer sg(kStage, S_COUNT);
    sg.on = o.profile != 0;
    sg.st = st;
    std::vector<PCell> cells;
    std::vector<oila::Chol> chol;
    std::vector<oila::TrsmRLT> trsm;
    std::vector<oila::Gemm> syrk;
    int64_t covoff = 0;  // cell c's covariance starts at sum_{k<c} nt_k^2
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0;
      const int64_t n0 = offs[c0], nn = offs[c1] - n0, t0 = toffs[c0], tt = toffs[c1] - t0;
      int64_t cc = 0;
      for (int64_t c = c0; c < c1; ++c) cc += (toffs[c + 1] - toffs[c]) * (toffs[c + 1] - toffs[c]);
      Carver cv{static_cast<double*>(ws.p)};
      const double* dx = xyt ? xyt + n0 * 3 : nullptr;
      const double* dz = z ? z + n0 : nullptr;
      if (host_in && nn > 0) {
        double* hx = cv.take(nn * 3);
        double* hz = cv.take(nn);
        HC(hipMemcpyAsync(hx, xyt + n0 * 3, nn * 3 * 8, hipMemcpyHostToDevice, st));
        HC(hipMemcpyAsync(hz, z + n0, nn * 8, hipMemcpyHostToDevice, st));
        dx = hx;
        dz = hz;
      }
      double* dxs = cv.take(tt * 3);
      if (tt > 0) HC(hipMemcpyAsync(dxs, xs + t0 * 3, tt * 3 * 8, hipMemcpyHostToDevice, st));
      double* dfs = cv.take(tt);
      double* dsd = cv.take(tt);
      double* dlz = cv.take(nc);
      int32_t* dflag = reinterpret_cast<int32_t*>(cv.take(nc));  // info [nc], status [nc]
      double* dcov = want_cov ? cv.take(cc) : nullptr;
      HC(hipMemsetAsync(dflag, 0, nc * 8, st));
      cells.clear();
      chol.clear();
      trsm.clear();
      syrk.clear();
      int64_t nmax = 0, ntmax = 0, pts = 0, xel = 0, co = 0;
      double fl_chol = 0.0, fl_solve = 0.0, fl_cov = 0.0, by_gen = 0.0, by_red = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const int64_t n = offs[c + 1] - offs[c], nt = toffs[c + 1] - toffs[c], Np = up(n, 64);
        const double* h = hyp + c * 5;
        PCell p;
        p.x = dx ? dx + (offs[c] - n0) * 3 : nullptr;
        p.z = dz ? dz + (offs[c] - n0) : nullptr;
        p.xs = dxs + (toffs[c] - t0) * 3;
        p.sc = cv.take(3 * n);
        p.xsc = cv.take(3 * nt);
        p.K = cv.take(Np * Np);
        double* dinv = cv.take(Np * 64);
        p.X = cv.take((nt + 1) * n);
        p.cov = want_cov ? dcov + co : nullptr;
        p.fs = dfs + (toffs[c] - t0);
        p.sd = dsd + (toffs[c] - t0);
        p.lz = dlz + (c - c0);
        p.info = dflag + (c - c0);
        p.status = dflag + nc + (c - c0);
        p.n = (int)n;
        p.nt = (int)nt;
        p.Np = (int)Np;
        p.l0 = h[0];
        p.l1 = h[1];
        p.l2 = h[2];
        p.sf2 = h[3];
        p.sn2 = h[4];
        p.mean = mean;
        cells.push_back(p);
        if (n > 0) {
          chol.push_back(oila::Chol{p.K, dinv, p.info, p.Np, p.Np});
          trsm.push_back(oila::TrsmRLT{p.X, p.K, dinv, p.nt + 1, p.n, p.nt + 1, p.Np});
        }
        if (want_cov && nt > 0)  // cov <- Kxs - X[:nt] X[:nt]' on the lower tiles
          syrk.push_back(oila::Gemm{p.X, p.X, p.cov, p.nt, p.nt, p.n, p.nt + 1, p.nt + 1, p.nt, -1.0, 1.0, 1});
        co += nt * nt;
        nmax = std::max(nmax, n);
        ntmax = std::max(ntmax, nt);
        pts = std::max(pts, n + nt);
        xel = std::max(xel, (nt + 1) * n);
        const double dn = (double)n, dt = (double)nt;
        fl_chol += dn * dn * dn / 3.0;
        fl_solve += (dt + 1.0) * dn * dn;
        fl_cov += dt * dt * dn;
        by_gen += 8.0 * (dn * dn / 2.0 + (dt + 1.0) * dn);
        by_red += 8.0 * (dt + 1.0) * dn;
      }
      if (cv.off > biggest) throw HipErr{"oi_gpr_predict_multi: workspace layout exceeds its estimate"};
      const PCell* dc = la.put(cells);
      const unsigned gz = (unsigned)nc;
      const unsigned Tn = blocks(nmax, 64), Tt = blocks(ntmax, 64);
      sg.begin(S_GEN, 0.0, by_gen);
      if (pts > 0) {
        hipLaunchKernelGGL(k_pm_scale, dim3(blocks(pts, 256), gz), dim3(256), 0, st, dc);
        KCHK();
      }
      if (nmax > 0) {
        hipLaunchKernelGGL(k_pm_kgen, dim3(Tn, Tn, gz), dim3(256), 0, st, dc);
        KCHK();
        hipLaunchKernelGGL(k_pm_xgen, dim3(blocks(xel, 256), gz), dim3(256), 0, st, dc);
        KCHK();
      }
      sg.end();
      sg.begin(S_CHOL, fl_chol, 0.0);
      oila::cholesky(la, st, chol);
      sg.end();
      sg.begin(S_SOLVE, fl_solve, 0.0);
      oila::trsm_right_lt(la, st, trsm);
      sg.end();
      sg.begin(S_REDUCE, by_red / 2.0, by_red);
      hipLaunchKernelGGL(k_pm_reduce, dim3(blocks(ntmax + 1, 64), gz), dim3(256), 0, st, dc);
      KCHK();
      sg.end();
      if (want_cov && ntmax > 0) {
        sg.begin(S_COV, fl_cov, 8.0 * (double)cc);
        hipLaunchKernelGGL(k_pm_kxs, dim3(Tt, Tt, gz), dim3(256), 0, st, dc);
        KCHK();
        oila::gemm(la, st, false, true, syrk);
        hipLaunchKernelGGL(k_pm_mirror, dim3(Tt, Tt, gz), dim3(256), 0, st, dc);
        KCHK();
        sg.end();
      }
      if (tt > 0) {
        HC(hipMemcpyAsync(fs + t0, dfs, tt * 8, hipMemcpyDeviceToHost, st));
        HC(hipMemcpyAsync(sd + t0, dsd, tt * 8, hipMemcpyDeviceToHost, st));
      }
      if (lz) HC(hipMemcpyAsync(lz + c0, dlz, nc * 8, hipMemcpyDeviceToHost, st));
      HC(hipMemcpyAsync(status + c0, dflag + nc, nc * 4, hipMemcpyDeviceToHost, st));
      if (want_cov && cc > 0) HC(hipMemcpyAsync(cov + covoff, dcov, cc * 8, hipMemcpyDeviceToHost, st));
      covoff += cc;
      // the next chunk reuses the workspace and the descriptor ring
      HC(hipStreamSynchronize(st));
      sg.flush();
      la.reset();
    }
    return 0;
  });
}
