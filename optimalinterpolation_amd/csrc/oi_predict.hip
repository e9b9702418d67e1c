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
// The second half of the file is oi_gpr_loo (include/oi_loo.h): leave-one-out
// cross-validation per cell on the same generation, Cholesky and solve, plus
// the block-column sweep k_loo_sweep over L^-1.  The third part is oi_gpr_lgo
// (include/oi_lgo.h): leave-group-out cross-validation, which keeps the sweep's
// L^-T and forms the blocks of K~^-1 that the groups touch (k_lgo_gram).  The
// fourth is oi_gpr_sample (include/oi_sample.h): joint draws from the posterior,
// a second factorisation (of the posterior covariance) and a device generator.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/oi_lgo.h"
#include "../../include/oi_loo.h"
#include "../../include/oi_sample.h"
#include "oi_gemm.h"
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

constexpr int64_t CHUNK_SLACK = 8 * 32;  // rounding of the chunk-wide arrays (doubles)
constexpr int64_t CHUNK_CELLS = 4096;    // cells per chunk at most (launch grids, descriptor arrays)

// The two layout functions below are the one description of both entry points'
// workspace.  A cell's size for the chunk planner is the same functions on
// counting Carvers: its own arrays rounded to 32 doubles (256 bytes), plus its
// unrounded share of the chunk-wide arrays (the cells' parts back to back).
struct DenseIn {  // the caller's inputs
  const double *xyt, *z;
  bool host;  // staged into the workspace chunk by chunk
  hipStream_t st;
};

// Chunk-wide, nc cells with nn rows from row n0 and tt targets: inputs 4 nn
// (host inputs only), targets 3 tt, two outputs of `no` doubles (fs, sd per
// target; leave-one-out: mu, sd per row), lZ / lpl + flags 2 nc, cov cc or none (< 0)
struct DenseChunk {
  const double *x, *z, *xs;
  double *mu, *sd, *lz;
  int32_t* flag;  // info [nc], status [nc], zeroed
  double* cov;
};
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
// One cell's own: scaled inputs 3 n and targets 3 nt, K Np^2, the factor's
// diagonal-block inverses 64 Np, X (nt + 1) n; leave-one-out adds their
// transposes 64 Np and the lpl partials Np / 64 (the sweep writes the panels of
// W' into K above the diagonal blocks and needs no n x n array of its own).
struct DenseCell {
  double *sc, *xsc, *K, *dinv, *wdt, *X, *part;
};
DenseCell dense_cell(Carver& cv, int64_t n, int64_t nt, bool loo) {
  const int64_t Np = up(n, 64);
  DenseCell a;
  a.sc = cv.take(3 * n);
  a.xsc = cv.take(3 * nt);
  a.K = cv.take(Np * Np);
  a.dinv = cv.take(Np * 64);
  a.wdt = loo ? cv.take(Np * 64) : nullptr;
  a.X = cv.take((nt + 1) * n);
  a.part = loo ? cv.take(Np / 64) : nullptr;
  return a;
}
int64_t dense_cell_doubles(int64_t n, int64_t nt, bool cov, bool host_inputs, bool loo) {
  Carver own, share{nullptr, 0, 1};
  dense_cell(own, n, nt, loo);
  dense_chunk(share, DenseIn{nullptr, nullptr, host_inputs, nullptr}, 0, n, nullptr, nt, loo ? n : nt, 1,
              cov ? nt * nt : -1);
  return own.off + share.off;
}

// What oi_gpr_predict_multi and oi_gpr_loo share per chunk: staging, carving,
// the PCell descriptors, generation, Cholesky and solve; status copy and hand-over.
struct Front {
  const DenseIn in;
  const int64_t* offs;
  const double* hyp;
  const double mean;
  const bool loo;
  hipStream_t st = in.st;
  oila::Stager la;
  StageTimer sg;
  std::vector<PCell> cells;
  std::vector<oila::Chol> chol;
  std::vector<oila::TrsmRLT> trsm;
  DenseChunk k;    // the chunk's arrays
  int64_t c0, nc;  // its cells
  int64_t nmax, ntmax, pts, xel;
  double fl_chol, fl_solve, by_gen;

  Front(const oi_options& o, const double* xyt, const double* z, const int64_t* offs, const double* hyp, double mean,
        bool loo, const char* const* stages, int count)
      : in{xyt, z, o.device_inputs == 0, (hipStream_t)o.stream}, offs(offs), hyp(hyp), mean(mean), loo(loo),
        sg(stages, count) {
    la.bind(st);
    sg.on = o.profile != 0;
    sg.st = st;
  }
  // cells c0 .. c1 - 1 with their tt targets at xs and cc covariance elements
  void begin(Carver& cv, int64_t c0_, int64_t c1, const double* xs, int64_t tt, int64_t cc) {
    c0 = c0_;
    nc = c1 - c0;
    const int64_t nn = offs[c1] - offs[c0];
    k = dense_chunk(cv, in, offs[c0], nn, xs, tt, loo ? nn : tt, nc, cc);
    cells.clear();
    chol.clear();
    trsm.clear();
    nmax = ntmax = pts = xel = 0;
    fl_chol = fl_solve = by_gen = 0.0;
  }
  // the chunk's next cell c: its arrays into a, and its descriptor's common fields
  PCell& add(Carver& cv, int64_t c, int64_t nt, DenseCell& a) {
    const int64_t r0 = offs[c] - offs[c0], n = offs[c + 1] - offs[c], q = c - c0;
    const double* h = hyp + c * 5;
    a = dense_cell(cv, n, nt, loo);
    const PCell p{.x = k.x ? k.x + r0 * 3 : nullptr, .z = k.z ? k.z + r0 : nullptr, .sc = a.sc, .K = a.K, .X = a.X,
                  .info = k.flag + q, .status = k.flag + nc + q, .n = (int)n, .nt = (int)nt, .Np = (int)up(n, 64),
                  .l0 = h[0], .l1 = h[1], .l2 = h[2], .sf2 = h[3], .sn2 = h[4], .mean = mean};
    if (n > 0) {
      chol.push_back(oila::Chol{p.K, a.dinv, p.info, p.Np, p.Np});
      trsm.push_back(oila::TrsmRLT{p.X, p.K, a.dinv, p.nt + 1, p.n, p.nt + 1, p.Np});
    }
    nmax = std::max(nmax, n);
    ntmax = std::max(ntmax, nt);
    pts = std::max(pts, n + nt);
    xel = std::max(xel, (nt + 1) * n);
    const double dn = (double)n, dt = (double)nt;
    fl_chol += dn * dn * dn / 3.0;
    fl_solve += (dt + 1.0) * dn * dn;
    by_gen += 8.0 * (dn * dn / 2.0 + (dt + 1.0) * dn);
    cells.push_back(p);
    return cells.back();
  }
  // descriptors up (returned), then generate, factor and solve under the caller's stage ids
  const PCell* factor(int s_gen, int s_chol, int s_solve) {
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
      hipLaunchKernelGGL(k_pm_xgen, dim3(blocks(xel, 256), gz), dim3(256), 0, st, dc);
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
  // after the caller's tail; the next chunk reuses the workspace and the descriptor ring
  void finish(int32_t* status) {
    HC(hipMemcpyAsync(status + c0, k.flag + nc, nc * 4, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    sg.flush();
    la.reset();
  }
};

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
    const bool want_cov = cov != nullptr;
    Front fr(o, xyt, z, offs, hyp, mean, false, kStage, S_COUNT);
    const auto [cuts, biggest] = plan_chunks(ncell, o, CHUNK_SLACK, CHUNK_CELLS, "prediction", [&](int64_t c) {
      return dense_cell_doubles(offs[c + 1] - offs[c], toffs[c + 1] - toffs[c], want_cov, fr.in.host, false);
    });
    DevBuf ws((size_t)biggest * 8);
    hipStream_t st = fr.st;
    std::vector<oila::Gemm> syrk;
    int64_t covoff = 0;  // cell c's covariance starts at sum_{k<c} nt_k^2
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, t0 = toffs[c0], tt = toffs[c1] - t0;
      int64_t cc = 0;
      for (int64_t c = c0; c < c1; ++c) cc += (toffs[c + 1] - toffs[c]) * (toffs[c + 1] - toffs[c]);
      Carver cv{static_cast<double*>(ws.p)};
      fr.begin(cv, c0, c1, xs + t0 * 3, tt, want_cov ? cc : -1);
      const DenseChunk& k = fr.k;
      syrk.clear();
      int64_t co = 0;
      double fl_cov = 0.0, by_red = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const int64_t nt = toffs[c + 1] - toffs[c];
        DenseCell a;
        PCell& p = fr.add(cv, c, nt, a);
        p.xs = k.xs + (toffs[c] - t0) * 3;
        p.xsc = a.xsc;
        p.cov = want_cov ? k.cov + co : nullptr;
        p.fs = k.mu + (toffs[c] - t0);
        p.sd = k.sd + (toffs[c] - t0);
        p.lz = k.lz + (c - c0);
        if (want_cov && nt > 0)  // cov <- Kxs - X[:nt] X[:nt]' on the lower tiles
          syrk.push_back(oila::Gemm{p.X, p.X, p.cov, p.nt, p.nt, p.n, p.nt + 1, p.nt + 1, p.nt, -1.0, 1.0, 1});
        co += nt * nt;
        const double dn = (double)p.n, dt = (double)nt;
        fl_cov += dt * dt * dn;
        by_red += 8.0 * (dt + 1.0) * dn;
      }
      if (cv.off > biggest) throw HipErr{"oi_gpr_predict_multi: workspace layout exceeds its estimate"};
      const PCell* dc = fr.factor(S_GEN, S_CHOL, S_SOLVE);
      const unsigned gz = (unsigned)nc, Tt = blocks(fr.ntmax, 64);
      fr.sg.begin(S_REDUCE, by_red / 2.0, by_red);
      hipLaunchKernelGGL(k_pm_reduce, dim3(blocks(fr.ntmax + 1, 64), gz), dim3(256), 0, st, dc);
      KCHK();
      fr.sg.end();
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

// ===========================================================================
// Leave-one-out cross-validation per cell (include/oi_loo.h; Rasmussen &
// Williams, GPML 5.4.2) at given hypers, from ONE factorisation:
//
//   r = z - mean;  K~ = K + sn2 I = L L';  zt = L^-1 r;  W = L^-1
//   q_c = [K~^-1]_cc = sum_r W_rc^2;  alpha_c = [K~^-1 r]_c = sum_r W_rc zt_r
//   mu_c = z_c - alpha_c / q_c;  sd_c = sqrt(1 / q_c)
//   lpl = sum_c [ -log(2 pi)/2 - log sd_c - (z_c - mu_c)^2 / (2 sd_c^2) ]
//
// K~ and its factor come from the kernels and oila calls above (PCell with no
// target); zt is the 1 x n row X through oila::trsm_right_lt.  k_loo_sweep
// then builds W one 64-column block panel per workgroup and folds every
// finished 64 x 64 tile into q and alpha; W itself is never kept beyond the
// panel, and K~^-1 is never formed.
// ===========================================================================
namespace {

struct LCell {
  double* K;           // Np x Np: L below the diagonal blocks; the sweep writes W' = L^-T
                       // into the strict upper BLOCK triangle (block (j, i), i > j, = W_ij')
  const double* dinv;  // Np / 64 inverses of L's diagonal blocks (oila::Chol)
  double* wdt;         // Np / 64 x 4096: their transposes (the panels' first B operand)
  const double* zt;    // n: L^-1 (z - mean)
  const double* z;     // n
  double* mu;          // n
  double* sd;          // n
  double* part;        // Np / 64 partial sums of lpl, one per block column
  double* lpl;         // 1
  const int32_t* info; // the Cholesky's info
  int32_t* status;     // 1
  int n, Np;
};
struct LItem {
  int cell, j;  // one workgroup: block column j of cell `cell` (of the chunk)
};

typedef __attribute__((address_space(1))) double gdbl;
typedef __attribute__((address_space(1))) dv2 gdv2w;

#define LOO_LD 72  // LDS row stride of the S / W tile (doubles)

// Block column j of W = L^-1 for one cell, top-down, per 64 x 64 tile
//   W_jj = Dinv_jj;   W_ij = -Dinv_ii (sum_{k=j}^{i-1} L_ik W_kj),  i > j
// 256 threads, wave w owns the 32 x 32 quadrant (32 (w >> 1), 32 (w & 1)) as
// 2 x 2 blocks of v_mfma_f64_16x16x4f64 (the oi_gemm.h layout).
//   S = sum_k L_ik W_kj is ONE product over the inner index kk = 64 j .. 64 i:
//   A row kk = L(64 i.., kk) (a column of K, contiguous), B row kk = W(kk, 64 j..)
//   = the finished tiles' transposes, which this workgroup stored at
//   K(64 j.., kk) -- also a contiguous column of K (the first 64 kk come from
//   wdt, the transpose of Dinv_jj).  Chunks 16 deep, two-deep register ring,
//   two LDS buffers, global-address-space loads, as gemm1_kmajor.
//   W_ij = -Dinv_ii S: S goes to LDS as the B operand, Dinv_ii (column-major =
//   k-major) fills the four staging slots as the A operand.
// Epilogue of every tile, rows r < n only (the pad's identity rows enter no
// sum), per column c: 16 rows in order per wave-quarter, the four quarters
// added in order, tiles i ascending -- a fixed order that depends on the cell
// alone.  The workgroup reads back only what it stored itself, behind a
// __syncthreads(); no other workgroup touches block row j above the diagonal.
__global__ void __launch_bounds__(256) k_loo_sweep(const LCell* __restrict__ cs,
                                                   const LItem* __restrict__ items) {
  __shared__ __attribute__((aligned(16))) double stg[4 * STAGE_A];  // 2 x (A, B) chunks; then Dinv_ii; then sums
  __shared__ __attribute__((aligned(16))) double tile[64 * LOO_LD];  // S, then W_ij, [row][column]
  const LItem item = items[blockIdx.x];
  const LCell c = cs[item.cell];
  const int j = item.j, T = c.Np / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  const size_t Np = (size_t)c.Np;
  gdbl* const K = (gdbl*)c.K;
  const gdbl* const zt = (const gdbl*)c.zt;
  double qa = 0.0, aa = 0.0;  // threads 0..63: column 64 j + t

  // tile[r][cc] = W_ij[r][cc] is complete: add its columns' sums and store its
  // transpose at dst[cc + ldd r]
  auto epilogue = [&](int i, gdbl* dst, size_t ldd) __attribute__((always_inline)) {
    const int rows = min(64, c.n - 64 * i);
    const int cc = t & 63;
    double s2 = 0.0, sz = 0.0;
    for (int r = 16 * w; r < 16 * w + 16; ++r) {
      if (r < rows) {
        const double v = tile[r * LOO_LD + cc];
        s2 += v * v;
        sz += v * zt[64 * i + r];
      }
    }
    stg[w * 64 + cc] = s2;
    stg[256 + w * 64 + cc] = sz;
    for (int e = t; e < 4096; e += 256) dst[(e & 63) + ldd * (size_t)(e >> 6)] = tile[(e >> 6) * LOO_LD + (e & 63)];
    __syncthreads();
    if (t < 64) {
      qa += ((stg[t] + stg[64 + t]) + stg[128 + t]) + stg[192 + t];
      aa += ((stg[256 + t] + stg[320 + t]) + stg[384 + t]) + stg[448 + t];
    }
    __syncthreads();
  };

  {  // i = j: W_jj = Dinv_jj (column-major)
    const gdbl* D = (const gdbl*)c.dinv + (size_t)j * 4096;
    for (int e = t; e < 4096; e += 256) tile[(e & 63) * LOO_LD + (e >> 6)] = D[e];
    __syncthreads();
    epilogue(j, (gdbl*)c.wdt + (size_t)j * 4096, 64);
  }

  const int sk = t >> 5, sm = (t & 31) * 2;  // this thread's two 16 B pieces of a 16 x 64 chunk: rows sk, sk + 8
  for (int i = j + 1; i < T; ++i) {
    const int nch = 4 * (i - j);
    const double* Ai = c.K + 64 * i;  // A row kk: Ai[m + Np kk]
    const double* Bj = c.K + 64 * j;  // B row kk >= 64 (j + 1): Bj[n + Np kk]
    StageRegs r0, r1;
    auto load = [&](int ch, StageRegs& q) __attribute__((always_inline)) {
      const size_t kk = (size_t)64 * j + (size_t)KC * ch + sk;
      const double* pa = Ai + sm + Np * kk;
      const bool first = ch < 4;  // uniform: rows of W_jj' from wdt
      const double* pb = first ? c.wdt + (size_t)j * 4096 + sm + 64 * (size_t)(KC * ch + sk) : Bj + sm + Np * kk;
      const size_t ldb = first ? 64 : Np;
      q.a0 = gload2(pa);
      q.a1 = gload2(pa + Np * 8);
      q.b0 = gload2(pb);
      q.b1 = gload2(pb + ldb * 8);
    };
    auto store = [&](int buf, const StageRegs& q) __attribute__((always_inline)) {
      double* As = stg + buf * 2 * STAGE_A;
      double* Bs = As + STAGE_A;
      *(dv2*)(As + sk * LDSA + sm) = q.a0;
      *(dv2*)(As + (sk + 8) * LDSA + sm) = q.a1;
      *(dv2*)(Bs + sk * LDSA + sm) = q.b0;
      *(dv2*)(Bs + (sk + 8) * LDSA + sm) = q.b1;
    };
    Quad acc;
    quad_zero(acc);
    auto compute = [&](const double* As, const double* Bs, int ldb, int ksteps) __attribute__((always_inline)) {
#pragma unroll
      for (int kq = 0; kq < ksteps; ++kq) {
        const int k = kq * 4 + fk;
        const double a0 = As[k * LDSA + 32 * wr + fr];
        const double a1 = As[k * LDSA + 32 * wr + 16 + fr];
        const double b0 = Bs[k * ldb + 32 * wc + fr];
        const double b1 = Bs[k * ldb + 32 * wc + 16 + fr];
        acc.c[0][0] = MFMA64(a0, b0, acc.c[0][0]);
        acc.c[0][1] = MFMA64(a0, b1, acc.c[0][1]);
        acc.c[1][0] = MFMA64(a1, b0, acc.c[1][0]);
        acc.c[1][1] = MFMA64(a1, b1, acc.c[1][1]);
      }
    };
    // S = sum over kk (nch is a multiple of 4; the prefetches past the end
    // re-read the last chunk, unused: see gemm2_kmajor)
    load(0, r0);
    load(1, r1);
    store(0, r0);
    __syncthreads();
    for (int ch = 0; ch < nch; ch += 2) {
      load(min(ch + 2, nch - 1), r0);
      compute(stg, stg + STAGE_A, LDSA, KC / 4);
      store(1, r1);
      __syncthreads();
      load(min(ch + 3, nch - 1), r1);
      compute(stg + 2 * STAGE_A, stg + 3 * STAGE_A, LDSA, KC / 4);
      if (ch + 2 < nch) store(0, r0);
      __syncthreads();
    }
    // Dinv_ii (A[m][k] = D[m + 64 k]) into the staging slots, S into the tile
    {
      const gdbl* D = (const gdbl*)c.dinv + (size_t)i * 4096;
      dv2 d[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) d[q] = *(const gdv2w*)(D + 2 * (t + 256 * q));
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int p = t + 256 * q;
        *(dv2*)(stg + (p >> 5) * LDSA + 2 * (p & 31)) = d[q];
      }
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[acc1_row(mb, r) * LOO_LD + acc1_col(nb)] = acc.c[mb][nb][r];
    __syncthreads();
    quad_zero(acc);
    compute(stg, tile, LOO_LD, 16);
    __syncthreads();
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[acc1_row(mb, r) * LOO_LD + acc1_col(nb)] = -acc.c[mb][nb][r];
    __syncthreads();
    epilogue(i, K + 64 * j + Np * 64 * (size_t)i, Np);
  }

  // mu, sd and this block column's share of lpl (wave 0: one lane per column)
  if (t < 64) {
    const int col = 64 * j + t;
    const bool bad = *c.info != 0;
    double term = 0.0;
    if (col < c.n) {
      const double zc = c.z[col];
      const double mu = bad ? NAN : zc - aa / qa;
      const double sd = bad ? NAN : sqrt(1.0 / qa);
      c.mu[col] = mu;
      c.sd[col] = sd;
      const double d = zc - mu;
      term = ((-LOG2PI / 2.0) - log(sd)) - (d * d) / ((2.0 * sd) * sd);
    }
    for (int o = 32; o > 0; o >>= 1) term += __shfl_down(term, o, 64);
    if (t == 0) c.part[j] = term;
  }
}

// lpl = the block columns' partial sums added in index order; status
__global__ void __launch_bounds__(256) k_loo_finish(const LCell* __restrict__ cs, int nc) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nc) return;
  const LCell c = cs[q];
  double s = 0.0;
  for (int j = 0; j < c.Np / 64; ++j) s += c.part[j];
  *c.lpl = s;
  *c.status = *c.info != 0 ? 1 : 0;
}

enum { L_GEN, L_CHOL, L_SOLVE, L_SWEEP, L_COUNT };
const char* kLooStage[L_COUNT] = {"loo_generate", "loo_cholesky", "loo_solve", "loo_sweep"};

}  // namespace

extern "C" int oi_gpr_loo(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                          double mean, const double* hyp, double* mu, double* sd, double* lpl,
                          int32_t* status, const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (ncell == 0) return 0;
  const int64_t N = offs[ncell];
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (!hyp) return oi_set_last_error(OI_E_ARG, "null hyp");
  if (N > 0 && (!xyt || !z)) return oi_set_last_error(OI_E_ARG, "null xyt / z");
  if (N > 0 && (!mu || !sd)) return oi_set_last_error(OI_E_ARG, "null mu / sd");
  constexpr int64_t LIM = 0x7FFFFFF0 / 8;  // oila's operands take 32-bit byte offsets
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t Np = up(offs[c + 1] - offs[c], 64);
    if (Np * Np >= LIM) return oi_set_last_error(OI_E_ARG, "cell too large (K reaches 2 GiB)");
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    Front fr(o, xyt, z, offs, hyp, mean, true, kLooStage, L_COUNT);
    const auto [cuts, biggest] = plan_chunks(ncell, o, CHUNK_SLACK, CHUNK_CELLS, "leave-one-out", [&](int64_t c) {
      return dense_cell_doubles(offs[c + 1] - offs[c], 0, false, fr.in.host, true);
    });
    DevBuf ws((size_t)biggest * 8);
    hipStream_t st = fr.st;
    std::vector<LCell> lcells;
    std::vector<LItem> items;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, n0 = offs[c0], nn = offs[c1] - n0;
      Carver cv{static_cast<double*>(ws.p)};
      fr.begin(cv, c0, c1, nullptr, 0, -1);
      const DenseChunk& k = fr.k;
      lcells.clear();
      items.clear();
      for (int64_t c = c0; c < c1; ++c) {
        DenseCell a;
        const PCell& p = fr.add(cv, c, 0, a);
        lcells.push_back(LCell{p.K, a.dinv, a.wdt, p.X, p.z, k.mu + (offs[c] - n0), k.sd + (offs[c] - n0), a.part,
                               k.lz + (c - c0), p.info, p.status, p.n, p.Np});
        for (int j = 0; j < p.Np / 64; ++j) items.push_back(LItem{(int)(c - c0), j});
      }
      if (cv.off > biggest) throw HipErr{"oi_gpr_loo: workspace layout exceeds its estimate"};
      // the longest block columns first (j ascending: Np / 64 - j tiles each);
      // ties keep the cells' order
      std::stable_sort(items.begin(), items.end(), [&](const LItem& a, const LItem& b) {
        return lcells[a.cell].Np / 64 - a.j > lcells[b.cell].Np / 64 - b.j;
      });
      const LCell* dl = fr.la.put(lcells);
      fr.factor(L_GEN, L_CHOL, L_SOLVE);
      fr.sg.begin(L_SWEEP, fr.fl_chol, 0.0);
      if (!items.empty()) {
        const LItem* di = fr.la.put(items);
        hipLaunchKernelGGL(k_loo_sweep, dim3((unsigned)items.size()), dim3(256), 0, st, dl, di);
        KCHK();
      }
      hipLaunchKernelGGL(k_loo_finish, dim3(blocks(nc, 256)), dim3(256), 0, st, dl, (int)nc);
      KCHK();
      fr.sg.end();
      if (nn > 0) {
        HC(hipMemcpyAsync(mu + n0, k.mu, nn * 8, hipMemcpyDeviceToHost, st));
        HC(hipMemcpyAsync(sd + n0, k.sd, nn * 8, hipMemcpyDeviceToHost, st));
      }
      if (lpl) HC(hipMemcpyAsync(lpl + c0, k.lz, nc * 8, hipMemcpyDeviceToHost, st));
      fr.finish(status);
    }
    return 0;
  });
}

// ===========================================================================
// Leave-group-out cross-validation per cell (include/oi_lgo.h; GPML 5.4.2 in
// block form) at given hypers, from ONE factorisation per cell:
//
//   r = z - mean;  K~ = L L';  W = L^-1;  U = W';  zt = W r;  alpha = U zt
//   Q = K~^-1 = U U';  per group G:  Q_GG = C C'
//   X_G = [I_g ; alpha_G'] C^-T  ((g + 1) x g):  e_i = X_i . X_g,
//   sd_i^2 = X_i . X_i,  d2 = X_g . X_g,  mu_i = z_i - e_i
//   lpd_G = -d2 / 2 + sum_k log C_kk - g log(2 pi) / 2;  lpl = sum_G lpd_G
//
// The host sorts a cell's observations so that groups are contiguous (groups
// in the order of first appearance, members in observation order: lgo_plan)
// and lists the aligned 64 x 64 tiles of Q that some group touches.  The front
// half and k_loo_sweep run unchanged on the sorted cell; the sweep leaves U in
// K's strict upper BLOCK triangle (K[row + Np col] = U(row, col) for a column
// block above the row block) and the diagonal blocks U_AA in wdt.  k_lgo_gram
// then forms the listed tiles of Q IN PLACE in K's lower block triangle, which
// holds only the dead L and which no k_lgo_gram workgroup reads: no ordering
// between workgroups and no second n x n array.  k_lgo_pack copies every
// group's block (at an arbitrary, possibly odd offset) into an aligned gp x gp
// buffer, gp = g rounded up to 64, padded with an identity, for oila::cholesky
// and oila::trsm_right_lt (one descriptor per group); k_lgo_reduce and
// k_lgo_finish sum in a fixed order that depends on the cell's partition alone.
// ===========================================================================
namespace {

struct GCell {
  double* K;          // Np x Np after k_loo_sweep; tiles of Q go into the lower block triangle
  const double* wdt;  // Np / 64 x 4096: U_AA, k-major with stride 64
  const double* zt;   // n: L^-1 (z - mean)
  double* alpha;      // Np: K~^-1 (z - mean) (rows >= n unused)
  int n, Np;
};
struct GItem {
  int cell, A, B;  // one workgroup: tile (A, B), A >= B, of Q of cell `cell` (of the chunk)
};
// One group of a chunk (k_lgo_pack, k_lgo_reduce)
struct GGroup {
  const double* K;      // its cell's K (Q in the lower block triangle)
  const double* alpha;  // its cell's alpha
  const double* z;      // its cell's observations, sorted
  double* P;            // gp x gp: Q_GG with an identity pad, then its factor C
  double* X;            // (g + 1) x g, leading dimension g + 1
  double *mu, *sd, *lpd, *d2;  // the chunk's output rows (observations' own order)
  const int32_t* perm;  // its cell's sorted row -> row of the chunk's outputs
  double* glpd;         // 1: lpd_G
  const int32_t* ginfo; // the group Cholesky's info
  const int32_t* cinfo; // the cell Cholesky's info
  int c0, g, gp, Np;    // first sorted row, size, padded size; the cell's Np
};
struct FCell {
  const double* glpd;    // ng
  const int32_t* ginfo;  // ng
  double* lpl;           // 1
  const int32_t* info;
  int32_t* status;
  int ng;
};

// sorted row k of the chunk <- row perm[k] of the caller's device arrays
__global__ void __launch_bounds__(256) k_lgo_gather(const double* __restrict__ x, const double* __restrict__ z,
                                                    const int32_t* __restrict__ perm, double* __restrict__ gx,
                                                    double* __restrict__ gz, int64_t nn) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nn) return;
  const int64_t s = perm[k];
  gx[3 * k] = x[3 * s];
  gx[3 * k + 1] = x[3 * s + 1];
  gx[3 * k + 2] = x[3 * s + 2];
  gz[k] = z[s];
}

// Tile (A, B), A >= B, of Q = U U' for one cell:
//   Q_AB[m][nn] = sum_{kk >= 64 A} U(64 A + m, kk) U(64 B + nn, kk)
// ONE product over the inner index kk = 64 A .. Np on k_loo_sweep's core (256
// threads, wave w owns the 32 x 32 quadrant (32 (w >> 1), 32 (w & 1)); chunks
// 16 deep, two-deep register ring, two LDS buffers, global-address-space loads,
// unconditional prefetches; the chunk count 4 (T - A) is a multiple of 4).
// Both operands are k-major pieces of columns of K (row stride Np): A row kk =
// K[64 A + m + Np kk], B row kk = K[64 B + nn + Np kk].  The first 64 kk are
// the exception: U_AA lives in wdt (stride 64), so the A operand comes from
// wdt_A, and the B operand too when B = A; for B < A it is block (B, A) of K.
// U(i, kk) = 0 for i < n <= kk (the pad of W is an identity), so the padding
// enters nothing.  The diagonal tiles also form alpha = U zt over kk < n: wave
// w takes rows 4 w .. 4 w + 3 of every chunk in order, and the four waves'
// sums are added in wave order.  The tile goes through LDS to K's lower block
// triangle (diagonal blocks whole: Q_AA comes out bitwise symmetric).
__global__ void __launch_bounds__(256) k_lgo_gram(const GCell* __restrict__ cs, const GItem* __restrict__ items) {
  __shared__ __attribute__((aligned(16))) double stg[4 * STAGE_A];  // 2 x (A, B) chunks; then the tile
  __shared__ double asum[256], zs[2 * KC];  // alpha partials; zt of the two staged chunks
  const GItem item = items[blockIdx.x];
  const GCell c = cs[item.cell];
  const int A = item.A, B = item.B, T = c.Np / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fk = lane >> 4;
  const size_t Np = (size_t)c.Np;
  const bool diag = A == B;  // uniform
  const gdbl* const zt = (const gdbl*)c.zt;
  const int nch = 4 * (T - A);
  const double* Ai = c.K + 64 * A;                    // A row kk >= 64 (A + 1): Ai[m + Np kk]
  const double* Bj = c.K + 64 * B;                    // B row kk: Bj[nn + Np kk]
  const double* wd = c.wdt + (size_t)A * 4096;        // rows kk - 64 A < 64 of U_AA: wd[m + 64 (kk - 64 A)]
  const int sk = t >> 5, sm = (t & 31) * 2;  // this thread's two 16 B pieces of a 16 x 64 chunk: rows sk, sk + 8
  double ap = 0.0;                           // diagonal tiles: this thread's share of alpha[64 A + lane]
  StageRegs r0, r1;
  double z0, z1;  // zt[kk] of row t & 15 of the chunk, staged with it (every tile: the loads stay unconditional)
  auto load = [&](int ch, StageRegs& q, double& zq) __attribute__((always_inline)) {
    const size_t kk = (size_t)64 * A + (size_t)KC * ch + sk;
    const bool first = ch < 4;  // uniform
    const double* ph = wd + sm + 64 * (size_t)(KC * ch + sk);
    const double* pa = first ? ph : Ai + sm + Np * kk;
    const size_t lda = first ? 64 : Np;
    const bool bw = first && diag;
    const double* pb = bw ? ph : Bj + sm + Np * kk;
    const size_t ldb = bw ? 64 : Np;
    q.a0 = gload2(pa);
    q.a1 = gload2(pa + lda * 8);
    q.b0 = gload2(pb);
    q.b1 = gload2(pb + ldb * 8);
    zq = zt[min(64 * A + KC * ch + (t & 15), c.n - 1)];
  };
  auto store = [&](int buf, const StageRegs& q, double zq) __attribute__((always_inline)) {
    double* As = stg + buf * 2 * STAGE_A;
    double* Bs = As + STAGE_A;
    *(dv2*)(As + sk * LDSA + sm) = q.a0;
    *(dv2*)(As + (sk + 8) * LDSA + sm) = q.a1;
    *(dv2*)(Bs + sk * LDSA + sm) = q.b0;
    *(dv2*)(Bs + (sk + 8) * LDSA + sm) = q.b1;
    if (t < KC) zs[buf * KC + t] = zq;
  };
  Quad acc;
  quad_zero(acc);
  auto compute = [&](int buf, int ch) __attribute__((always_inline)) {
    const double* As = stg + buf * 2 * STAGE_A;
    const double* Bs = As + STAGE_A;
#pragma unroll
    for (int kq = 0; kq < KC / 4; ++kq) {
      const int k = kq * 4 + fk;
      const double a0 = As[k * LDSA + 32 * wr + fr];
      const double a1 = As[k * LDSA + 32 * wr + 16 + fr];
      const double b0 = Bs[k * LDSA + 32 * wc + fr];
      const double b1 = Bs[k * LDSA + 32 * wc + 16 + fr];
      acc.c[0][0] = MFMA64(a0, b0, acc.c[0][0]);
      acc.c[0][1] = MFMA64(a0, b1, acc.c[0][1]);
      acc.c[1][0] = MFMA64(a1, b0, acc.c[1][0]);
      acc.c[1][1] = MFMA64(a1, b1, acc.c[1][1]);
    }
    if (diag) {
#pragma unroll
      for (int k = 4 * w; k < 4 * w + 4; ++k) {
        const int kk = 64 * A + KC * ch + k;
        if (kk < c.n) ap += As[k * LDSA + lane] * zs[buf * KC + k];
      }
    }
  };
  load(0, r0, z0);
  load(1, r1, z1);
  store(0, r0, z0);
  __syncthreads();
  for (int ch = 0; ch < nch; ch += 2) {
    load(min(ch + 2, nch - 1), r0, z0);
    compute(0, ch);
    store(1, r1, z1);
    __syncthreads();
    load(min(ch + 3, nch - 1), r1, z1);
    compute(1, ch + 1);
    if (ch + 2 < nch) store(0, r0, z0);
    __syncthreads();
  }
  // the tile, transposed, into LDS (the staging buffers are free behind the
  // loop's last barrier), then whole columns of K
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) stg[acc1_col(nb) * LOO_LD + acc1_row(mb, r)] = acc.c[mb][nb][r];
  asum[t] = ap;
  __syncthreads();
  gdbl* dst = (gdbl*)c.K + 64 * A + Np * 64 * (size_t)B;
  for (int e = t; e < 4096; e += 256) dst[(e & 63) + Np * (size_t)(e >> 6)] = stg[(e >> 6) * LOO_LD + (e & 63)];
  if (diag && t < 64) c.alpha[64 * A + t] = ((asum[t] + asum[64 + t]) + asum[128 + t]) + asum[192 + t];
}

// Group blockIdx.x, tile blockIdx.y = it (it + 1) / 2 + jt (it >= jt) of its
// padded block: P[i + gp j] = Q(c0 + i, c0 + j) for j <= i < g, an identity on
// the pad (entries with row >= column only, as k_pm_kgen), and the same tile(s)
// of X = [I_g ; alpha_G']; the diagonal tiles add the alpha row.
__global__ void __launch_bounds__(256) k_lgo_pack(const GGroup* __restrict__ gs) {
  const GGroup c = gs[blockIdx.x];
  const int y = blockIdx.y;
  int it = (int)((sqrt(8.0 * y + 1.0) - 1.0) / 2.0);
  while ((it + 1) * (it + 2) / 2 <= y) ++it;
  while (it * (it + 1) / 2 > y) --it;
  const int jt = y - it * (it + 1) / 2;
  if (it * 64 >= c.gp) return;
  const size_t Np = (size_t)c.Np, gp = (size_t)c.gp, ldx = (size_t)c.g + 1;
  const double* Q = c.K + c.c0 + Np * (size_t)c.c0;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int i = it * 64 + (e & 63), j = jt * 64 + (e >> 6);
    const bool in = i < c.g && j < c.g;
    if (i >= j) c.P[i + gp * j] = in ? Q[i + Np * j] : (i == j ? 1.0 : 0.0);
    if (in) {
      c.X[i + ldx * j] = i == j ? 1.0 : 0.0;
      if (it != jt) c.X[j + ldx * i] = 0.0;
    }
  }
  if (it == jt && threadIdx.x < 64) {
    const int i = it * 64 + threadIdx.x;
    if (i < c.g) c.X[c.g + ldx * i] = c.alpha[c.c0 + i];
  }
}

// One pass over a group's solved X, in k_pm_reduce's order (rows t = 64
// blockIdx.y + lane; wave w takes the columns i = w, w + 4, ...; the four wave
// partials are added in wave order): e_t = X_t . X_g, sd_t^2 = X_t . X_t.
// Every block of the group sums d2 = X_g . X_g and sum log C_kk itself (thread
// t takes i = t, t + 256, ...; lanes by shuffle, waves in order), so that each
// writes lpd_G and d2_G to its own rows; block 0 keeps lpd_G for lpl.
__global__ void __launch_bounds__(256) k_lgo_reduce(const GGroup* __restrict__ gs) {
  __shared__ double ra[4][64], rb[4][64], rz[4], rl[4];
  const GGroup c = gs[blockIdx.x];
  const int rows = c.g + 1, r0 = blockIdx.y * 64;
  if (r0 >= c.g) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = r0 + lane;
  const double* Xz = c.X + c.g;
  double a = 0.0, b = 0.0;
  if (t < c.g) {
    const double* Xt = c.X + t;
    for (int i = w; i < c.g; i += 4) {
      const size_t o = (size_t)rows * i;
      const double v = Xt[o], zt = Xz[o];
      a += v * zt;
      b += v * v;
    }
  }
  ra[w][lane] = a;
  rb[w][lane] = b;
  double zz = 0.0, ld = 0.0;
  for (int i = threadIdx.x; i < c.g; i += 256) {
    const double v = Xz[(size_t)rows * i];
    zz += v * v;
    ld += log(c.P[i + (size_t)c.gp * i]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    zz += __shfl_down(zz, o, 64);
    ld += __shfl_down(ld, o, 64);
  }
  if (lane == 0) {
    rz[w] = zz;
    rl[w] = ld;
  }
  __syncthreads();
  const bool bad = *c.cinfo != 0 || *c.ginfo != 0;
  const double d2 = ((rz[0] + rz[1]) + rz[2]) + rz[3];
  const double ldc = ((rl[0] + rl[1]) + rl[2]) + rl[3];
  const double lpd = ((-d2 / 2.0) + ldc) - ((double)c.g * LOG2PI) / 2.0;
  if (w == 0 && t < c.g) {
    a = ((ra[0][lane] + ra[1][lane]) + ra[2][lane]) + ra[3][lane];
    b = ((rb[0][lane] + rb[1][lane]) + rb[2][lane]) + rb[3][lane];
    const int o = c.perm[c.c0 + t];
    c.mu[o] = bad ? NAN : c.z[c.c0 + t] - a;
    c.sd[o] = bad ? NAN : sqrt(b);
    c.lpd[o] = bad ? NAN : lpd;
    c.d2[o] = bad ? NAN : d2;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) *c.glpd = bad ? NAN : lpd;
}

// lpl = the groups' lpd added in group order; status 1 cell, 2 some group
__global__ void __launch_bounds__(256) k_lgo_finish(const FCell* __restrict__ cs, int nc) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nc) return;
  const FCell c = cs[q];
  double s = 0.0;
  bool gbad = false;
  for (int k = 0; k < c.ng; ++k) {
    s += c.glpd[k];
    gbad = gbad || c.ginfo[k] != 0;
  }
  const bool bad = *c.info != 0;
  *c.lpl = bad || gbad ? NAN : s;
  *c.status = bad ? 1 : gbad ? 2 : 0;
}

// A cell's plan: perm[k] = the observation at sorted row k (groups contiguous,
// in the order of first appearance; members in observation order), the groups'
// first rows c0 and sizes g, and the tiles (A, B), A >= B, of Q that some group
// touches -- every (A, B) with bA <= B <= A <= bE for a group spanning block
// columns bA .. bE -- each once, in lexicographic order.  An off-diagonal tile
// belongs to one group alone (the next group starts at or behind block bE), a
// diagonal one may be shared: `done` is the last diagonal block listed.
struct LgoPlan {
  std::vector<int32_t> perm, c0, g, tiles;  // tiles: A, B pairs
};
LgoPlan lgo_plan(const int64_t* group, int64_t n) {
  LgoPlan p;
  std::unordered_map<int64_t, int32_t> id;
  std::vector<int32_t> gid((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const auto [it, fresh] = id.try_emplace(group[i], (int32_t)p.g.size());
    if (fresh) p.g.push_back(0);
    gid[i] = it->second;
    ++p.g[gid[i]];
  }
  p.c0.resize(p.g.size());
  int32_t at = 0;
  for (size_t q = 0; q < p.g.size(); ++q) {
    p.c0[q] = at;
    at += p.g[q];
  }
  std::vector<int32_t> next(p.c0);
  p.perm.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) p.perm[next[gid[i]]++] = (int32_t)i;
  int32_t done = -1;
  for (size_t q = 0; q < p.g.size(); ++q) {
    const int32_t bA = p.c0[q] / 64, bE = (p.c0[q] + p.g[q] - 1) / 64;
    for (int32_t A = bA; A <= bE; ++A)
      for (int32_t B = bA; B <= A; ++B) {
        if (A == B && A <= done) continue;
        p.tiles.push_back(A);
        p.tiles.push_back(B);
      }
    done = std::max(done, bE);
  }
  return p;
}

// The workspace on top of leave-one-out's (dense_chunk, dense_cell with loo):
// chunk-wide, the gathered inputs 4 nn (device inputs only: host inputs are
// sorted on the host before they are staged), lpd and d2 per row, lpd_G and the
// group Cholesky's info per group (zeroed); per cell alpha Np; per group the
// padded block gp^2, its diagonal-block inverses 64 gp and X (g + 1) g.
struct LgoChunk {
  double *gx, *gz, *lpd, *d2, *glpd;
  int32_t* ginfo;
};
LgoChunk lgo_chunk(Carver& cv, bool gather, int64_t nn, int64_t ng, hipStream_t st) {
  LgoChunk k{};
  if (gather) {
    k.gx = cv.take(nn * 3);
    k.gz = cv.take(nn);
  }
  k.lpd = cv.take(nn);
  k.d2 = cv.take(nn);
  k.glpd = cv.take(ng);
  k.ginfo = reinterpret_cast<int32_t*>(cv.take(ng));
  if (k.ginfo && ng > 0) HC(hipMemsetAsync(k.ginfo, 0, ng * 8, st));
  return k;
}
struct LgoGroup {
  double *P, *dinv, *X;
};
LgoGroup lgo_group(Carver& cv, int64_t g) {
  const int64_t gp = up(g, 64);
  LgoGroup a;
  a.P = cv.take(gp * gp);
  a.dinv = cv.take(64 * gp);
  a.X = cv.take((g + 1) * g);
  return a;
}
int64_t lgo_cell_doubles(int64_t n, const int32_t* gs, int64_t ng, bool host_inputs) {
  Carver own, share{nullptr, 0, 1};
  dense_cell(own, n, 0, true);
  own.take(up(n, 64));
  for (int64_t q = 0; q < ng; ++q) lgo_group(own, gs[q]);
  dense_chunk(share, DenseIn{nullptr, nullptr, host_inputs, nullptr}, 0, n, nullptr, 0, n, 1, -1);
  lgo_chunk(share, !host_inputs, n, ng, nullptr);
  return own.off + share.off;
}

constexpr int64_t LGO_SLACK = 16 * 32;  // rounding of the chunk-wide arrays (doubles)

enum { G_GEN, G_CHOL, G_SOLVE, G_SWEEP, G_GRAM, G_GROUPS, G_COUNT };
const char* kLgoStage[G_COUNT] = {"lgo_generate", "lgo_cholesky", "lgo_solve", "lgo_sweep", "lgo_gram", "lgo_groups"};

}  // namespace

extern "C" int oi_gpr_lgo(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                          const int64_t* group, double mean, const double* hyp, double* mu, double* sd,
                          double* lpd, double* d2, double* lpl, int32_t* status, const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (ncell == 0) return 0;
  const int64_t N = offs[ncell];
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (!hyp) return oi_set_last_error(OI_E_ARG, "null hyp");
  if (N > 0 && (!xyt || !z)) return oi_set_last_error(OI_E_ARG, "null xyt / z");
  if (N > 0 && !group) return oi_set_last_error(OI_E_ARG, "null group");
  if (N > 0 && (!mu || !sd)) return oi_set_last_error(OI_E_ARG, "null mu / sd");
  constexpr int64_t LIM = 0x7FFFFFF0 / 8;  // oila's operands take 32-bit byte offsets
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t Np = up(offs[c + 1] - offs[c], 64);
    if (Np * Np >= LIM) return oi_set_last_error(OI_E_ARG, "cell too large (K reaches 2 GiB)");
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    const bool host = o.device_inputs == 0;
    std::vector<LgoPlan> plans((size_t)ncell);
    for (int64_t c = 0; c < ncell; ++c) plans[c] = lgo_plan(group + offs[c], offs[c + 1] - offs[c]);
    // host inputs: sorted here, so that the front half stages them as they are
    std::vector<double> sx, sz;
    if (host) {
      sx.resize((size_t)N * 3);
      sz.resize((size_t)N);
      for (int64_t c = 0; c < ncell; ++c)
        for (int64_t k = 0, n = offs[c + 1] - offs[c]; k < n; ++k) {
          const int64_t s = offs[c] + plans[c].perm[k], d = offs[c] + k;
          for (int e = 0; e < 3; ++e) sx[d * 3 + e] = xyt[s * 3 + e];
          sz[d] = z[s];
        }
    }
    Front fr(o, host ? sx.data() : nullptr, host ? sz.data() : nullptr, offs, hyp, mean, true, kLgoStage, G_COUNT);
    const auto [cuts, biggest] = plan_chunks(ncell, o, LGO_SLACK, CHUNK_CELLS, "leave-group-out", [&](int64_t c) {
      return lgo_cell_doubles(offs[c + 1] - offs[c], plans[c].g.data(), (int64_t)plans[c].g.size(), host);
    });
    DevBuf ws((size_t)biggest * 8);
    hipStream_t st = fr.st;
    std::vector<LCell> lcells;
    std::vector<LItem> items;
    std::vector<GCell> gcells;
    std::vector<GItem> gitems;
    std::vector<GGroup> groups;
    std::vector<FCell> fcells;
    std::vector<oila::Chol> gchol;
    std::vector<oila::TrsmRLT> gtrsm;
    std::vector<int32_t> perm;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, n0 = offs[c0], nn = offs[c1] - n0;
      int64_t ng = 0;
      for (int64_t c = c0; c < c1; ++c) ng += (int64_t)plans[c].g.size();
      Carver cv{static_cast<double*>(ws.p)};
      fr.begin(cv, c0, c1, nullptr, 0, -1);
      const DenseChunk& k = fr.k;
      const LgoChunk lk = lgo_chunk(cv, !host, nn, ng, st);
      // sorted row of the chunk -> row of the chunk in the caller's order
      perm.resize((size_t)nn);
      for (int64_t c = c0; c < c1; ++c)
        for (int64_t i = 0, n = offs[c + 1] - offs[c], r0 = offs[c] - n0; i < n; ++i)
          perm[r0 + i] = (int32_t)(r0 + plans[c].perm[i]);
      const int32_t* dperm = nn > 0 ? fr.la.put(perm) : nullptr;
      lcells.clear();
      items.clear();
      gcells.clear();
      gitems.clear();
      groups.clear();
      fcells.clear();
      gchol.clear();
      gtrsm.clear();
      int64_t g0 = 0, gmax = 0;
      double fl_gram = 0.0, fl_groups = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const LgoPlan& pl = plans[c];
        const int64_t r0 = offs[c] - n0, cq = c - c0;
        DenseCell a;
        PCell& p = fr.add(cv, c, 0, a);
        if (!host) {
          p.x = lk.gx + r0 * 3;
          p.z = lk.gz + r0;
        }
        double* alpha = cv.take(p.Np);
        lcells.push_back(LCell{p.K, a.dinv, a.wdt, p.X, p.z, k.mu + r0, k.sd + r0, a.part, k.lz + cq, p.info, p.status,
                               p.n, p.Np});
        for (int j = 0; j < p.Np / 64; ++j) items.push_back(LItem{(int)cq, j});
        gcells.push_back(GCell{p.K, a.wdt, p.X, alpha, p.n, p.Np});
        for (size_t e = 0; e < pl.tiles.size(); e += 2) {
          gitems.push_back(GItem{(int)cq, pl.tiles[e], pl.tiles[e + 1]});
          fl_gram += 2.0 * 64.0 * 64.0 * 64.0 * (double)(p.Np / 64 - pl.tiles[e]);
        }
        for (size_t e = 0; e < pl.g.size(); ++e) {
          const int g = pl.g[e], gp = (int)up(g, 64);
          const LgoGroup b = lgo_group(cv, g);
          int32_t* gi = lk.ginfo + g0 + (int64_t)e;
          groups.push_back(GGroup{p.K, alpha, p.z, b.P, b.X, k.mu, k.sd, lk.lpd, lk.d2, dperm + r0,
                                  lk.glpd + g0 + (int64_t)e, gi, p.info, pl.c0[e], g, gp, p.Np});
          gchol.push_back(oila::Chol{b.P, b.dinv, gi, gp, gp});
          gtrsm.push_back(oila::TrsmRLT{b.X, b.P, b.dinv, g + 1, g, g + 1, gp});
          gmax = std::max<int64_t>(gmax, g);
          const double dg = (double)g;
          fl_groups += dg * dg * dg / 3.0 + (dg + 1.0) * dg * dg;
        }
        fcells.push_back(FCell{lk.glpd + g0, lk.ginfo + g0, k.lz + cq, p.info, p.status, (int)pl.g.size()});
        g0 += (int64_t)pl.g.size();
      }
      if (cv.off > biggest) throw HipErr{"oi_gpr_lgo: workspace layout exceeds its estimate"};
      if (!host && nn > 0) {
        hipLaunchKernelGGL(k_lgo_gather, dim3(blocks(nn, 256)), dim3(256), 0, st, xyt + n0 * 3, z + n0, dperm, lk.gx,
                           lk.gz, nn);
        KCHK();
      }
      // the longest block columns / inner dimensions first; ties keep the cells' order
      std::stable_sort(items.begin(), items.end(), [&](const LItem& a, const LItem& b) {
        return lcells[a.cell].Np / 64 - a.j > lcells[b.cell].Np / 64 - b.j;
      });
      std::stable_sort(gitems.begin(), gitems.end(), [&](const GItem& a, const GItem& b) {
        return gcells[a.cell].Np / 64 - a.A > gcells[b.cell].Np / 64 - b.A;
      });
      const LCell* dl = fr.la.put(lcells);
      fr.factor(G_GEN, G_CHOL, G_SOLVE);
      fr.sg.begin(G_SWEEP, fr.fl_chol, 0.0);
      if (!items.empty()) {
        const LItem* di = fr.la.put(items);
        hipLaunchKernelGGL(k_loo_sweep, dim3((unsigned)items.size()), dim3(256), 0, st, dl, di);
        KCHK();
      }
      fr.sg.end();
      fr.sg.begin(G_GRAM, fl_gram, 0.0);
      if (!gitems.empty()) {
        const GCell* dg = fr.la.put(gcells);
        const GItem* di = fr.la.put(gitems);
        hipLaunchKernelGGL(k_lgo_gram, dim3((unsigned)gitems.size()), dim3(256), 0, st, dg, di);
        KCHK();
      }
      fr.sg.end();
      fr.sg.begin(G_GROUPS, fl_groups, 0.0);
      if (!groups.empty()) {
        const GGroup* dg = fr.la.put(groups);
        const unsigned Tg = blocks(gmax, 64);
        hipLaunchKernelGGL(k_lgo_pack, dim3((unsigned)groups.size(), Tg * (Tg + 1) / 2), dim3(256), 0, st, dg);
        KCHK();
        oila::cholesky(fr.la, st, gchol);
        oila::trsm_right_lt(fr.la, st, gtrsm);
        hipLaunchKernelGGL(k_lgo_reduce, dim3((unsigned)groups.size(), Tg), dim3(256), 0, st, dg);
        KCHK();
      }
      const FCell* df = fr.la.put(fcells);
      hipLaunchKernelGGL(k_lgo_finish, dim3(blocks(nc, 256)), dim3(256), 0, st, df, (int)nc);
      KCHK();
      fr.sg.end();
      if (nn > 0) {
        HC(hipMemcpyAsync(mu + n0, k.mu, nn * 8, hipMemcpyDeviceToHost, st));
        HC(hipMemcpyAsync(sd + n0, k.sd, nn * 8, hipMemcpyDeviceToHost, st));
        if (lpd) HC(hipMemcpyAsync(lpd + n0, lk.lpd, nn * 8, hipMemcpyDeviceToHost, st));
        if (d2) HC(hipMemcpyAsync(d2 + n0, lk.d2, nn * 8, hipMemcpyDeviceToHost, st));
      }
      if (lpl) HC(hipMemcpyAsync(lpl + c0, k.lz, nc * 8, hipMemcpyDeviceToHost, st));
      fr.finish(status);
    }
    return 0;
  });
}

// Test hooks (not in the headers; neither touches a device).  The workspace
// the chunk planner counts for one cell of oi_gpr_lgo with the given group
// sizes (flags 2: host inputs); -1 when the sizes do not add up to n.
extern "C" int64_t oi_test_lgo_cell_doubles(int64_t n, const int64_t* gsizes, int64_t ngroups, int32_t flags) {
  std::vector<int32_t> gs;
  int64_t sum = 0;
  for (int64_t q = 0; q < ngroups; ++q) {
    if (gsizes[q] < 1) return -1;
    gs.push_back((int32_t)gsizes[q]);
    sum += gsizes[q];
  }
  if (sum != n) return -1;
  return lgo_cell_doubles(n, gs.data(), ngroups, (flags & 2) != 0);
}
// A cell's plan from its labels: perm [n], the groups' first rows and sizes
// (room for n each) and their number, and up to `cap` tiles as (A, B) pairs in
// dispatch order within the cell; returns the number of tiles.
extern "C" int64_t oi_test_lgo_plan(const int64_t* group, int64_t n, int64_t* perm, int64_t* gstart, int64_t* gsize,
                                    int64_t* ngroups, int64_t* tiles, int64_t cap) {
  const LgoPlan p = lgo_plan(group, n);
  for (int64_t i = 0; i < n; ++i) perm[i] = p.perm[i];
  for (size_t q = 0; q < p.g.size(); ++q) {
    gstart[q] = p.c0[q];
    gsize[q] = p.g[q];
  }
  *ngroups = (int64_t)p.g.size();
  const int64_t nt = (int64_t)p.tiles.size() / 2;
  for (int64_t e = 0; e < std::min(nt, cap); ++e) {
    tiles[2 * e] = p.tiles[2 * e];
    tiles[2 * e + 1] = p.tiles[2 * e + 1];
  }
  return nt;
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

// ===========================================================================
// Joint posterior draws per cell (include/oi_sample.h) at given hypers.  With
// fs and cov = Kxs - v'v exactly as oi_gpr_predict_multi forms them:
//
//   C = cov + (noise ? sn2 : 0) I + jitter I = Lc Lc'
//   samples[t, s] = fs[t] + sum_u Lc[t, u] Xi[u, s]
//
// The front half and k_pm_reduce run unchanged (fs and sd are bit for bit
// oi_gpr_predict_multi's).  k_ps_cgen writes the lower tiles of Kxs plus the
// diagonal term into a padded Ntp x Ntp buffer, Ntp = nt rounded up to 64,
// with an identity on the pad and zeros in the strict upper triangle of the
// diagonal tiles; oila::gemm (tri = 3) subtracts X[:nt] X[:nt]' and
// oila::cholesky factors in place, neither touching those zeros.  k_ps_draw
// fills the result with fs and, without the caller's Xi, writes the normals
// (Philox4x32-10, Box-Muller; ps_normal).  The cell's block of samples, row-major
// [nt x nsamp], is the column-major nsamp x nt matrix Xi' Lc', one oila::gemm
// with tri = 2 (Lc' is upper triangular) and beta = 1 on top of fs.
// ===========================================================================
namespace {

struct SCell {
  const double* xsc;     // nt x 3 scaled targets
  double* C;             // Ntp x Ntp: C, then its Cholesky factor (lower)
  const double* fs;      // nt
  double* xi;            // [nt x nsamp] row-major
  double* out;           // [nt x nsamp] row-major
  const int32_t* info;   // the cell's Cholesky
  const int32_t* cinfo;  // C's Cholesky
  int32_t* status;       // 1
  uint64_t stream;       // the generator's stream id
  int nt, Ntp, nsamp;
  double sf2, add;       // add = (noise ? sn2 : 0) + jitter
};

// Philox4x32-10 (Salmon et al., SC'11): key = (seed lo, seed hi), counter =
// (block lo, block hi, stream lo, stream hi)
__device__ inline void philox4x32_10(uint64_t seed, uint64_t stream, uint64_t block, uint32_t (&w)[4]) {
  uint32_t c0 = (uint32_t)block, c1 = (uint32_t)(block >> 32), c2 = (uint32_t)stream, c3 = (uint32_t)(stream >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = (h1 ^ c1) ^ k0, n2 = (h0 ^ c3) ^ k1;
    c0 = n0;
    c1 = l1;
    c2 = n2;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

// Element e of a stream's standard normals: block e >> 1, Box-Muller on the
// block's two 53-bit uniforms; the even element is the cosine branch
__device__ inline double ps_normal(uint64_t seed, uint64_t stream, uint64_t e) {
  uint32_t w[4];
  philox4x32_10(seed, stream, e >> 1, w);
  const uint64_t k1 = ((uint64_t)w[0] << 21) | (uint64_t)(w[1] >> 11);
  const uint64_t k2 = ((uint64_t)w[2] << 21) | (uint64_t)(w[3] >> 11);
  const double u1 = (double)(k1 + 1) * 0x1p-53, u2 = (double)k2 * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  const double th = 6.283185307179586 * u2;  // 2 * np.pi
  double sn, cs;
  sincos(th, &sn, &cs);
  return r * ((e & 1) ? sn : cs);
}

// 64 x 64 tile (it, jt), it >= jt, of the padded C: Kxs (k_pm_kxs's
// expression; its diagonal is sf2 exactly) plus `add` on the diagonal for rows
// and columns < nt, the identity on the pad, and zeros above the diagonal of
// the diagonal tiles (the product with Lc' reads them).
__global__ void __launch_bounds__(256) k_ps_cgen(const SCell* __restrict__ cs) {
  __shared__ double si[3][64], sj[3][64];
  const SCell c = cs[blockIdx.z];
  const int it = blockIdx.x, jt = blockIdx.y;
  if (it < jt || it * 64 >= c.Ntp) return;
  stage_tile(c.xsc, c.nt, it, jt, si, sj);
  const int m = threadIdx.x & 63, i = it * 64 + m;
  for (int q = 0; q < 16; ++q) {
    const int nn = (threadIdx.x >> 6) * 16 + q, j = jt * 64 + nn;
    double v;
    if (i < j) {
      v = 0.0;
    } else if (i < c.nt) {  // j <= i < nt
      v = matern32(c.sf2, si[0][m] - sj[0][nn], si[1][m] - sj[1][nn], si[2][m] - sj[2][nn]);
      if (i == j) v = v + c.add;
    } else {
      v = i == j ? 1.0 : 0.0;
    }
    c.C[i + (size_t)c.Ntp * j] = v;
  }
}

// out[t, s] = fs[t]; with rng, Xi[t, s] = element s nt + t of the cell's stream
__global__ void __launch_bounds__(256) k_ps_draw(const SCell* __restrict__ cs, uint64_t seed, int rng) {
  const SCell c = cs[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)c.nt * c.nsamp) return;
  const int t = (int)(e / c.nsamp), s = (int)(e % c.nsamp);
  c.out[e] = c.fs[t];
  if (rng) c.xi[e] = ps_normal(seed, c.stream, (uint64_t)s * (uint64_t)c.nt + (uint64_t)t);
}

// status 2 where C did not factor; NaN samples for a failed cell (either status)
__global__ void __launch_bounds__(256) k_ps_finish(const SCell* __restrict__ cs) {
  const SCell c = cs[blockIdx.y];
  const bool bad = *c.info != 0, cbad = *c.cinfo != 0;
  if (!bad && !cbad) return;
  if (blockIdx.x == 0 && threadIdx.x == 0 && !bad) *c.status = 2;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (int64_t)c.nt * c.nsamp) c.out[e] = NAN;
}

// the test hook's kernel: normals of elements first .. first + count - 1 and
// the words of the blocks they touch
__global__ void __launch_bounds__(256) k_ps_hook(uint64_t seed, uint64_t stream, uint64_t first, int64_t count,
                                                 double* __restrict__ out, uint32_t* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  out[i] = ps_normal(seed, stream, first + (uint64_t)i);
  const uint64_t b0 = first >> 1, nb = ((first + (uint64_t)count - 1) >> 1) - b0 + 1;
  if (words && (uint64_t)i < nb) {
    uint32_t w[4];
    philox4x32_10(seed, stream, b0 + (uint64_t)i, w);
    for (int q = 0; q < 4; ++q) words[4 * i + q] = w[q];
  }
}

enum { P_GEN, P_CHOL, P_SOLVE, P_REDUCE, P_COV, P_FACTOR, P_NORMALS, P_PRODUCT, P_COUNT };
const char* kSampleStage[P_COUNT] = {"ps_generate", "ps_cholesky", "ps_solve",   "ps_reduce",
                                     "ps_cov",      "ps_factor",   "ps_normals", "ps_product"};

constexpr int64_t SAMPLE_SLACK = CHUNK_SLACK + 3 * 32;  // three more chunk-wide arrays

// What the draw adds to oi_gpr_predict_multi's layout.  Chunk-wide, the cells'
// parts back to back in the ABI's own layout: Xi and the samples, ee = sum of
// nt nsamp doubles each, and the second factorisation's info [nc], zeroed.
struct SampleChunk {
  double *xi, *out;
  int32_t* cinfo;
};
SampleChunk sample_chunk(Carver& cv, int64_t ee, int64_t nc, hipStream_t st) {
  SampleChunk k;
  k.xi = cv.take(ee);
  k.out = cv.take(ee);
  k.cinfo = reinterpret_cast<int32_t*>(cv.take((nc + 1) / 2));
  if (k.cinfo) HC(hipMemsetAsync(k.cinfo, 0, nc * 4, st));
  return k;
}
// One cell's own: the padded C, Ntp^2, and its factor's diagonal-block inverses, 64 Ntp
struct SampleCell {
  double *C, *dinv;
};
SampleCell sample_cell(Carver& cv, int64_t nt) {
  const int64_t Ntp = up(nt, 64);
  SampleCell a;
  a.C = cv.take(Ntp * Ntp);
  a.dinv = cv.take(Ntp * 64);
  return a;
}
int64_t sample_cell_doubles(int64_t n, int64_t nt, int64_t nsamp, bool host_inputs) {
  Carver own, share{nullptr, 0, 1};
  dense_cell(own, n, nt, false);
  sample_cell(own, nt);
  dense_chunk(share, DenseIn{nullptr, nullptr, host_inputs, nullptr}, 0, n, nullptr, nt, nt, 1, -1);
  sample_chunk(share, nt * nsamp, 1, nullptr);
  return own.off + share.off;
}

}  // namespace

extern "C" int oi_gpr_sample(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                             const double* xs, const int64_t* toffs, double mean, const double* hyp,
                             int64_t nsamp, int32_t noise, double jitter, uint64_t seed,
                             const uint64_t* streams, const double* xi, double* samples, double* fs,
                             double* sd, int32_t* status, const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (int rc = oi_check_offs(toffs, ncell, 0, "toffs")) return rc;
  if (nsamp < 0) return oi_set_last_error(OI_E_ARG, "negative nsamp");
  if (noise != 0 && noise != 1) return oi_set_last_error(OI_E_ARG, "noise must be 0 or 1");
  if (!(jitter >= 0.0) || !std::isfinite(jitter))
    return oi_set_last_error(OI_E_ARG, "jitter must be finite and >= 0");
  if (ncell == 0) return 0;
  const int64_t N = offs[ncell], T = toffs[ncell];
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (!hyp) return oi_set_last_error(OI_E_ARG, "null hyp");
  if (N > 0 && (!xyt || !z)) return oi_set_last_error(OI_E_ARG, "null xyt / z");
  if (T > 0 && !xs) return oi_set_last_error(OI_E_ARG, "null xs");
  if (T > 0 && nsamp > 0 && !samples) return oi_set_last_error(OI_E_ARG, "null samples");
  // oila's operands take 32-bit byte offsets: K, X, C, Xi and the samples stay below 2 GiB each
  constexpr int64_t LIM = 0x7FFFFFF0 / 8;
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t n = offs[c + 1] - offs[c], nt = toffs[c + 1] - toffs[c], Np = up(n, 64), Ntp = up(nt, 64);
    if (Np * Np >= LIM || (nt + 1) * n >= LIM || Ntp * Ntp >= LIM || (nsamp > 0 && nt >= LIM / nsamp))
      return oi_set_last_error(OI_E_ARG, "cell too large (K, X, C or nt * nsamp reaches 2 GiB)");
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    Front fr(o, xyt, z, offs, hyp, mean, false, kSampleStage, P_COUNT);
    const auto [cuts, biggest] = plan_chunks(ncell, o, SAMPLE_SLACK, CHUNK_CELLS, "sampling", [&](int64_t c) {
      return sample_cell_doubles(offs[c + 1] - offs[c], toffs[c + 1] - toffs[c], nsamp, fr.in.host);
    });
    DevBuf ws((size_t)biggest * 8);
    hipStream_t st = fr.st;
    std::vector<SCell> scells;
    std::vector<oila::Gemm> syrk, prod;
    std::vector<oila::Chol> cchol;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, t0 = toffs[c0], tt = toffs[c1] - t0;
      const int64_t ee = tt * nsamp;
      Carver cv{static_cast<double*>(ws.p)};
      fr.begin(cv, c0, c1, xs + t0 * 3, tt, -1);
      const DenseChunk& k = fr.k;
      const SampleChunk sk = sample_chunk(cv, ee, nc, st);
      if (xi && ee > 0) HC(hipMemcpyAsync(sk.xi, xi + t0 * nsamp, ee * 8, hipMemcpyHostToDevice, st));
      scells.clear();
      syrk.clear();
      prod.clear();
      cchol.clear();
      int64_t emax = 0;
      double fl_cov = 0.0, fl_fac = 0.0, fl_prod = 0.0, by_red = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const int64_t nt = toffs[c + 1] - toffs[c], tq = toffs[c] - t0, cq = c - c0;
        DenseCell a;
        PCell& p = fr.add(cv, c, nt, a);
        p.xs = k.xs + tq * 3;
        p.xsc = a.xsc;
        p.cov = nullptr;
        p.fs = k.mu + tq;
        p.sd = k.sd + tq;
        p.lz = k.lz + cq;
        const SampleCell b = sample_cell(cv, nt);
        const int Ntp = (int)up(nt, 64);
        int32_t* ci = sk.cinfo + cq;
        scells.push_back(SCell{a.xsc, b.C, p.fs, sk.xi + tq * nsamp, sk.out + tq * nsamp, p.info, ci, p.status,
                               streams ? streams[c] : (uint64_t)c, p.nt, Ntp, (int)nsamp, p.sf2,
                               (noise ? p.sn2 : 0.0) + jitter});
        const SCell& s = scells.back();
        if (nt > 0) {
          if (p.n > 0)  // C -= X[:nt] X[:nt]' on and below the diagonal
            syrk.push_back(oila::Gemm{p.X, p.X, s.C, p.nt, p.nt, p.n, p.nt + 1, p.nt + 1, Ntp, -1.0, 1.0, 3});
          cchol.push_back(oila::Chol{s.C, b.dinv, ci, Ntp, Ntp});
          if (nsamp > 0)  // out (nsamp x nt, column-major) += Xi' Lc'
            prod.push_back(oila::Gemm{s.xi, s.C, s.out, s.nsamp, s.nt, s.nt, s.nsamp, Ntp, s.nsamp, 1.0, 1.0, 2});
        }
        emax = std::max(emax, nt * nsamp);
        const double dn = (double)p.n, dt = (double)nt, ds = (double)nsamp;
        fl_cov += dt * dt * dn;
        fl_fac += dt * dt * dt / 3.0;
        fl_prod += ds * dt * dt;
        by_red += 8.0 * (dt + 1.0) * dn;
      }
      if (cv.off > biggest) throw HipErr{"oi_gpr_sample: workspace layout exceeds its estimate"};
      const PCell* dc = fr.factor(P_GEN, P_CHOL, P_SOLVE);
      const SCell* ds = fr.la.put(scells);
      const unsigned gz = (unsigned)nc, Tt = blocks(fr.ntmax, 64), ge = std::max(1u, blocks(emax, 256));
      fr.sg.begin(P_REDUCE, by_red / 2.0, by_red);
      hipLaunchKernelGGL(k_pm_reduce, dim3(blocks(fr.ntmax + 1, 64), gz), dim3(256), 0, st, dc);
      KCHK();
      fr.sg.end();
      fr.sg.begin(P_COV, fl_cov, 0.0);
      if (fr.ntmax > 0) {
        hipLaunchKernelGGL(k_ps_cgen, dim3(Tt, Tt, gz), dim3(256), 0, st, ds);
        KCHK();
        oila::gemm(fr.la, st, false, true, syrk);
      }
      fr.sg.end();
      fr.sg.begin(P_FACTOR, fl_fac, 0.0);
      oila::cholesky(fr.la, st, cchol);
      fr.sg.end();
      fr.sg.begin(P_NORMALS, 0.0, 16.0 * (double)ee);
      if (emax > 0) {
        hipLaunchKernelGGL(k_ps_draw, dim3(ge, gz), dim3(256), 0, st, ds, seed, xi ? 0 : 1);
        KCHK();
      }
      fr.sg.end();
      fr.sg.begin(P_PRODUCT, fl_prod, 0.0);
      oila::gemm(fr.la, st, false, true, prod);
      hipLaunchKernelGGL(k_ps_finish, dim3(ge, gz), dim3(256), 0, st, ds);
      KCHK();
      fr.sg.end();
      if (tt > 0) {
        if (fs) HC(hipMemcpyAsync(fs + t0, k.mu, tt * 8, hipMemcpyDeviceToHost, st));
        if (sd) HC(hipMemcpyAsync(sd + t0, k.sd, tt * 8, hipMemcpyDeviceToHost, st));
      }
      if (ee > 0) HC(hipMemcpyAsync(samples + t0 * nsamp, sk.out, ee * 8, hipMemcpyDeviceToHost, st));
      fr.finish(status);
    }
    return 0;
  });
}

// Test hooks (in no header).  The workspace the chunk planner counts for one
// cell of oi_gpr_sample (flags 2: host inputs); touches no device.
extern "C" int64_t oi_test_sample_cell_doubles(int64_t n, int64_t nt, int64_t nsamp, int32_t flags) {
  return sample_cell_doubles(n, nt, nsamp, (flags & 2) != 0);
}
// The product's own device function for elements first .. first + count - 1 of
// (seed, stream): their normals into out [count] and, when words is not null,
// the raw Philox words of every block touched (4 each, blocks first >> 1 ..
// (first + count - 1) >> 1).  Host arrays; 0 or an OI_E_* code.
extern "C" int oi_test_sample_normals(uint64_t seed, uint64_t stream, uint64_t first, int64_t count, double* out,
                                      uint32_t* words) {
  if (count < 0 || (count > 0 && !out)) return oi_set_last_error(OI_E_ARG, "bad count / null out");
  if (count == 0) return 0;
  const oi_options o = oi_resolve(nullptr);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    const int64_t nb = (int64_t)(((first + (uint64_t)count - 1) >> 1) - (first >> 1)) + 1;
    DevBuf dout((size_t)count * 8), dw(words ? (size_t)nb * 16 : 0);
    hipLaunchKernelGGL(k_ps_hook, dim3(blocks(count, 256)), dim3(256), 0, nullptr, seed, stream, first, count,
                       dout.as<double>(), dw.as<uint32_t>());
    KCHK();
    HC(hipMemcpy(out, dout.p, (size_t)count * 8, hipMemcpyDeviceToHost));
    if (words) HC(hipMemcpy(words, dw.p, (size_t)nb * 16, hipMemcpyDeviceToHost));
    return 0;
  });
}
