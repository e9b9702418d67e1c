// A trained SVGP model put to use: GPflow's SVGP.predict_f / predict_y at any
// number of targets per cell, and model.elbo((X, Y)) on all of a cell's data,
// from the `params` rows that oi_svgp_batch writes (oi_svgp.hip; restated
// algorithm: oracle/svgp_oracle.py predict_f and loss_and_grad(grad=False)).
// Nothing here trains.  Per cell, with the constrained hypers of the row:
//
//   L = chol(K_uu + 1e-6 I);  a_t = L^-1 k_u(x_t);  sa_t = S' a_t
//   mean_t = c + a_t . q_mu;  var_t = (kvar - a_t . a_t) + sa_t . sa_t  [+ s2]
//   cov_tu = (k(x_t, x_u) - a_t . a_u) + sa_t . sa_u
//   elbo   = sum_i [-log(2 pi)/2 - log(s2)/2 - ((y_i - mean_i)^2 + var_i)/(2 s2)]
//            - (q.q + |S|^2 - M - sum log S_ii^2) / 2
//
// Three kernels per chunk of cells (as many as the workspace budget holds):
//
//   k_sp_model    one workgroup per cell: hypers, scaled Z, K_uu + jitter and
//                 its Cholesky in LDS (chol_lds, as the training kernel), the
//                 KL term and the status -> a per-cell record in global memory
//   k_sp_targets  grid (tile of 128 targets, cell), lane = target: tril(L) and
//                 tril(S), both packed, staged in LDS once per block, k_u by m32, the
//                 forward substitution with the lane's a column in an LDS panel
//                 (a[m][lane]: lane-contiguous, L[i][k] an LDS broadcast), then
//                 S'a, mean and variance.  The ELBO call runs it over the
//                 observations: each block writes one partial of sum v_i and
//                 k_sp_reduce adds a cell's partials in index order.
//   k_sp_cov      (cov only) grid (64 x 64 output tile, cell): every entry from
//                 the A and S'A panels that k_sp_targets stored, each dot
//                 product summed over m ascending exactly as var_t is -- so the
//                 diagonal is var bit for bit, cov is symmetric bit for bit, and
//                 two equal targets give two equal rows.
//
// Every sum has a fixed order that depends on the cell and the target alone:
// batch mates, chunking, the tile a target lands in and host / device inputs
// do not change a result.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "oi_host.h"
#include "oi_svgp_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int TL = 128;  // targets per block of k_sp_targets (two waves)
constexpr int CT = 64;   // covariance tile
constexpr size_t LDS_MAX = 160 * 1024;

// per-cell record (doubles): ls[3], kvar, s2, c, KL, bad; Zs[M x 3] (scaled),
// q_mu[M], tril(L) and tril(S) packed row-major (tri_index)
enum { R_LS = 0, R_KVAR = 3, R_S2 = 4, R_C = 5, R_KL = 6, R_BAD = 7, R_ZS = 8 };
__host__ __device__ inline int rec_doubles(int M) { return R_ZS + 4 * M + M * (M + 1); }

inline size_t model_lds(int M) { return (size_t)(2 * M * M + 3 * M + 4) * 8 + 16; }
inline size_t targets_lds(int M) {
  return (size_t)(M * (M + 1) + 4 * M + M * TL + 2) * 8;
}
inline size_t cov_lds(int M) { return (size_t)(2 * M * CT + 3 * CT) * 8; }

// One workgroup per cell of the chunk: the model's record.  bad = a pivot of the
// Cholesky that is not positive, or any non-finite parameter in the row.
__global__ void __launch_bounds__(256) k_sp_model(const double* __restrict__ params, int M, int P,
                                                  double* __restrict__ rec,
                                                  int32_t* __restrict__ status) {
  extern __shared__ double lds[];
  double* W = lds;
  double* L = W + M * M;
  double* Zs = L + M * M;
  double* red = Zs + 3 * M;
  int* flag = (int*)(red + 4);
  int* nonfin = flag + 1;
  const int tid = threadIdx.x;
  const double* th = params + (size_t)blockIdx.x * P;
  double* r = rec + (size_t)blockIdx.x * rec_doubles(M);
  // a non-finite parameter fails the cell outright: m32's r2 clamp (a > 0 ? a : 0)
  // would turn a NaN coordinate or lengthscale into distance 0, not into a NaN pivot
  if (tid == 0) *nonfin = 0;
  __syncthreads();
  for (int e = tid; e < P; e += 256)
    if (!(fabs(th[e]) <= 1.7976931348623157e308)) *nonfin = 1;
  const double ls[3] = {softplus(th[0]), softplus(th[1]), softplus(th[2])};
  const double var = softplus(th[3]), s2 = softplus(th[4]) + LIK_LOWER;
  const double* Z = th + 6;
  const double* qg = th + 6 + 3 * M;
  const double* St = th + 6 + 4 * M;
  for (int m = tid; m < M; m += 256)
    for (int d = 0; d < 3; ++d) Zs[m * 3 + d] = Z[m * 3 + d] / ls[d];
  __syncthreads();
  for (int e = tid; e < M * M; e += 256) {
    const int i = e / M, j = e % M;
    double ee;
    W[e] = var * m32(Zs + i * 3, Zs + j * 3, ee) + (i == j ? JITTER : 0.0);
  }
  __syncthreads();
  const bool ok = chol_lds(W, L, M, flag) && *nonfin == 0;
  // KL = (q.q + |S|^2 - M - sum log S_ii^2) / 2: lanes by shuffle tree, waves in index order
  const int ntri = M * (M + 1) / 2;
  double kl = 0.0;
  for (int e = tid; e < ntri; e += 256) kl += St[e] * St[e];
  for (int m = tid; m < M; m += 256) {
    const double d = St[tri_index(m, m)];
    kl += qg[m] * qg[m] - log(d * d) - 1.0;
  }
  for (int o = 32; o > 0; o >>= 1) kl += __shfl_down(kl, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = kl;
  __syncthreads();
  if (tid == 0) {
    r[R_LS] = ls[0];
    r[R_LS + 1] = ls[1];
    r[R_LS + 2] = ls[2];
    r[R_KVAR] = var;
    r[R_S2] = s2;
    r[R_C] = th[5];
    r[R_KL] = 0.5 * (((red[0] + red[1]) + red[2]) + red[3]);
    r[R_BAD] = ok ? 0.0 : 1.0;
    status[blockIdx.x] = ok ? 0 : 1;
  }
  double* o = r + R_ZS;
  for (int e = tid; e < 3 * M; e += 256) o[e] = Zs[e];
  o += 3 * M;
  for (int e = tid; e < M; e += 256) o[e] = qg[e];
  o += M;
  for (int e = tid; e < M * M; e += 256)
    if (e % M <= e / M) o[tri_index(e / M, e % M)] = L[e];
  o += ntri;
  for (int e = tid; e < ntri; e += 256) o[e] = St[e];
}

// Points of every kernel below: cell c of the chunk is cell c0 + c of the call
// and owns rows offs[c0 + c] .. offs[c0 + c + 1] - 1.  `pts` (and `y`) hold
// row i of the call at index i - pbase (pbase = 0 for the caller's device
// arrays, the chunk's first row for the staged host copy); the chunk's own
// arrays (mean, var, A, SA) are indexed from the chunk's first row obase.
struct SpChunk {
  const double* rec;
  const double* pts;
  const double* y;
  const int64_t* offs;
  int64_t c0, pbase, obase;
  int M;
};

// Tile blockIdx.x of cell blockIdx.y, lane = target (or observation).
// mean / var: outputs (predict);  A / SA: the M x nt panels a and S'a of each
// cell, row-major with the targets contiguous, or null;  part / poffs: one
// partial of sum v_i per block at poffs[cell] - poffs[c0] + tile (ELBO).
__global__ void __launch_bounds__(TL) k_sp_targets(SpChunk k, int with_noise,
                                                   double* __restrict__ mean,
                                                   double* __restrict__ var,
                                                   double* __restrict__ A, double* __restrict__ SA,
                                                   double* __restrict__ part,
                                                   const int64_t* __restrict__ poffs) {
  extern __shared__ double lds[];
  const int M = k.M, ntri = M * (M + 1) / 2, lane = threadIdx.x;
  const int64_t cell = k.c0 + blockIdx.y;
  const int64_t t0 = k.offs[cell], nt = k.offs[cell + 1] - t0;
  if ((int64_t)blockIdx.x * TL >= nt) return;  // uniform over the block
  const double* r = k.rec + (size_t)blockIdx.y * rec_doubles(M);
  double* Zs = lds;
  double* q = Zs + 3 * M;
  double* L = q + M;
  double* S = L + ntri;
  double* ap = S + ntri + lane;  // a[m] of this lane at ap[m * TL]
  double* red = S + ntri + M * TL;
  for (int e = lane; e < 4 * M + 2 * ntri; e += TL) lds[e] = r[R_ZS + e];
  __syncthreads();
  const double kvar = r[R_KVAR], s2 = r[R_S2];
  const bool bad = r[R_BAD] != 0.0;
  const int64_t i = (int64_t)blockIdx.x * TL + lane;
  const bool live = i < nt;
  double v = 0.0;
  if (live && bad && !part) mean[t0 - k.obase + i] = var[t0 - k.obase + i] = NAN;
  if (live && !bad) {
    const double* xp = k.pts + (t0 - k.pbase + i) * 3;
    const double x[3] = {xp[0] / r[R_LS], xp[1] / r[R_LS + 1], xp[2] / r[R_LS + 2]};
    // a = L^-1 k_u by forward substitution
    for (int m = 0; m < M; ++m) {
      double ee;
      double a = kvar * m32(Zs + m * 3, x, ee);
      const double* Lm = L + tri_index(m, 0);
      for (int j = 0; j < m; ++j) a -= Lm[j] * ap[j * TL];
      ap[m * TL] = a / Lm[m];
    }
    double* Ac = A ? A + (size_t)M * (t0 - k.obase) + i : nullptr;
    double* SAc = SA ? SA + (size_t)M * (t0 - k.obase) + i : nullptr;
    double mu = 0.0, aa = 0.0, ss = 0.0;
    for (int m = 0; m < M; ++m) {
      const double a = ap[m * TL];
      mu += a * q[m];
      aa += a * a;
      if (Ac) Ac[(size_t)m * nt] = a;
    }
    for (int j = 0; j < M; ++j) {
      double sa = 0.0;
      for (int m = j; m < M; ++m) sa += S[tri_index(m, j)] * ap[m * TL];
      ss += sa * sa;
      if (SAc) SAc[(size_t)j * nt] = sa;
    }
    mu = r[R_C] + mu;
    const double fv = (kvar - aa) + ss;
    if (part) {
      const double res = k.y[t0 - k.pbase + i] - mu;
      v = -0.5 * LOG2PI - 0.5 * log(s2) - 0.5 * (res * res + fv) / s2;
    } else {
      mean[t0 - k.obase + i] = mu;
      var[t0 - k.obase + i] = with_noise ? fv + s2 : fv;
    }
  }
  if (part) {  // lanes by shuffle tree, then the two waves in order
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((lane & 63) == 0) red[lane >> 6] = v;
    __syncthreads();
    if (lane == 0) part[poffs[cell] - poffs[k.c0] + blockIdx.x] = red[0] + red[1];
  }
}

// elbo[c] = (sum of the cell's partials in index order) - KL; NaN for a failed cell
__global__ void __launch_bounds__(64) k_sp_reduce(const double* __restrict__ rec, int M,
                                                  const double* __restrict__ part,
                                                  const int64_t* __restrict__ poffs, int64_t c0,
                                                  double* __restrict__ elbo) {
  if (threadIdx.x != 0) return;
  const double* r = rec + (size_t)blockIdx.x * rec_doubles(M);
  const int64_t p0 = poffs[c0 + blockIdx.x] - poffs[c0], p1 = poffs[c0 + blockIdx.x + 1] - poffs[c0];
  double s = 0.0;
  for (int64_t p = p0; p < p1; ++p) s += part[p];
  elbo[blockIdx.x] = r[R_BAD] != 0.0 ? NAN : s - r[R_KL];
}

// 64 x 64 tile (it, jt) of cell blockIdx.y's covariance, row-major nt x nt at
// cov + coffs[cell] - coffs[c0].  Rows i from LDS (a broadcast per wave),
// lane = column j; thread t takes rows 16 (t >> 6) .. + 15.  Both triangles are
// computed: entry (i, j) and entry (j, i) are the same products summed in the
// same order, so they are equal bit for bit, and entry (i, i) repeats var_i's
// own arithmetic (it is written from var all the same).
__global__ void __launch_bounds__(256) k_sp_cov(SpChunk k, const double* __restrict__ A,
                                                const double* __restrict__ SA,
                                                const double* __restrict__ var,
                                                double* __restrict__ cov,
                                                const int64_t* __restrict__ coffs) {
  extern __shared__ double lds[];
  const int M = k.M;
  const int64_t cell = k.c0 + blockIdx.y;
  const int64_t t0 = k.offs[cell], nt = k.offs[cell + 1] - t0;
  const int64_t T = (nt + CT - 1) / CT;
  if ((int64_t)blockIdx.x >= T * T) return;
  const int64_t it = blockIdx.x / T, jt = blockIdx.x % T;
  const double* r = k.rec + (size_t)blockIdx.y * rec_doubles(M);
  const double* Ac = A + (size_t)M * (t0 - k.obase);
  const double* SAc = SA + (size_t)M * (t0 - k.obase);
  double* C = cov + (coffs[cell] - coffs[k.c0]);
  double* Ai = lds;
  double* Si = Ai + M * CT;
  double* xi = Si + M * CT;  // [64][3] scaled row targets
  const int tid = threadIdx.x;
  for (int e = tid; e < M * CT; e += 256) {
    const int m = e / CT;
    const int64_t i = it * CT + e % CT;
    Ai[e] = i < nt ? Ac[(size_t)m * nt + i] : 0.0;
    Si[e] = i < nt ? SAc[(size_t)m * nt + i] : 0.0;
  }
  if (tid < CT * 3) {
    const int64_t i = it * CT + tid / 3;
    xi[tid] = i < nt ? k.pts[(t0 - k.pbase + i) * 3 + tid % 3] / r[R_LS + tid % 3] : 0.0;
  }
  __syncthreads();
  const int lane = tid & 63, w = tid >> 6;
  const int64_t j = jt * CT + lane;
  if (j >= nt) return;
  const bool bad = r[R_BAD] != 0.0;
  const double kvar = r[R_KVAR];
  const double* xp = k.pts + (t0 - k.pbase + j) * 3;
  const double xj[3] = {xp[0] / r[R_LS], xp[1] / r[R_LS + 1], xp[2] / r[R_LS + 2]};
  double aa[16], ss[16];
  for (int q = 0; q < 16; ++q) aa[q] = ss[q] = 0.0;
  for (int m = 0; m < M; ++m) {
    const double aj = Ac[(size_t)m * nt + j], sj = SAc[(size_t)m * nt + j];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      aa[q] += Ai[m * CT + w * 16 + q] * aj;
      ss[q] += Si[m * CT + w * 16 + q] * sj;
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int rr = w * 16 + q;
    const int64_t i = it * CT + rr;
    if (i >= nt) break;
    double ee;
    double c = (kvar * m32(xi + rr * 3, xj, ee) - aa[q]) + ss[q];
    if (i == j) c = var[t0 - k.obase + i];
    C[(size_t)i * nt + j] = bad ? NAN : c;
  }
}

// ------------------------------------------------------------------- host --

enum { S_MODEL, S_TARGETS, S_COV, S_REDUCE, S_COUNT };
const char* kStage[S_COUNT] = {"svgp_model", "svgp_targets", "svgp_cov", "svgp_reduce"};

constexpr int64_t CHUNK_CELLS = 32768;   // cells per chunk at most (the grids' y dimension)
constexpr int64_t CHUNK_SLACK = 16 * 32;  // rounding of the chunk-wide arrays (doubles)

// What both entry points do.  pts / y / offs: the targets (y null) or the
// observations of every cell; exactly one of (mean, var[, cov]) and elbo is set.
struct Job {
  const double* params;
  int M;
  int64_t ncell;
  const double* pts;
  const double* y;
  const int64_t* offs;
  int with_noise;
  double *mean, *var, *cov, *elbo;
  int32_t* status;
};

// A chunk's workspace, described once (nc cells from c0, tt rows from row t0,
// pp covariance elements / ELBO partials): parameter rows, records, status,
// the staged host inputs, the outputs and (cov) the two M x tt panels and the
// covariances, or (ELBO) the block partials.  All chunk-wide, the cells' parts
// back to back: a cell's size for the chunk planner is this layout for the
// cell alone on a counting Carver that does not round.
struct SpArrays {
  double *par, *rec;
  int32_t* stat;
  const double *pts, *y;  // the caller's device arrays (pbase 0) or the chunk's staged rows (pbase t0)
  int64_t pbase;
  double *mean, *var, *A, *SA, *cov, *part, *elbo;
};
SpArrays sp_layout(Carver& cv, const Job& j, bool host_in, hipStream_t st, int64_t c0, int64_t nc, int64_t t0,
                   int64_t tt, int64_t pp) {
  const int P = oi_svgp_param_count(j.M);
  SpArrays a{};
  a.par = stage_host(cv, j.params + c0 * P, nc * P, st);
  a.rec = cv.take(nc * rec_doubles(j.M));
  a.stat = reinterpret_cast<int32_t*>(cv.take(nc));
  a.pts = j.pts;
  a.y = j.y;
  if (host_in) {
    a.pts = stage_host(cv, j.pts + t0 * 3, tt * 3, st);
    a.pbase = t0;
    if (j.elbo) a.y = stage_host(cv, j.y + t0, tt, st);
  }
  if (j.elbo) {
    a.part = cv.take(pp);
    a.elbo = cv.take(nc);
  } else {
    a.mean = cv.take(tt);
    a.var = cv.take(tt);
    if (j.cov) {
      a.A = cv.take(j.M * tt);
      a.SA = cv.take(j.M * tt);
      a.cov = cv.take(pp);
    }
  }
  return a;
}
int64_t cell_pp(const Job& j, int64_t n) { return j.elbo ? (int64_t)blocks(n, TL) : n * n; }
int64_t cell_doubles(const Job& j, int64_t n, bool host_in) {
  Carver cv{nullptr, 0, 1};
  sp_layout(cv, j, host_in, nullptr, 0, 1, 0, n, cell_pp(j, n));
  return cv.off;
}

int run(const Job& j, const oi_options& o) {
  const int M = j.M, P = oi_svgp_param_count(M), RD = rec_doubles(M);
  const int64_t ncell = j.ncell;
  const bool host_in = o.device_inputs == 0, want_cov = j.cov != nullptr, elbo = j.elbo != nullptr;
  hipStream_t st = (hipStream_t)o.stream;
  if (model_lds(M) > LDS_MAX || targets_lds(M) > LDS_MAX || cov_lds(M) > LDS_MAX)
    throw HipErr{"svgp predict: a block's LDS need exceeds 160 KiB"};
  HC(hipFuncSetAttribute((const void*)k_sp_model, hipFuncAttributeMaxDynamicSharedMemorySize, (int)model_lds(M)));
  HC(hipFuncSetAttribute((const void*)k_sp_targets, hipFuncAttributeMaxDynamicSharedMemorySize, (int)targets_lds(M)));
  HC(hipFuncSetAttribute((const void*)k_sp_cov, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cov_lds(M)));
  const auto [cuts, biggest] = plan_chunks(ncell, o, CHUNK_SLACK, CHUNK_CELLS, "SVGP prediction", [&](int64_t c) {
    return cell_doubles(j, j.offs[c + 1] - j.offs[c], host_in);
  });
  // per-cell prefix arrays: rows, covariance elements, ELBO partials
  std::vector<int64_t> pre(ncell + 1, 0);
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t n = j.offs[c + 1] - j.offs[c];
    pre[c + 1] = pre[c] + cell_pp(j, n);
  }
  DevBuf ws((size_t)biggest * 8), doffs((ncell + 1) * 8), dpre((ncell + 1) * 8);
  HC(hipMemcpyAsync(doffs.p, j.offs, (ncell + 1) * 8, hipMemcpyHostToDevice, st));
  HC(hipMemcpyAsync(dpre.p, pre.data(), (ncell + 1) * 8, hipMemcpyHostToDevice, st));
  StageTimer sg(kStage, S_COUNT);
  sg.on = o.profile != 0;
  sg.st = st;
  for (size_t q = 0; q + 1 < cuts.size(); ++q) {
    const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0;
    const int64_t t0 = j.offs[c0], tt = j.offs[c1] - t0, pp = pre[c1] - pre[c0];
    int64_t nmax = 0;
    for (int64_t c = c0; c < c1; ++c) nmax = std::max(nmax, j.offs[c + 1] - j.offs[c]);
    Carver cv{static_cast<double*>(ws.p)};
    const SpArrays a = sp_layout(cv, j, host_in, st, c0, nc, t0, tt, pp);
    if (cv.off > biggest) throw HipErr{"svgp predict: workspace layout exceeds its estimate"};
    const SpChunk k{a.rec, a.pts, a.y, doffs.as<int64_t>(), c0, a.pbase, t0, M};
    const double dM = M, dT = (double)tt;
    sg.begin(S_MODEL, (double)nc * dM * dM * dM / 3.0, 8.0 * (double)nc * (P + RD));
    hipLaunchKernelGGL(k_sp_model, dim3((unsigned)nc), dim3(256), model_lds(M), st, a.par, M, P, a.rec, a.stat);
    KCHK();
    sg.end();
    if (nmax > 0) {
      // per target: the substitution M^2, S'a M^2, k_u and the dot products
      sg.begin(S_TARGETS, dT * (2.0 * dM * dM + 30.0 * dM), 8.0 * dT * (5.0 + (want_cov ? 2.0 * dM : 0.0)));
      hipLaunchKernelGGL(k_sp_targets, dim3(blocks(nmax, TL), (unsigned)nc), dim3(TL), targets_lds(M), st, k,
                         j.with_noise, a.mean, a.var, a.A, a.SA, a.part, dpre.as<int64_t>());
      KCHK();
      sg.end();
    }
    if (want_cov && nmax > 0) {
      const unsigned T = blocks(nmax, CT);
      sg.begin(S_COV, 4.0 * dM * (double)pp, 8.0 * (double)pp);
      hipLaunchKernelGGL(k_sp_cov, dim3(T * T, (unsigned)nc), dim3(256), cov_lds(M), st, k, a.A, a.SA, a.var, a.cov,
                         dpre.as<int64_t>());
      KCHK();
      sg.end();
    }
    if (elbo) {
      sg.begin(S_REDUCE, (double)pp, 8.0 * (double)pp);
      hipLaunchKernelGGL(k_sp_reduce, dim3((unsigned)nc), dim3(64), 0, st, a.rec, M, a.part, dpre.as<int64_t>(), c0,
                         a.elbo);
      KCHK();
      sg.end();
      HC(hipMemcpyAsync(j.elbo + c0, a.elbo, nc * 8, hipMemcpyDeviceToHost, st));
    } else if (tt > 0) {
      HC(hipMemcpyAsync(j.mean + t0, a.mean, tt * 8, hipMemcpyDeviceToHost, st));
      HC(hipMemcpyAsync(j.var + t0, a.var, tt * 8, hipMemcpyDeviceToHost, st));
      if (want_cov && pp > 0) HC(hipMemcpyAsync(j.cov + pre[c0], a.cov, pp * 8, hipMemcpyDeviceToHost, st));
    }
    HC(hipMemcpyAsync(j.status + c0, a.stat, nc * 4, hipMemcpyDeviceToHost, st));
    // the next chunk reuses the workspace
    HC(hipStreamSynchronize(st));
    sg.flush();
  }
  return 0;
}

}  // namespace

int64_t oi_svgp_cell_doubles(int M, int64_t n, bool cov, bool host_inputs, bool elbo) {
  double set;  // of a Job's outputs, the layout asks only which are set
  return cell_doubles(Job{.M = M, .cov = cov ? &set : nullptr, .elbo = elbo ? &set : nullptr}, n, host_inputs);
}

extern "C" int oi_svgp_predict(const double* params, int32_t M, int64_t ncell, const double* xs,
                               const int64_t* toffs, int32_t with_noise, double* mean, double* var,
                               double* cov, int32_t* status, const oi_options* opts) {
  if (ncell < 0) return oi_set_last_error(OI_E_ARG, "negative ncell");
  if (ncell == 0) return 0;
  if (M < 1 || M > MMAX) return oi_set_last_error(OI_E_ARG, "M must be in [1, 64]");
  if (!params) return oi_set_last_error(OI_E_ARG, "null params");
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (int rc = oi_check_offs(toffs, ncell, 0, "toffs")) return rc;
  if (toffs[ncell] > 0 && (!xs || !mean || !var)) return oi_set_last_error(OI_E_ARG, "null xs / mean / var");
  if (with_noise && cov)
    return oi_set_last_error(OI_E_ARG, "cov must be NULL with with_noise (no full-covariance predict_y)");
  if (cov) {  // a cell's covariance stays below 2 GiB, as oi_gpr_predict_multi's
    constexpr int64_t LIM = 0x7FFFFFF0 / 8;
    for (int64_t c = 0; c < ncell; ++c) {
      const int64_t nt = toffs[c + 1] - toffs[c];
      if (nt >= LIM || nt * nt >= LIM)
        return oi_set_last_error(OI_E_ARG, "toffs: a cell has too many targets for cov (nt^2 doubles reach 2 GiB)");
    }
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    return run(Job{params, M, ncell, xs, nullptr, toffs, with_noise ? 1 : 0, mean, var, cov, nullptr, status}, o);
  });
}

extern "C" int oi_svgp_elbo(const double* params, int32_t M, const double* xyt, const double* y,
                            const int64_t* offs, int64_t ncell, double* elbo, int32_t* status,
                            const oi_options* opts) {
  if (ncell < 0) return oi_set_last_error(OI_E_ARG, "negative ncell");
  if (ncell == 0) return 0;
  if (M < 1 || M > MMAX) return oi_set_last_error(OI_E_ARG, "M must be in [1, 64]");
  if (!params) return oi_set_last_error(OI_E_ARG, "null params");
  if (!xyt || !y) return oi_set_last_error(OI_E_ARG, "null xyt / y");
  if (!elbo) return oi_set_last_error(OI_E_ARG, "null elbo");
  if (!status) return oi_set_last_error(OI_E_ARG, "null status");
  if (int rc = oi_check_offs(offs, ncell, 1, "offs")) return rc;
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    return run(Job{params, M, ncell, xyt, y, offs, 0, nullptr, nullptr, nullptr, elbo, status}, o);
  });
}
