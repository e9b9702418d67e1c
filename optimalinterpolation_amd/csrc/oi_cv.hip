// Cross-validation per cell at given hypers from ONE factorisation per cell, on
// the front half of oi_predict.hip (oi_dense.h: generation, Cholesky and the
// solve for zt, with no target): oi_gpr_loo, leave-one-out, and below it
// oi_gpr_lgo, leave-group-out, which keeps the sweep's L^-T and forms the
// blocks of K~^-1 that the groups touch.
//
// Leave-one-out (Rasmussen & Williams, GPML 5.4.2):
//
//   r = z - mean;  K~ = K + sn2 I = L L';  zt = L^-1 r;  W = L^-1
//   q_c = [K~^-1]_cc = sum_r W_rc^2;  alpha_c = [K~^-1 r]_c = sum_r W_rc zt_r
//   mu_c = z_c - alpha_c / q_c;  sd_c = sqrt(1 / q_c)
//   lpl = sum_c [ -log(2 pi)/2 - log sd_c - (z_c - mu_c)^2 / (2 sd_c^2) ]
//
// K~ and its factor come from the front half (PCell with no target); zt is the
// 1 x n row X through oila::trsm_right_lt.  k_loo_sweep
// then builds W one 64-column block panel per workgroup and folds every
// finished 64 x 64 tile into q and alpha; W itself is never kept beyond the
// panel, and K~^-1 is never formed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "oi_dense.h"
#include "oi_gemm.h"

#pragma clang fp contract(off)

using namespace oi_dense;

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

// What oi_gpr_loo and oi_gpr_lgo share per chunk around the front half: the
// sweep's cells and work items, their staging and the launch.
struct Sweep {
  std::vector<LCell> cells;
  std::vector<LItem> items;
  void clear() {
    cells.clear();
    items.clear();
  }
  // the front's cell p with its arrays a as the chunk's next; its rows of mu and sd, its lpl
  void add(const PCell& p, const DenseCell& a, double* mu, double* sd, double* lpl) {
    const int cq = (int)cells.size();
    cells.push_back(LCell{p.K, a.dinv, a.wdt, p.X, p.z, mu, sd, a.part, lpl, p.info, p.status, p.n, p.Np});
    for (int j = 0; j < p.Np / 64; ++j) items.push_back(LItem{cq, j});
  }
  // descriptors up (returned), the front half under its three stage ids, then
  // the sweep as stage s_sweep, which stays open for the caller's tail
  const LCell* run(Front& fr, const char* entry, int s_gen, int s_chol, int s_solve, int s_sweep) {
    // the longest block columns first (j ascending: Np / 64 - j tiles each);
    // ties keep the cells' order
    std::stable_sort(items.begin(), items.end(), [&](const LItem& a, const LItem& b) {
      return cells[a.cell].Np / 64 - a.j > cells[b.cell].Np / 64 - b.j;
    });
    const LCell* dl = fr.la.put(cells);
    fr.factor(entry, s_gen, s_chol, s_solve);
    fr.sg.begin(s_sweep, fr.fl_chol, 0.0);
    if (!items.empty()) {
      const LItem* di = fr.la.put(items);
      hipLaunchKernelGGL(k_loo_sweep, dim3((unsigned)items.size()), dim3(256), 0, fr.st, dl, di);
      KCHK();
    }
    return dl;
  }
};

}  // namespace

extern "C" int oi_gpr_loo(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                          double mean, const double* hyp, double* mu, double* sd, double* lpl,
                          int32_t* status, const oi_options* opts) {
  if (int rc = oi_check_offs(offs, ncell, 0, "offs")) return rc;
  if (ncell == 0) return 0;
  const char* missing = offs[ncell] > 0 && (!mu || !sd) ? "null mu / sd" : nullptr;
  if (int rc = dense_check(xyt, z, offs, nullptr, ncell, hyp, status, missing, {.nsamp = -1})) return rc;
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    Front fr(o, xyt, z, offs, hyp, mean, true, kLooStage, L_COUNT);
    const std::vector<int64_t> cuts = fr.plan(ncell, CHUNK_SLACK, "leave-one-out", [&](int64_t c) {
      return dense_cell_doubles(offs[c + 1] - offs[c], 0, false, fr.in.host, true);
    });
    hipStream_t st = fr.st;
    Sweep sw;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, n0 = offs[c0], nn = offs[c1] - n0;
      fr.begin(c0, c1, nullptr, 0, -1);
      const DenseChunk& k = fr.k;
      sw.clear();
      for (int64_t c = c0; c < c1; ++c) {
        DenseCell a;
        const PCell& p = fr.add(c, 0, 0, a);
        sw.add(p, a, k.mu + (offs[c] - n0), k.sd + (offs[c] - n0), k.lz + (c - c0));
      }
      const LCell* dl = sw.run(fr, "oi_gpr_loo", L_GEN, L_CHOL, L_SOLVE, L_SWEEP);
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
// Leave-group-out cross-validation per cell (GPML 5.4.2 in block form) at
// given hypers, from ONE factorisation per cell:
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
  const char* missing = N > 0 && !group ? "null group" : N > 0 && (!mu || !sd) ? "null mu / sd" : nullptr;
  if (int rc = dense_check(xyt, z, offs, nullptr, ncell, hyp, status, missing, {.nsamp = -1})) return rc;
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
    const std::vector<int64_t> cuts = fr.plan(ncell, LGO_SLACK, "leave-group-out", [&](int64_t c) {
      return lgo_cell_doubles(offs[c + 1] - offs[c], plans[c].g.data(), (int64_t)plans[c].g.size(), host);
    });
    hipStream_t st = fr.st;
    Carver& cv = fr.cv;
    Sweep sw;
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
      fr.begin(c0, c1, nullptr, 0, -1);
      const DenseChunk& k = fr.k;
      const LgoChunk lk = lgo_chunk(cv, !host, nn, ng, st);
      // sorted row of the chunk -> row of the chunk in the caller's order
      perm.resize((size_t)nn);
      for (int64_t c = c0; c < c1; ++c)
        for (int64_t i = 0, n = offs[c + 1] - offs[c], r0 = offs[c] - n0; i < n; ++i)
          perm[r0 + i] = (int32_t)(r0 + plans[c].perm[i]);
      const int32_t* dperm = nn > 0 ? fr.la.put(perm) : nullptr;
      sw.clear();
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
        PCell& p = fr.add(c, 0, 0, a);
        if (!host) {
          p.x = lk.gx + r0 * 3;
          p.z = lk.gz + r0;
        }
        double* alpha = cv.take(p.Np);
        sw.add(p, a, k.mu + r0, k.sd + r0, k.lz + cq);
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
      if (!host && nn > 0) {
        hipLaunchKernelGGL(k_lgo_gather, dim3(blocks(nn, 256)), dim3(256), 0, st, xyt + n0 * 3, z + n0, dperm, lk.gx,
                           lk.gz, nn);
        KCHK();
      }
      // the longest inner dimensions first; ties keep the cells' order
      std::stable_sort(gitems.begin(), gitems.end(), [&](const GItem& a, const GItem& b) {
        return gcells[a.cell].Np / 64 - a.A > gcells[b.cell].Np / 64 - b.A;
      });
      sw.run(fr, "oi_gpr_lgo", G_GEN, G_CHOL, G_SOLVE, G_SWEEP);
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
