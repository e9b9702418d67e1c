// HIP kernels (gfx950 / CDNA4, fp64) for the per-cell full-GP hot path:
// SMLII (GPR_CS2S3.py:107-141) and the GPR3D predict block (GPR_CS2S3.py:173-182)
// for a ragged batch of independent grid cells.  Data layout: oi_device.h.
//
// Per objective evaluation of a cell (T = ceil(n/64) tiles per side):
//   (K + sn2 I, Matern-3/2, GPR:93-94, is never stored: each factor kernel
//                  generates the pristine tiles it reads from the coordinates)
//   k_diag_factor4w(j) factor + invert diagonal tile j: one 256-thread
//                  workgroup per cell, the tile in LDS                   ~n^2 * 64
//   k_panel4(j) / k_panel_even(j), j even: left-looking Cholesky for the column
//                  pair (j, j+1) on one stream of the L tiles (128x128 blocks of
//                  two block rows, or 64x128 blocks of one, 512 threads):
//                  L_ij = (A_ij - sum_{k<j} L_ik L_jk^T) Dinv_jj^T, A_i,j+1 -=
//                  sum_{k<j} L_ik L_j+1,k^T, look-ahead of diagonal tile j+1;
//                  rows j and j+1 of W = L^-1 from one stream of W_k,jj
//   k_chol_panel(j), j odd: finishes column j / W row j with the one pair k = j-1
//                  the even panel left out (two products per tile), look-ahead
//                  of tile j+1                                     (both) 2 n^3/3
//   (forward substitution z = L^-1 r runs inside the factorisation: k_diag_factor4w
//                  applies Dinv_jj to block j, the panels subtract L_ij z_j; and
//                  alpha = W^T z = K^-1 r (GPR:127) is accumulated as each W tile
//                  is finished: alpha_jj += W_j,jj^T z_j; r^T alpha = z^T z)
//   k_lauum_grad1  K^-1 = W^T W, one tile per workgroup, fused with the
//                  gradient traces sum((K^-1 - alpha alpha^T) o dK_j); K and
//                  dK_j are regenerated from coordinates (GPR:130-138)         n^3/3
//   k_finalize     nlZ and dnlZ (GPR:128, GPR:131-138), fixed-order sums
// Predict (GPR:173-182): k* = D kd* (k_diag_factor4w(0)), the Cholesky with the forward
// substitution of r and k* folded in, then k_finalize (fs = mean + v.z,
// sd = sqrt(sf2 - v.v), lZ from z.z): no separate triangular solves.
//
// Every reduction has a fixed order that depends only on the cell, so a
// cell's results are bitwise independent of the batch it runs in.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include "oi_device.h"
#include "oi_gemm.h"
#include "oi_masks.h"

// GEMM1(acc, lds, npairs, pair): the 64x64 tile-GEMM loop of the panel / lauum kernels
#define GEMM1(acc, lds, np, ...) gemm1_kmajor<false>(acc, lds, 4 * (np), 0u, __VA_ARGS__)

#define NB OI_NB
#define SQRT3 1.7320508075688772
#define LOG2PI 1.8378770664093453  // np.log(2*np.pi)

// structurally-zero operand tile (tiles above the block diagonal); device
// globals are zero-initialised by the loader and never written
__device__ double g_zero_tile[OI_TILE];
// OI_DEBUG=1 (oi_set_debug): diagnostic printf from the factorisation
__device__ int g_debug;

extern "C" int oi_set_debug(int on) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_debug), &on, sizeof(int)) == hipSuccess ? 0 : -1;
}

// Descriptor pointers are generic, so plain accesses through them compile to
// flat_* instructions, which count against lgkmcnt as well: every LDS wait and
// single-wave barrier then also waits for the tile stores still in flight.
// gst / gld access through the global address space (global_* instructions).
typedef __attribute__((address_space(1))) double gdouble;
__device__ __forceinline__ void gst(double* p, double v) { *(gdouble*)p = v; }
__device__ __forceinline__ double gld(const double* p) { return *(const gdouble*)p; }
__device__ __forceinline__ size_t tri(int i) { return (size_t)i * (i + 1) / 2; }
__device__ __forceinline__ double* tileL(const OiCell& c, int i, int j) {
  return c.L + (tri(i) + j) * OI_TILE;
}
__device__ __forceinline__ double* tileW(const OiCell& c, int i, int j) {
  return c.W + (tri(i) + j) * OI_TILE;
}
__device__ __forceinline__ double* tileD(const OiCell& c, int j) {
  return c.Dinv + (size_t)j * OI_TILE;
}

// deterministic block reduction of NV values, result valid in thread 0;
// red must hold NWAVES*NV doubles
template <int NV, int NWAVES>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double x = v[q];
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
    v[q] = x;
  }
  __syncthreads();
  if (lane == 0)
    for (int q = 0; q < NV; ++q) red[w * NV + q] = v[q];
  __syncthreads();
  if (t == 0)
    for (int q = 0; q < NV; ++q) {
      double s = red[q];
      for (int ww = 1; ww < NWAVES; ++ww) s += red[ww * NV + q];
      v[q] = s;
    }
}

__device__ __forceinline__ bool decode_tri(int x, int T, int& i, int& j) {
  if (x >= T * (T + 1) / 2) return false;
  int ii = (int)((sqrt(8.0 * x + 1.0) - 1.0) * 0.5);
  while ((ii + 1) * (ii + 2) / 2 <= x) ++ii;
  while (ii * (ii + 1) / 2 > x) --ii;
  i = ii;
  j = x - ii * (ii + 1) / 2;
  return true;
}

// Blocks are dealt round-robin over the 8 XCDs (b, b+8, ... share one).  Deal
// whole CELLS round-robin instead: block b works on cell (b&7) + 8*((b>>3)/gx),
// slot (b>>3) % gx, so all tiles of a cell run on one XCD and share its L2,
// while neighbouring cells (similar sizes: the list is sorted by T) spread
// over all XCDs.  The grid is gx * roundup(ncell, 8) blocks.
__device__ __forceinline__ bool xcd_cell_slot(int gx, int ncell, int& cell, int& x) {
  const int b = blockIdx.x, t = b >> 3;
  cell = (b & 7) + 8 * (t / gx);
  x = t % gx;
  return cell < ncell;
}

// Same cell -> XCD dealing, but the slot-0 workgroups of every cell are
// dispatched first: in k_chol_panel slot 0 also runs the look-ahead of the
// next diagonal tile (j + 1 serial products), the launch's longest chain, so
// all of them start at once instead of trailing the short two-product rows.
__device__ __forceinline__ bool xcd_cell_slot_lead0(int gx, int ncell, int& cell, int& x) {
  const int b = blockIdx.x, t = b >> 3, g0 = (ncell + 7) >> 3;
  if (t < g0) {
    cell = (b & 7) + 8 * t;
    x = 0;
  } else {
    const int u = t - g0;
    cell = (b & 7) + 8 * (u / (gx - 1));
    x = 1 + u % (gx - 1);
  }
  return cell < ncell;
}

// ------------------------------------------------ the covariance, generated
// A = M = D Kd D + sn2 I for the sites (K + sn2 I of GPR:93-94 / GPR:126,
// oi_device.h; identity on padding) is never stored (the kernel that wrote
// it once per round, only for the factor kernels to read it back, went in
// round 5).  The kernel that first reads a pristine tile generates it from the
// coordinates instead: k_diag_factor4w(0) the first diagonal tile, the even
// panels every tile of their column j (and the partial update of column j+1),
// k_chol_panel its column at j = 1 and every look-ahead diagonal tile.
// SiteBlk: the 64 sites of one block -- scaled coordinates sqrt(3) x_d / ell_d
// (exactly k_lauum_grad1's) and the site weights d, 0 past n.
struct SiteBlk {
  double u[3][NB];
  double d[NB];
};

__device__ __forceinline__ void stage_sites(const OiCell& c, int b, SiteBlk* S, int t, int nt) {
  double* dst = &S->u[0][0];
  for (int e = t; e < 4 * NB; e += nt) {
    const int d = e >> 6, a = b * NB + (e & 63);
    double v = 0.0;
    if (a < c.n) v = d < 3 ? (SQRT3 * c.xyt[3 * a + d]) / c.hyp[d] : c.dw[a];
    dst[e] = v;
  }
}

// A[a][b] for row site a = 64 ib + r (block R) and column site b = 64 jb + q
// (block C): (d_a d_b) sf2 (1 + Q) e^-Q (+ sn2 if a = b), Q the scaled distance
__device__ __forceinline__ double amat(const SiteBlk& R, int r, int a, const SiteBlk& C, int q, int b, int n,
                                       double sf2, double sn2) {
  if (a >= n || b >= n) return a == b ? 1.0 : 0.0;
  const double d0 = R.u[0][r] - C.u[0][q], d1 = R.u[1][r] - C.u[1][q], d2 = R.u[2][r] - C.u[2][q];
  const double Q = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  double v = (R.d[r] * C.d[q]) * (sf2 * ((1.0 + Q) * exp(-Q)));
  if (a == b) v += sn2;
  return v;
}

// a generated tile (ib, jb): element (r, q) -- row r of block ib, column q of block jb
struct GenTile {
  const SiteBlk* R;
  const SiteBlk* C;
  int ib, jb, n;
  double sf2, sn2;
  __device__ __forceinline__ double operator()(int r, int q) const {
    return amat(*R, r, ib * NB + r, *C, q, jb * NB + q, n, sf2, sn2);
  }
};
__device__ __forceinline__ GenTile gen_tile(const OiCell& c, const SiteBlk* R, int ib, const SiteBlk* C, int jb) {
  return GenTile{R, C, ib, jb, c.n, c.hyp[3], c.hyp[4]};
}

// ------------------------------------------------- diagonal-tile helpers
// v_readlane broadcast of a double from one lane of the wave
__device__ __forceinline__ double rdlane(double v, int lane) {
  const long long x = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(x & 0xffffffffLL), lane);
  const int hi = __builtin_amdgcn_readlane((int)(x >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// acc (16x16, lane l holds rows (l>>4) + 4q, column l&15) += A B with
// A[m][k] = Am[m * la + k] (or Am[k * la + m] if a_km) and B[k][n] = Bt[n * lb + k]
__device__ __forceinline__ void mfma16x16(d4& acc, const double* Am, int la, bool a_km, const double* Bt,
                                          int lb) {
  const int l = threadIdx.x & 63, fr = l & 15, fk = l >> 4;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int k = 4 * kk + fk;
    const double a = a_km ? Am[k * la + fr] : Am[fr * la + k];
    acc = MFMA64(a, Bt[fr * lb + k], acc);
  }
}

// stage timestamps for tools/diag_engine_probe (compiled in only there)
#ifdef OI_DIAG_TIMING
// sums of the stamps over every diagonal factor block 0 runs (slot 15: calls);
// differences of consecutive sums = total cycles per stage
__device__ long long g_diag_stamps[16];
#define DIAG_STAMP(k) \
  do { if (threadIdx.x == 0 && blockIdx.x == 0) { g_diag_stamps[k] += clock64(); if (k == 0) g_diag_stamps[15] += 1; } } while (0)
extern "C" int oi_diag_stamps(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_stamps), sizeof(long long) * 16) != hipSuccess) return 1;
  if (reset) {
    long long z[16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_diag_stamps), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
#else
#define DIAG_STAMP(k) do {} while (0)
#endif

// ------------------------------------------ k_diag_factor4w(j)
// Factor + invert diagonal tile j of every cell, one 256-thread workgroup per
// cell.  The tile already holds the updated A_jj - sum_{k<j} L_jk L_jk^T
// (the previous step's look-ahead wrote it); for j = 0 the kernel generates
// K + sn2 I itself and initialises the forward substitution's right-hand sides.  Writes L_jj, its log-determinant, Dinv_jj and (eval mode) W_jj.
// Pivot <= 0 -> status = not PD (GPR:139-140); NaN pivots propagate like the
// reference's numpy/OpenBLAS cholesky.  Four waves with the tile in LDS, for
// latency (config 1's lone cell waits for four of these per evaluation; the
// round-2 single-wave kernel spent half its 60 k cycles outside the serial
// potrf -- retired in round 4 with the round-1 kernel):
//   potrf: 16-column panels; wave 0 factors the panel (row per lane; the
//          next pivot's column value by v_readlane, the rest of the column
//          through LDS one column late), all four waves then apply the trailing
//          update A_IK -= P_I P_K^T (I >= K > J) on v_mfma_f64_16x16x4f64;
//   inverse: wave b inverts diagonal block b by forward substitution, one
//          lane per column (L read by LDS broadcast), then the off-diagonal
//          blocks Inv_IJ = -Inv_II sum_{K=J}^{I-1} L_IK Inv_KJ by levels
//          I - J = 1, 2, 3, one block per wave;
//   stores of L, Dinv and W by all 256 threads (coalesced columns).
// LDS (77 KB, two workgroups per CU): As = the tile, then L (row-major, stride
// 65, zero above the diagonal); Is = Inv (row-major, zero above); per-wave
// 16 x 17 scratch; z_j / v_j.
#define DW_LD 65
// workgroup barrier that waits for this wave's LDS operations only: HIP's
// __syncthreads() is a workgroup-scope release, which also waits for every
// outstanding global store (vmcnt(0)) -- here the L / Dinv / W stores would
// stall each following phase on HBM write latency.  The workgroup shares only
// LDS data between phases; the "memory" clobber keeps the compiler from moving
// memory operations across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// potrf of the 64 x 64 tile in As (row-major, stride DW_LD, lower triangle; the
// upper triangle is scratch) on four waves, As <- L with zeros above the
// diagonal.  Returns the smallest pivot in wave 0 (+inf in the other waves;
// minNum passes a NaN pivot over, as the reference's cholesky does).
// Broadcasts (round 6): the element the next column's pivot waits for comes by
// v_readlane; the rest of column q (rows c0+q+2 ..) goes through `bc` in LDS
// -- one store, then uniform-address reads, against two v_readlane per element
// -- the same doubles in the same update order.
// Y (optional): the tile's global storage -- panel J-1's columns of L, final,
// are stored by waves 1-3 while wave 0 factors panel J (the last panel's by
// the caller), instead of all 64 columns after the factorisation
__device__ __forceinline__ double potrf4w(double* As, double* bc, double* Y = nullptr) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fk = lane >> 4;
  double dmin = __builtin_inf();
#pragma unroll
  for (int J = 0; J < 4; ++J) {
    const int c0 = 16 * J;
    if (w == 0) {
      const int r = lane;
      double R[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) R[q] = As[r * DW_LD + c0 + q];
      // rows r < c0 + q compute values nobody reads (zeros are written back)
      double bq[16], qprev = 0.0;  // column q-1's broadcast elements (rows c0+q+1 ..) and its qd
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int cc = c0 + q;
        const double d = rdlane(R[q], cc);
        dmin = fmin(dmin, d);
        // 1/sqrt(d) by v_rsq_f64 + two Newton steps (<= 1 ulp)
        double il = __builtin_amdgcn_rsq(d);
        il = fma(0.5 * il, fma(-d * il, il, 1.0), il);
        il = fma(0.5 * il, fma(-d * il, il, 1.0), il);
        const double l = d * il;
        const double qd = R[q] * il;
        R[q] = r == cc ? l : qd;
        // column q-1's updates of rows c0+q+1 .. (their broadcasts were read
        // during this column's pivot), before column q's own updates of them
        if (q >= 1 && q - 1 < 14)
#pragma unroll
          for (int s2 = q + 1; s2 < 16; ++s2) R[s2] -= qprev * bq[s2];
        if (q < 15) R[q + 1] -= qd * rdlane(R[q], c0 + q + 1);
        if (q < 14) {
          double* bb = bc + 64 * (q & 1);
          bb[r] = R[q];
#pragma unroll
          for (int s2 = q + 2; s2 < 16; ++s2) bq[s2] = bb[c0 + s2];
        }
        qprev = qd;
        __builtin_amdgcn_sched_barrier(0);  // (later columns' broadcasts not hoisted: registers)
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) As[r * DW_LD + c0 + q] = r >= c0 + q ? R[q] : 0.0;
    } else if (Y && w < 4 && J >= 1) {
#pragma unroll
      for (int u = 0; u < 6; ++u) {  // 16 columns x 64 rows over 192 lanes; column-major, zeros above
        const int e = (w - 1) * 64 + lane + 192 * u;
        if (u < 5 || e < 1024) {
          const int q = 16 * (J - 1) + (e >> 6), r = e & 63;
          gst(Y + q * NB + r, r >= q ? As[r * DW_LD + q] : 0.0);
        }
      }
    }
    lds_barrier();
    if (J == 3) break;
    // trailing update A_IK -= P_I P_K^T for J < K <= I (P: the panel's rows),
    // 6 / 3 / 1 blocks of 16 x 16 over the four waves; the diagonal blocks'
    // upper halves are scratch until their panel writes zeros back
    const int nblk = (3 - J) * (4 - J) / 2;
    for (int b = w; w < 4 && b < nblk; b += 4) {
      int I = J + 1, rem = b;
      while (rem >= I - J) {
        rem -= I - J;
        ++I;
      }
      const int K = J + 1 + rem;
      d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
      mfma16x16(acc, As + 16 * I * DW_LD + c0, DW_LD, false, As + 16 * K * DW_LD + c0, DW_LD);
#pragma unroll
      for (int q = 0; q < 4; ++q) As[(16 * I + fk + 4 * q) * DW_LD + 16 * K + fr] -= acc[q];
    }
    lds_barrier();
  }
  return dmin;
}

// Packed storage (round 5): the factored tile keeps L in the lower triangle of
// As (row-major, stride DW_LD = 65) and its inverse in the strict upper one --
// Inv[R][C] (R >= C) at As[C * DW_LD + R + 1] -- so the diagonal factor needs
// one 64 x 65 array (33 KB) and fits in a panel kernel's LDS (the look-ahead
// workgroup of every panel launch factors the next diagonal tile itself).
__device__ __forceinline__ double& inv_at(double* As, int R, int C) { return As[C * DW_LD + R + 1]; }
__device__ __forceinline__ double inv_get(const double* As, int R, int C) {
  // an unconditional read (row C, column R + 1 <= 64 always exists) masked to 0
  // above the diagonal: a `R >= C ? load : 0` compiled to exec-masked loads
  const unsigned long long v = __builtin_bit_cast(unsigned long long, As[C * DW_LD + R + 1]);
  return __builtin_bit_cast(double, R >= C ? v : 0ull);
}

// Inv <- L^-1 of the factored tile in As (packed, above); waves 0..3 work, every
// wave of the workgroup takes the barriers (so 512-thread callers may run it).
// dump: 64 doubles of scratch (the zeros above the diagonal of each column's
// x are stored there rather than under a per-element branch: a conditional
// store with a lane-dependent bound made the compiler take 256 VGPRs)
__device__ __forceinline__ void trtri4w(double* As, double* dump) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fk = lane >> 4;
  if (w < 4) {
    // column fr of Inv_ww: x = L_ww^-1 e_fr, right-looking (x_i final once the
    // columns before it are applied; the updates of later rows are independent),
    // x_i scaled by 1/L_ii as LAPACK's dtrti2 does (lane i holds 1/L_ii)
    const int o = 16 * w;
    const double rl = 1.0 / As[(o + fr) * DW_LD + o + fr];
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = i == fr ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[i] *= rdlane(rl, i);  // rows above the column: exact zeros
#pragma unroll
      for (int k = i + 1; k < 16; ++k) x[k] -= As[(o + k) * DW_LD + o + i] * x[i];
    }
    if (fk == 0)
#pragma unroll
      for (int i = 0; i < 16; ++i) *(i >= fr ? &inv_at(As, o + i, o + fr) : dump + lane) = x[i];
  }
  lds_barrier();
  DIAG_STAMP(4);
  // ---------------- off-diagonal blocks by levels (wave w: J = w, I = J + lev):
  // X = sum_K L_IK Inv_KJ on the MFMA unit, then Inv_IJ = -Inv_II X with X
  // taken straight from the accumulator (lane (fk, fr) holds X[fk + 4q][fr],
  // exactly the B operand of k-step q)
#pragma unroll
  for (int lev = 1; lev < 4; ++lev) {
    const int Jb = w, Ib = w + lev;
    if (w < 4 && Ib < 4) {
      d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
      for (int K = Jb; K < Ib; ++K)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int k = 4 * kk + fk;
          acc = MFMA64(As[(16 * Ib + fr) * DW_LD + 16 * K + k], inv_get(As, 16 * K + k, 16 * Jb + fr), acc);
        }
      d4 y = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) y = MFMA64(inv_get(As, 16 * Ib + fr, 16 * Ib + 4 * kk + fk), acc[kk], y);
#pragma unroll
      for (int q = 0; q < 4; ++q) inv_at(As, 16 * Ib + fk + 4 * q, 16 * Jb + fr) = -y[q];
    }
    lds_barrier();
  }
}

// LDS of the diagonal factor: As (packed L / Inv) | Vs | sites (j = 0) | bad |
// (the chains' partials: sb's 4 NB and 4 NB more)
#define DIAG_LDS (NB * DW_LD + 3 * NB + 4 * NB + 2 + 4 * NB)
// diag_tile(j + 1) runs inside the panel kernels on their GEMM LDS arrays
// (the fused look-ahead factor, oi_engine.cpp OI_FUSE_DIAG_MIN)
static_assert(DIAG_LDS <= GEMM1_LDS, "the diagonal factor must fit k_chol_panel's LDS");
static_assert(DIAG_LDS <= GEMM2_LDS, "the diagonal factor must fit k_panel_even's LDS");
static_assert(DIAG_LDS <= GEMM4_LDS, "the diagonal factor must fit k_panel4's LDS");

// the body of k_diag_factor4w for cell c and tile j: 256 threads work, any
// larger workgroup passes every barrier with them; `lds` holds DIAG_LDS doubles.
// in_lds (j > 0, the fused look-ahead of k_chol_panel / k_panel_even): the
// caller left the updated tile in As already (row-major, stride DW_LD, zeros
// above the diagonal -- the doubles the load below would read back), so it is
// handed over without a store -> barrier -> load round trip through L2
__device__ __forceinline__ void diag_tile(const OiCell& c, int j, double* lds, bool in_lds = false) {
  double* As = lds;
  double* Vs = As + NB * DW_LD;
  SiteBlk* sb = (SiteBlk*)(Vs + 3 * NB);
  int& bad = *(int*)(Vs + 7 * NB);
  if (j >= c.T || *c.status != OI_OK) return;
  DIAG_STAMP(0);
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const bool act = t < 256;
  const bool pred = c.mode == OI_MODE_PREDICT;
  double* Y = tileL(c, j, j);
  double* zj = c.vec + j * NB;
  double* vj = c.vec + 3 * c.T * NB + j * NB;
  if (j == 0) {
    // the round's first kernel for the cell.  Duplicate sites make K + sn2 I
    // singular up to sn2: the reference's n x n Cholesky loses the pivot of a
    // repeated row, (sf2 + sn2) - sf2^2 / (sf2 + sn2), to rounding (always once
    // sf2 + sn2 rounds to sf2, sn2 = 0 included; with probability 1/2 at
    // sn2 / sf2 = OI_DUP_NONPD_TAU n_obs) and takes the LinAlgError branch
    // (GPR:139-140); the m x m site form would not notice (oi_device.h).
    // (a non-finite sf2 -- exp overflow at a CG trial point -- makes the
    // reference's K inf / NaN, which numpy's cholesky propagates as NaN rather
    // than raising: no not-PD flag then, the NaNs run through as they do there)
    const double sf2 = c.hyp[3], sn2 = c.hyp[4];
    if (c.n_obs > c.n && isfinite(sf2) && (sf2 + sn2 == sf2 || sn2 < OI_DUP_NONPD_TAU * c.n_obs * sf2)) {
      if (t == 0) *c.status = OI_NOT_PD;
      return;
    }
    // right-hand sides of the forward substitution run inside the
    // factorisation: z = r (site residuals), and for predict v = k* = D kd*
    // (GPR:174, cdist of scaled coordinates); block 0 also into Vs
    const int n = c.n;
    double xs0 = 0.0, xs1 = 0.0, xs2 = 0.0;
    if (pred) {
      xs0 = (SQRT3 * c.xs[0]) / c.hyp[0];
      xs1 = (SQRT3 * c.xs[1]) / c.hyp[1];
      xs2 = (SQRT3 * c.xs[2]) / c.hyp[2];
    }
    for (int a = t; act && a < c.T * NB; a += 256) {
      const double z = a < n ? c.r[a] : 0.0;
      gst(c.vec + a, z);
      double kv = 0.0;
      if (pred && a < n) {
        const double d0 = (SQRT3 * c.xyt[3 * a]) / c.hyp[0] - xs0;
        const double d1 = (SQRT3 * c.xyt[3 * a + 1]) / c.hyp[1] - xs1;
        const double d2 = (SQRT3 * c.xyt[3 * a + 2]) / c.hyp[2] - xs2;
        const double Q = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        kv = c.dw[a] * (sf2 * ((1.0 + Q) * exp(-Q)));
      }
      if (pred) gst(c.vec + 3 * c.T * NB + a, kv);
      if (a < NB) {
        Vs[a] = z;
        Vs[NB + a] = kv;
      }
    }
    // tile (0, 0) generated from the sites (lower triangle; zeros above)
    if (act) stage_sites(c, 0, sb, t, 256);
    lds_barrier();
    const GenTile A0 = gen_tile(c, sb, 0, sb, 0);
#pragma unroll 4
    for (int u = 0; act && u < 16; ++u) {
      const int e = t + 256 * u, q = e >> 6, r = e & 63;
      As[r * DW_LD + q] = r >= q ? A0(r, q) : 0.0;
    }
  } else {
    // element (r, q) of the column-major tile at q*64 + r: 16 coalesced loads per
    // thread; the upper triangle (scratch of the look-ahead) is replaced by zeros
    if (act && !in_lds)
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int e = t + 256 * u, q = e >> 6, r = e & 63;
        const double v = gld(Y + e);
        As[r * DW_LD + q] = r >= q ? v : 0.0;
      }
    if (t < NB) {
      Vs[t] = zj[t];
      Vs[NB + t] = pred ? vj[t] : 0.0;
    }
  }
  lds_barrier();
  DIAG_STAMP(1);
  const double dmin = potrf4w(As, (double*)sb, Y);  // smallest pivot (wave 0); sb: the broadcast scratch
  DIAG_STAMP(2);
  if (t == 0) bad = dmin <= 0.0;
  lds_barrier();
  if (bad) {
    if (t == 0) {
      *c.status = OI_NOT_PD;
      if (g_debug)
        printf("oi debug: not PD: cell n=%d T=%d diagonal tile j=%d hyp %g %g %g %g %g\n", c.n, c.T,
               j, c.hyp[0], c.hyp[1], c.hyp[2], c.hyp[3], c.hyp[4]);
    }
    return;
  }
  // L_jj (column-major): columns 0-47 went out during the potrf, the last panel's here
  if (act)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = 48 * NB + t + 256 * u, q = e >> 6, r = e & 63;
      gst(Y + e, r >= q ? As[r * DW_LD + q] : 0.0);
    }
  DIAG_STAMP(3);
  trtri4w(As, (double*)sb);  // (the j = 0 sites are dead by now)
  DIAG_STAMP(5);
  // Dinv_jj column-major: D[q*64 + r] = Inv[r][q]
  double* Dj = tileD(c, j);
  if (act)
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = t + 256 * u, q = e >> 6, r = e & 63;
      gst(Dj + e, inv_get(As, r, q));
    }
  // forward substitution, block j: z_j = Dinv_jj z_j (the panels subtracted the
  // sum over k < j), v_j likewise for predict; z^T z, z^T v, v^T v partials.
  // Four chains, q = k (mod 4), summed (c0 + c1) + (c2 + c3): chain k on wave k
  // (round 6; the round-5 kernel ran the four interleaved on wave 0 -- the same
  // operations in the same order), the partials through LDS (sb is dead: the
  // sites, the potrf broadcasts and the inverse's scratch are done).  For a
  // fitting cell v = 0: its chains are skipped (they summed +0 exactly)
  double* Pz = (double*)sb;  // 4 x NB
  double* Pv = Vs + 7 * NB + 2;  // 4 x NB, past `bad`
  if (w < 4) {
    double zp = 0.0, vp = 0.0;
#pragma unroll 4
    for (int i = 0; i < NB / 4; ++i) {
      const int q = 4 * i + w;
      const double a = inv_get(As, lane, q);
      zp = fma(a, Vs[q], zp);
      if (pred) vp = fma(a, Vs[NB + q], vp);
    }
    Pz[w * NB + lane] = zp;
    if (pred) Pv[w * NB + lane] = vp;
  }
  lds_barrier();
  if (w == 0) {
    const double zn = (Pz[lane] + Pz[NB + lane]) + (Pz[2 * NB + lane] + Pz[3 * NB + lane]);
    const double vn = pred ? (Pv[lane] + Pv[NB + lane]) + (Pv[2 * NB + lane] + Pv[3 * NB + lane]) : 0.0;
    gst(zj + lane, zn);
    if (pred) gst(vj + lane, vn);
    Vs[2 * NB + lane] = zn;
    double zz = zn * zn, zv = zn * vn, vv = vn * vn;
    for (int o = 32; o >= 1; o >>= 1) {
      zz += __shfl_down(zz, o, 64);
      zv += __shfl_down(zv, o, 64);
      vv += __shfl_down(vv, o, 64);
    }
    if (lane == 0) {
      double* pp = c.part + OI_PART_PRED(c.T * (c.T + 1) / 2, c.T) + 3 * j;
      pp[0] = zz;
      pp[1] = zv;
      pp[2] = vv;
    }
  } else if (w == 1) {
    // sum log L_rr: off wave 0's serial chain (the trtri leaves As's diagonal
    // -- L's -- untouched; its inverse sits above it), beside the forward
    // substitution
    double lg = (j * NB + lane < c.n) ? log(As[lane * (DW_LD + 1)]) : 0.0;
    for (int o = 32; o >= 1; o >>= 1) lg += __shfl_down(lg, o, 64);
    if (lane == 0) {
      const int ntile = c.T * (c.T + 1) / 2;
      c.part[OI_PART_LOGDET(ntile, c.T) + j] = lg;
    }
  }
  DIAG_STAMP(6);
  if (c.mode == OI_MODE_EVAL) {
    // W_jj row-major (W[q][r] = Inv[q][r]) and alpha_j = W_jj^T z_j
    double* Wj = tileW(c, j, j);
    if (act)
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int e = t + 256 * u;
        gst(Wj + e, inv_get(As, e >> 6, e & 63));
      }
    lds_barrier();  // z_j in Vs (and wave 0 done with Pz)
    if (w < 4) {  // alpha's four chains likewise, chain k on wave k
      double ap = 0.0;
#pragma unroll 4
      for (int i = 0; i < NB / 4; ++i) {
        const int q = 4 * i + w;
        ap = fma(inv_get(As, q, lane), Vs[2 * NB + q], ap);
      }
      Pz[w * NB + lane] = ap;
    }
    lds_barrier();
    if (w == 0)
      gst(c.vec + c.T * NB + j * NB + lane, (Pz[lane] + Pz[NB + lane]) + (Pz[2 * NB + lane] + Pz[3 * NB + lane]));
  }
  DIAG_STAMP(7);
}

__global__ __launch_bounds__(256) void k_diag_factor4w(const OiCell* __restrict__ cells,
                                                      const int32_t* __restrict__ list, int j) {
  __shared__ double lds[DIAG_LDS];
  diag_tile(cells[list[blockIdx.x]], j, lds);
}

// wave masks of the GEMM cores (padding, triangular operands, syrk halves): oi_masks.h

#define XLD 65  // LDS row stride of a staged 64x64 tile (doubles)

// Forward substitution inside the factorisation: once tile L_ij (i > j) is
// final, z_i -= L_ij z_j (and v_i -= L_ij v_j for predict; z_j, v_j final since
// k_diag_factor(j)).  fwd_preload, issued before the tile's GEMM loop so its
// latency hides behind it, gives thread t one value: z_i[t] (t < 64), z_j
// (64..127), v_i (128..191), v_j (192..255).  fwd_update then stages z_j, v_j
// in LDS, forms L_ij [z_j v_j] from the tile staged as X[col * ld + row] with
// partial sums over NTHREADS/64 column groups combined in a fixed order, and
// writes z_i, v_i.  scratch (>= (2 * NTHREADS/64 + 2) * 64 doubles) must not
// alias X.  Launch order makes the updates of z_i sequential in j.
__device__ __forceinline__ double fwd_preload(const OiCell& c, int i, int j) {
  const int t = threadIdx.x;
  const bool pred = c.mode == OI_MODE_PREDICT;
  const double* z = c.vec;
  const double* v = c.vec + 3 * c.T * NB;
  if (t < 64) return z[i * NB + t];
  if (t < 128) return z[j * NB + t - 64];
  if (pred && t < 192) return v[i * NB + t - 128];
  if (pred && t < 256) return v[j * NB + t - 192];
  return 0.0;
}

template <int NTHREADS>
__device__ __forceinline__ void fwd_update(const OiCell& c, const double* X, int ld, int i, double pre,
                                           double* scratch) {
  constexpr int G = NTHREADS / 64, CW = NB / G;
  const bool pred = c.mode == OI_MODE_PREDICT;
  const int t = threadIdx.x, row = t & 63, grp = t >> 6;
  double* red = scratch;
  double* zj = scratch + 2 * G * NB;
  double* vj = zj + NB;
  if (t >= 64 && t < 128) zj[t - 64] = pre;
  if (t >= 192 && t < 256) vj[t - 192] = pre;
  __syncthreads();
  double sz = 0.0, sv = 0.0;
#pragma unroll 4
  for (int q = 0; q < CW; ++q) {
    const int col = grp * CW + q;
    const double l = X[col * ld + row];
    sz = fma(l, zj[col], sz);
    if (pred) sv = fma(l, vj[col], sv);
  }
  red[grp * NB + row] = sz;
  red[(G + grp) * NB + row] = sv;
  __syncthreads();
  if (t < 64 || (pred && t >= 128 && t < 192)) {
    const int h = t < 64 ? 0 : 1;
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += red[(h * G + g) * NB + row];
    gst(c.vec + (h ? 3 * c.T * NB : 0) + i * NB + row, pre - a);
  }
}

// alpha = W^T z accumulated while W is built (round 2; replaces k_avec):
// once tile W_{j,jj} is final, alpha_jj += W_{j,jj}^T z_j (z_j final since
// k_diag_factor(j), which also starts alpha_j = W_jj^T z_j).  Same staging as
// fwd_update: the tile sits in LDS as X[col * ld + row] with the product's
// output index as `row`; thread t < 64 preloads alpha_jj[t], 64..127 z_j.
__device__ __forceinline__ double alpha_preload(const OiCell& c, int jj, int j) {
  const int t = threadIdx.x;
  if (t < 64) return c.vec[c.T * NB + jj * NB + t];
  if (t < 128) return c.vec[j * NB + t - 64];
  return 0.0;
}

template <int NTHREADS>
__device__ __forceinline__ void alpha_update(const OiCell& c, const double* X, int ld, int jj, double pre,
                                             double* scratch) {
  constexpr int G = NTHREADS / 64, CW = NB / G;
  const int t = threadIdx.x, row = t & 63, grp = t >> 6;
  double* red = scratch;
  double* zj = scratch + G * NB;
  if (t >= 64 && t < 128) zj[t - 64] = pre;
  __syncthreads();
  double sa = 0.0;
#pragma unroll 4
  for (int q = 0; q < CW; ++q) {
    const int col = grp * CW + q;
    sa = fma(X[col * ld + row], zj[col], sa);
  }
  red[grp * NB + row] = sa;
  __syncthreads();
  if (t < 64) {
    double a = 0.0;
    for (int g = 0; g < G; ++g) a += red[g * NB + row];
    gst(c.vec + c.T * NB + jj * NB + row, pre + a);
  }
}

// acc(m, n) = -base[m*64 + n] (the gemm1 accumulator layout)
__device__ __forceinline__ void acc_load_neg(Quad& acc, const double* base) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc.c[mb][nb][r] = -gld(base + acc1_row(mb, r) * NB + acc1_col(nb));
}

// --------------------------------------------------- k_chol_panel(j), j odd
// The even panel of column j-1 summed k < j-1 into column j and W row j; this
// kernel streams the one remaining pair k = j-1 and finishes them.
// One 256-thread workgroup per output tile; logical slots of a cell:
//   x <  T-1-j : tile (i = j+1+x, j) of the factor; slot 0 (i = j+1) then
//                applies the update of diagonal tile j+1 (look-ahead) for
//                k_diag_factor4w(j+1);
//   x >= T-1-j : (eval) tile (j, jj = x-(T-1-j)) of W = L^-1.
// The Dinv_jj product is applied once to the finished sum (post_left;
// "post-form"), A'_ij and Vneg being what the even panel stored:
//   L_ij^T  = Dinv_jj (A'_ij^T - L_j,j-1 L_i,j-1^T)
//   W_j,jj  = Dinv_jj (Vneg - L_j,j-1 W_j-1,jj)   (jj = j-1: no Vneg, W_jj,jj triangular)
// out(m, n) = sum_q Dinv[m][q] S(q, n), S(m, n) = base[m*64 + n] - acc(m, n)
// (base null: the generated pristine tile, gen(n, m); both null: S = -acc).  S is staged in LDS at row stride LDSA = 80 (B operand:
// rows k, k+1 of a 32-lane ds_read_b64 in opposite bank halves); Dinv_jj (column-major,
// lower triangular, zero above the diagonal) is read into registers once, all
// loads in flight together.  The 160 block-k-steps of the triangular product
// are split evenly: wave w owns row blocks {0, 3} (w even) or {1, 2} and column
// blocks 2(w>>1), 2(w>>1)+1 -- 40 MFMAs per wave.  The result is written to
// dst[m*64 + n] and staged in lds as X[m*XLD + n] (what fwd_update /
// alpha_update and the look-ahead read).
__device__ __forceinline__ void post_left(const Quad& acc, double* lds, const double* base, const GenTile* gen,
                                          const double* Dj, double* dst) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int mA = (w & 1) ? 1 : 0, mB = 3 - mA, n0 = 2 * (w >> 1);
  double bv[16];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        bv[(2 * mb + nb) * 4 + r] = base  ? gld(base + acc1_row(mb, r) * NB + acc1_col(nb))
                                    : gen ? (*gen)(acc1_col(nb), acc1_row(mb, r))
                                          : 0.0;
  __syncthreads();  // the GEMM's last LDS reads are done
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // B(q, n) = S[q][n] at q*LDSA + n
        lds[acc1_row(mb, r) * LDSA + acc1_col(nb)] = bv[(2 * mb + nb) * 4 + r] - acc.c[mb][nb][r];
  // A(m, q) = Dinv[m][q] at Dj[q*64 + m]: row block mA needs k-steps kk <= 4 mA + 3, mB up to
  // 4 mB + 3; loaded once S is staged (acc, bv dead: the kernel stays at 4 waves per SIMD)
  double dA[8], dB[16];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) dA[kk] = kk <= 4 * mA + 3 ? gld(Dj + (4 * kk + fk) * NB + 16 * mA + fr) : 0.0;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) dB[kk] = kk <= 4 * mB + 3 ? gld(Dj + (4 * kk + fk) * NB + 16 * mB + fr) : 0.0;
  __syncthreads();
  d4 o[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) o[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int k = 4 * kk + fk;
    const double b0 = lds[k * LDSA + 16 * n0 + fr], b1 = lds[k * LDSA + 16 * n0 + 16 + fr];
    if (kk <= 4 * mA + 3) {  // wave-uniform
      o[0][0] = MFMA64(dA[kk < 8 ? kk : 7], b0, o[0][0]);
      o[0][1] = MFMA64(dA[kk < 8 ? kk : 7], b1, o[0][1]);
    }
    if (kk <= 4 * mB + 3) {
      o[1][0] = MFMA64(dB[kk], b0, o[1][0]);
      o[1][1] = MFMA64(dB[kk], b1, o[1][1]);
    }
  }
  __syncthreads();  // S is read before the result replaces it
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * (a ? mB : mA) + (lane >> 4) + 4 * r, n = 16 * (n0 + b) + fr;
        gst(dst + m * NB + n, o[a][b][r]);
        lds[m * XLD + n] = o[a][b][r];
      }
  __syncthreads();
}

// GEN = (j == 1): k_panel_even(0) / k_panel4(0) had nothing to subtract from
// column 1, so its A_ij are still pristine and generated here (its own
// instantiation: the generating epilogue would cost the j > 1 launches a wave
// per SIMD)
template <bool GEN, bool FUSE>
__device__ __forceinline__ void chol_slot(const OiCell& c, int j, int x, double* lds) {
  constexpr bool fuse = FUSE;
  const int T = c.T;
  if (j >= T || *c.status != OI_OK) return;
  const int ntrsm = T - 1 - j;
  const double* Dj = tileD(c, j);
  Quad acc;
  quad_zero(acc);
  // padding rows of the last block (exact zeros) are skipped per 16x16 block
  const int rT = c.n - NB * (T - 1);
  const int wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
  if (x < ntrsm) {
    const int i = j + 1 + x;
    const double pre = fwd_preload(c, i, j);
    // n = row of block row i: padding rows of the last block are skipped
    const unsigned psk = i == T - 1 ? pad_skip(32 * wr, 32 * wc, NB, rT) : 0u;
    double* Y = tileL(c, i, j);
    // the stored A'_ij enters the accumulators before the GEMM (acc = -A'),
    // so its load overlaps the operand stream instead of following it:
    // afterwards S = A' - sum = -acc (post_left with no base)
    if (!GEN) acc_load_neg(acc, Y);
    gemm1_kmajor<true>(acc, lds, 4, psk, [=, &c](int, const double*& a, const double*& b) {
      a = tileL(c, j, j - 1);
      b = tileL(c, i, j - 1);
    });
    // j = 1: A_ij is still pristine -- generated from the sites (the GEMM's
    // last barrier freed lds)
    if (GEN) {
      SiteBlk* sbl = (SiteBlk*)lds;
      stage_sites(c, i, &sbl[0], threadIdx.x, 256);
      stage_sites(c, j, &sbl[1], threadIdx.x, 256);
      __syncthreads();
      const GenTile Aij = gen_tile(c, &sbl[0], i, &sbl[1], j);
      post_left(acc, lds, nullptr, &Aij, Dj, Y);  // L_ij^T = Dinv_jj (A_ij^T - acc), stored and staged
    } else {
      post_left(acc, lds, nullptr, nullptr, Dj, Y);
    }
    fwd_update<256>(c, lds, XLD, i, pre, lds + NB * XLD);
    if (x != 0) return;
    // ---- look-ahead: diagonal tile j+1 = i.
    // S_d = A_ii - L_ij L_ij^T - sum_{k<j} L_ik L_ik^T; the first product uses
    // this workgroup's own L_ij, staged k-major in lds (X[c*XLD + m] = L_ij[m][c])
    const double* Xs = lds;
    Quad accd;
    quad_zero(accd);
    {
      const int t = threadIdx.x, lane = t & 63, w = t >> 6;
      const int wr = w >> 1, wc = w & 1, fr = lane & 15, fk = lane >> 4;
#pragma unroll 4
      for (int kk = 0; kk < NB / 4; ++kk) {
        const int k = kk * 4 + fk;
        const double a0 = Xs[k * XLD + 32 * wr + fr], a1 = Xs[k * XLD + 32 * wr + 16 + fr];
        const double b0 = Xs[k * XLD + 32 * wc + fr], b1 = Xs[k * XLD + 32 * wc + 16 + fr];
        accd.c[0][0] = MFMA64(a0, b0, accd.c[0][0]);
        accd.c[0][1] = MFMA64(a0, b1, accd.c[0][1]);
        accd.c[1][0] = MFMA64(a1, b0, accd.c[1][0]);
        accd.c[1][1] = MFMA64(a1, b1, accd.c[1][1]);
      }
    }
    __syncthreads();
    // symmetric, and only its lower triangle is read (k_diag_factor): accd(m, n)
    // lands at row n, column m of the column-major tile, so the accumulator
    // blocks with m > n -- the tile's upper triangle -- are skipped
    gemm1_kmajor<true>(accd, lds, 4 * j, lower_blocks(32 * wr, 32 * wc), [=, &c](int p, const double*& a, const double*& b) {
      a = tileL(c, i, p);
      b = a;
    });
    // the diagonal tile is pristine here (no earlier step touches it): generated
    double* Yd = tileL(c, i, i);
    SiteBlk* sbd = (SiteBlk*)lds;
    stage_sites(c, i, sbd, threadIdx.x, 256);
    __syncthreads();
    const GenTile Ad = gen_tile(c, sbd, i, sbd, i);
    if (fuse) {  // the diagonal tile j+1 is final: factor it here, handed over in LDS
      double v[16];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = acc1_row(mb, r), n = acc1_col(nb);
            v[(2 * mb + nb) * 4 + r] = Ad(n, m) - accd.c[mb][nb][r];
          }
      __syncthreads();  // the staged sites are read
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = acc1_row(mb, r), n = acc1_col(nb);  // element (row n, column m)
            lds[n * DW_LD + m] = n >= m ? v[(2 * mb + nb) * 4 + r] : 0.0;
          }
      diag_tile(c, i, lds, true);
      return;
    }
    for (int mb = 0; mb < 2; ++mb)
      for (int nb = 0; nb < 2; ++nb)
        for (int r = 0; r < 4; ++r) {
          const int m = acc1_row(mb, r), n = acc1_col(nb);
          gst(Yd + m * NB + n, Ad(n, m) - accd.c[mb][nb][r]);
        }
    return;
  }
  const int jj = x - ntrsm;
  if (c.mode != OI_MODE_EVAL || jj >= j) return;
  // jj < j-1: W_j,jj holds Vneg = -sum_{k=jj}^{j-2} L_jk W_k,jj (k_panel_even /
  // k_panel4), so W_j,jj = Dinv_jj (Vneg - L_j,j-1 W_j-1,jj);
  // jj = j-1: the sum is the one pair, whose B = W_jj,jj (B(k, n) = 0 for k < n)
  const bool tri = jj == j - 1;
  const double apre = alpha_preload(c, jj, j);
  // m = row of W block row j: padding rows of the last block are skipped
  const unsigned psk = j == T - 1 ? pad_skip(32 * wr, 32 * wc, rT, NB) : 0u;
  double* Wt = tileW(c, j, jj);
  if (!tri) acc_load_neg(acc, Wt);  // Vneg into the accumulators (as A'_ij above)
  auto cm = [=](int ch) { return tri ? cols_below(ch, 32 * wc) : 0u; };
  gemm1_kmajor<true>(acc, lds, 4, psk, [=, &c](int, const double*& a, const double*& b) {
    a = tileL(c, j, j - 1);
    b = tileW(c, j - 1, jj);
  }, cm);
  post_left(acc, lds, nullptr, nullptr, Dj, Wt);  // W_j,jj = Dinv_jj (Vneg - sum), stored and staged
  alpha_update<256>(c, lds, XLD, jj, apre, lds + NB * XLD);  // alpha_jj += W_j,jj^T z_j
}

template <bool GEN, bool FUSE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_chol_panel(const OiCell* __restrict__ cells,
                                                   const int32_t* __restrict__ list, int j,
                                                   int gx, int ncell) {
  __shared__ __attribute__((aligned(16))) double lds[GEMM1_LDS];
  int ci, x;
  if (!xcd_cell_slot_lead0(gx, ncell, ci, x)) return;
  chol_slot<GEN, FUSE>(cells[list[ci]], j, x, lds);
}

// --------------------------------------------------- k_panel_even(j), j even
// Shared-stream form of two consecutive block columns: every streamed tile
// feeds two outputs (64 x 128 block per 512-thread workgroup, gemm2 core), so
// the L / W streams of the left-looking factorisation are read from HBM once
// per PAIR of columns.  Slots of a cell:
//   x <  T-1-j : row i = j+1+x of the factor:
//                  L_ij      = (A_ij - sum_{k<j} L_ik L_jk^T) Dinv_jj^T
//                  A_i,j+1  -= sum_{k<j} L_ik L_j+1,k^T     (partial update of
//                              column j+1; k_chol_panel(j+1) adds k = j)
//                i = j+1 (x = 0) instead completes A_j+1,j+1 (look-ahead):
//                  A_j+1,j+1 -= sum_{k<j} L_j+1,k L_j+1,k^T + L_j+1,j L_j+1,j^T
//   x >= T-1-j : (eval) jj = x-(T-1-j) < j, rows j and j+1 of W = L^-1:
//                  W_j,jj^T  = -(sum_{k=jj}^{j-1} W_k,jj^T L_jk^T) Dinv_jj^T
//                  W_j+1,jj  = Vneg := -sum_{k=jj}^{j-1} L_j+1,k W_k,jj  (finished
//                              by k_chol_panel(j+1))
// Accumulators come out transposed with respect to the tile storage, so each
// 64x64 half goes through LDS and is written back with coalesced 16 B rows.
enum { EMIT_STORE = 0, EMIT_SUB = 1, EMIT_NEG = 2, EMIT_GENSUB = 3 };

// dst[n*64 + m] (op)= X[n*XLD + m] for a tile staged in lds
__device__ __forceinline__ void emit_copy(const double* X, double* dst, int op, const GenTile* gen = nullptr) {
  for (int e = threadIdx.x; e < OI_TILE; e += GEMM_THREADS) {
    const double v = X[(e >> 6) * XLD + (e & 63)];
    if (op == EMIT_STORE)
      gst(dst + e, v);
    else if (op == EMIT_SUB)
      gst(dst + e, gld(dst + e) - v);
    else if (op == EMIT_GENSUB)
      gst(dst + e, (*gen)(e & 63, e >> 6) - v);
    else
      gst(dst + e, -v);
  }
}

// dst[n*64 + m] (op)= D_h[m][n] for the 64x64 half h of a gemm2 accumulator
// (EMIT_GENSUB: dst = A - D_h, A the pristine tile generated by *gen).
// Leaves the staged tile in X[n*XLD + m] (= dst's storage order) for reuse.
__device__ __forceinline__ void stage_half(const Quad& acc, int h, double* X) {
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if (((w & 3) >> 1) == h) {
    for (int mb = 0; mb < 2; ++mb)
      for (int nb = 0; nb < 2; ++nb)
        for (int r = 0; r < 4; ++r)
          X[(acc_col(nb) - 64 * h) * XLD + acc_row(mb, r)] = acc.c[mb][nb][r];
  }
  __syncthreads();
}
__device__ __forceinline__ void emit_half(const Quad& acc, int h, double* X, double* dst, int op,
                                          const GenTile* gen = nullptr) {
  stage_half(acc, h, X);
  emit_copy(X, dst, op, gen);
}

// Post-form (POST): half 0 accumulates sum_{k<j} L_ik L_jk^T (factor) or
// sum_k W_k,jj^T L_jk^T (W rows) and is finished by post_right:
//   L_ij = (A_ij - acc) Dinv_jj^T,   W_j,jj^T = -acc Dinv_jj^T.
// out(m, n) = sum_q S(m, q) Dinv[n][q], S(m, n) = A(m, n) - acc(m, n), A the
// pristine tile generated from the sites (base null: S = -acc).  S is staged in LDS row-major at S[m*SLD + q] (A
// operand, SLD = 66: the ds_read_b64 of rows k, k+1 by one 32-lane group land
// on disjoint banks, 4m + 2k mod 64, and the accumulator write-back is 16
// consecutive doubles per lane group) and Dinv_jj's ten lower 16x16 blocks
// next to it, packed (block (I, K) at (I(I+1)/2 + K) * 256, element (n, k) at
// (k & 15) * 16 + (n & 15): rows k, k+1 in opposite bank halves); both global
// reads are issued before the first barrier.  (Round 2 staged S as X[q*65 + m]
// and packed Dinv at stride 17: 2-way conflicts on every read, PMC
// SQ_LDS_BANK_CONFLICT 1.2e11 over the day.)  All eight waves share
// the 160 block-k-steps of the triangular product: wave w owns row block w & 3
// and column blocks {0, 3} (w < 4) or {1, 2} -- 20 MFMAs each.  The result is
// left staged as X[n*XLD + m] (emit_half's layout) for emit_copy.
#define SLD 66
#define DPK_OFF (NB * SLD)
static_assert(DPK_OFF + 10 * 256 <= GEMM2_LDS, "post_right staging must fit the GEMM LDS");
__device__ __forceinline__ void post_right(const Quad& acc, double* lds, const GenTile* base, const double* Dj) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const bool mine = (w & 3) < 2;  // the waves holding half 0
  double dv[5];                   // 2560 packed Dinv entries, 5 per thread
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int e = t + GEMM_THREADS * q, blk = e >> 8, kl = (e >> 4) & 15, nl = e & 15;
    const int I = blk >= 6 ? 3 : blk >= 3 ? 2 : blk >= 1 ? 1 : 0, K = blk - I * (I + 1) / 2;
    dv[q] = gld(Dj + (16 * K + kl) * NB + 16 * I + nl);
  }
  double bv[16];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        bv[(2 * mb + nb) * 4 + r] = (mine && base) ? (*base)(acc_row(mb, r), acc_col(nb)) : 0.0;
  __syncthreads();  // the GEMM's last LDS reads are done
  if (mine) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          lds[acc_row(mb, r) * SLD + acc_col(nb)] = bv[(2 * mb + nb) * 4 + r] - acc.c[mb][nb][r];
  }
  double* Dp = lds + DPK_OFF;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int e = t + GEMM_THREADS * q, blk = e >> 8, kl = (e >> 4) & 15, nl = e & 15;
    Dp[blk * 256 + kl * 16 + nl] = dv[q];
  }
  __syncthreads();
  const int mb = w & 3, nA = (w >> 2) ? 1 : 0, nB = 3 - nA;
  d4 o0 = (d4){0.0, 0.0, 0.0, 0.0}, o1 = o0;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int k = 4 * kk + fk, K = kk >> 2;
    const double a = lds[(16 * mb + fr) * SLD + k];
    // B(k, n) = Dinv[n][k]: block (nX, K), zero for K > nX (wave-uniform skip)
    if (kk <= 4 * nA + 3) o0 = MFMA64(a, Dp[(nA * (nA + 1) / 2 + K) * 256 + (k & 15) * 16 + fr], o0);
    if (kk <= 4 * nB + 3) o1 = MFMA64(a, Dp[(nB * (nB + 1) / 2 + K) * 256 + (k & 15) * 16 + fr], o1);
  }
  __syncthreads();  // S and Dinv are read before the result replaces S
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 16 * mb + (lane >> 4) + 4 * r;
    lds[(16 * nA + fr) * XLD + m] = o0[r];
    lds[(16 * nB + fr) * XLD + m] = o1[r];
  }
  __syncthreads();
}

// FUSE: the look-ahead slot factors the diagonal tile j+1 itself (its own
// instantiation: with both hand-over paths in one kernel the register
// allocator spilled)
template <bool FUSE>
__global__ __launch_bounds__(GEMM_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_panel_even(const OiCell* __restrict__ cells,
                                                            const int32_t* __restrict__ list,
                                                            int j, int gx, int ncell) {
  constexpr bool fuse = FUSE;
  __shared__ __attribute__((aligned(16))) double lds[GEMM2_LDS];
  __shared__ SiteBlk sb[3];  // sites of block row i, block columns j, j+1
  static_assert(NB * XLD <= GEMM2_LDS, "staging tile must fit the GEMM LDS");
  int ci, x;
  if (!xcd_cell_slot(gx, ncell, ci, x)) return;
  const OiCell& c = cells[list[ci]];
  const int T = c.T;
  if (j >= T || *c.status != OI_OK) return;
  const int ntrsm = T - 1 - j;
  const bool has_next = j + 1 < T;
  const double* Dj = tileD(c, j);
  Quad acc;
  quad_zero(acc);
  // rows / columns of the last block beyond n are padding: their products are
  // exact zeros (identity padding), so those accumulator blocks are skipped
  const int rT = c.n - NB * (T - 1);
  const int w = threadIdx.x >> 6, wr = (w >> 2) & 1, wc = w & 3;
  if (x < ntrsm) {
    const int i = j + 1 + x;
    // m = row of block row i; half 1's n = column of block column j+1
    const int mlim = i == T - 1 ? rT : NB, nlim = (wc >= 2 && j + 1 == T - 1) ? rT : NB;
    const double pre = fwd_preload(c, i, j);
    // the first row's half 1 (x = 0) is the diagonal tile j+1, symmetric: its
    // blocks above the diagonal are never read
    const unsigned sk = pad_skip(32 * wr, 32 * (wc & 1), mlim, nlim) |
                        (x == 0 && wc >= 2 ? upper_blocks(32 * wr, 32 * (wc - 2)) : 0u);
    stage_sites(c, i, &sb[0], threadIdx.x, GEMM_THREADS);  // read after the GEMM's barriers
    stage_sites(c, j, &sb[1], threadIdx.x, GEMM_THREADS);
    stage_sites(c, j + 1, &sb[2], threadIdx.x, GEMM_THREADS);
    gemm2_kmajor<true>(acc, lds, j, [=, &c](int p, const double*& a, const double*& b0, const double*& b1) {
      a = tileL(c, i, p);
      b0 = tileL(c, j, p);
      b1 = tileL(c, j + 1, p);
    }, sk);
    if (j == 0) __syncthreads();  // no GEMM ran: the staged sites need a barrier
    const GenTile Aij = gen_tile(c, &sb[0], i, &sb[1], j), Ai1 = gen_tile(c, &sb[0], i, &sb[2], j + 1);
    // (x = 0: half 1 is the diagonal tile j+1; it is completed below as
    // (A - acc) - L_j+1,j L_j+1,j^T -- the look-ahead arithmetic of k_panel4,
    // so the two even-column kernels agree bit for bit and the engine may pick
    // either per round, round 5)
    post_right(acc, lds, &Aij, Dj);  // L_ij = (A_ij - acc) Dinv_jj^T, staged
    emit_copy(lds, tileL(c, i, j), EMIT_STORE);
    fwd_update<GEMM_THREADS>(c, lds, XLD, i, pre, lds + NB * XLD);
    if (x != 0) {
      // partial update of A_i,j+1 (empty at j = 0: k_chol_panel(1) generates the tile)
      if (j > 0) emit_half(acc, 1, lds, tileL(c, i, j + 1), EMIT_GENSUB, &Ai1);
      return;
    }
    // i = j+1: the fresh L_j+1,j L_j+1,j^T (staged in lds as X[q*XLD + m] =
    // L[m][q]) in zeroed accumulators; then A_j+1,j+1 - acc and that minus it
    Quad lf;
    quad_zero(lf);
    __syncthreads();
    {
      const int t = threadIdx.x, lane = t & 63, w = t >> 6;
      const int wr = (w >> 2) & 1, wc = w & 3, fr = lane & 15, fk = lane >> 4;
      if ((wc >> 1) == 1) {
        const int c0 = 32 * (wc - 2);
#pragma unroll 4
        for (int kk = 0; kk < NB / 4; ++kk) {
          const int q = kk * 4 + fk;
          const double a0 = lds[q * XLD + 32 * wr + fr], a1 = lds[q * XLD + 32 * wr + 16 + fr];
          const double b0 = lds[q * XLD + c0 + fr], b1 = lds[q * XLD + c0 + 16 + fr];
          lf.c[0][0] = MFMA64(a0, b0, lf.c[0][0]);
          lf.c[0][1] = MFMA64(a0, b1, lf.c[0][1]);
          lf.c[1][0] = MFMA64(a1, b0, lf.c[1][0]);
          lf.c[1][1] = MFMA64(a1, b1, lf.c[1][1]);
        }
      }
    }
    if (fuse) {
      // the diagonal tile j+1 is final: factor it here, handed over in LDS.
      // The two emit_half passes below, with A - acc kept in LDS and
      // (A - acc) - L L^T formed in the lanes holding L L^T -- the doubles
      // they would store and read back
      const int wh = (threadIdx.x >> 6) & 3;
      stage_half(acc, 1, lds);
      for (int e = threadIdx.x; e < OI_TILE; e += GEMM_THREADS) {  // A - acc, in place
        double* xe = lds + (e >> 6) * XLD + (e & 63);
        *xe = Ai1(e & 63, e >> 6) - *xe;
      }
      __syncthreads();
      if ((wh >> 1) == 1)  // the lanes holding L L^T: (A - acc) - L L^T at their own elements
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              lf.c[mb][nb][r] = lds[(acc_col(nb) - 64) * XLD + acc_row(mb, r)] - lf.c[mb][nb][r];
      __syncthreads();
      if ((wh >> 1) == 1)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int m = acc_row(mb, r), n = acc_col(nb) - 64;  // element (row m, column n)
              lds[m * DW_LD + n] = m >= n ? lf.c[mb][nb][r] : 0.0;
            }
      diag_tile(c, i, lds, true);
      return;
    }
    emit_half(acc, 1, lds, tileL(c, i, i), EMIT_GENSUB, &Ai1);
    emit_half(lf, 1, lds, tileL(c, i, i), EMIT_SUB);  // (A_j+1,j+1 - acc) - L L^T
    return;
  }
  const int jj = x - ntrsm;
  if (c.mode != OI_MODE_EVAL || jj >= j) return;
  auto wpair = [=, &c](int p, const double*& a, const double*& b0, const double*& b1) {
    const int k = jj + p;
    a = tileW(c, k, jj);
    b0 = tileL(c, j, k);
    b1 = has_next ? tileL(c, j + 1, k) : g_zero_tile;
  };
  // n = row of W block row j (half 0) or j+1 (half 1)
  const int nlim = ((wc < 2 && j == T - 1) || (wc >= 2 && j + 1 == T - 1)) ? rT : NB;
  const double apre = alpha_preload(c, jj, j);
  // pair k = jj: A = W_jj,jj^T (A(m, k) = 0 for k < m); no row j+1: half 1 idle
  const unsigned sk = pad_skip(0, 32 * (wc & 1), NB, nlim) | (!has_next && wc >= 2 ? 0xFu : 0u);
  auto cm = [=](int ch) { return ch < 4 ? rows_below(ch, 32 * wr) : 0u; };
  gemm2_kmajor<true>(acc, lds, j - jj, wpair, sk, cm);
  post_right(acc, lds, nullptr, Dj);  // W_j,jj^T = -acc Dinv_jj^T, staged
  emit_copy(lds, tileW(c, j, jj), EMIT_STORE);
  alpha_update<GEMM_THREADS>(c, lds, XLD, jj, apre, lds + NB * XLD);  // alpha_jj += W_j,jj^T z_j
  if (has_next) emit_half(acc, 1, lds, tileW(c, j + 1, jj), EMIT_NEG);  // Vneg
}

// --------------------------------------------------- k_panel4(j), j even
// k_panel_even on the 128 x 128 gemm4 core (OI_PANEL4=1): a workgroup owns TWO
// block rows, so every streamed tile feeds four outputs instead of two -- half
// the operand traffic per flop of the 64 x 128 core, whose in-kernel rate
// (53.9 TF/s executed on the day) sits at its own streaming limit (52.5 TF/s,
// tools/gemm4_probe.hip; the 128 x 128 core streams at 61).  Slots of a cell:
//   x <  nfp = ceil((T-1-j)/2) : rows i1 = j+1+2x, i2 = i1+1 (absent past T-1):
//        quadrant (r, 0) = L_{i_r, j} (post-form: (A - sum_k L L^T) Dinv_jj^T),
//        quadrant (r, 1) = partial update of A_{i_r, j+1}; x = 0 completes the
//        diagonal tile A_{j+1, j+1} (look-ahead) with the fresh L_{j+1,j} L^T
//   x >= nfp (eval): W columns jj1 = 2y, jj2 = 2y+1 (y = x - nfp, j even):
//        quadrant (r, 0) = W_{j, jj_r}, quadrant (r, 1) = Vneg of W_{j+1, jj_r}
// Nothing but the accumulators is live across the GEMM (the core takes all 128
// VGPRs at 4 waves per SIMD; even loading A_ij into the accumulators before it
// spills), and the epilogue
// empties the accumulators into LDS first: the column-(j+1) quadrants go out
// as partial updates, then both S tiles are staged (row-major, stride SLD) and
// the two triangular products S_r Dinv_jj^T run together, each wave holding
// its Dinv_jj operand fragments in registers.
__host__ __device__ inline int nslot4_factor(int T, int j) { return (T - j) >> 1; }  // ceil((T-1-j)/2)

// quadrant (qr, 1) of a gemm4 accumulator staged as X[n*XLD + m] (dst's storage order)
__device__ __forceinline__ void stage4_q1(const Quad8& acc, int qr, double* X) {
  const int w = threadIdx.x >> 6;
  if ((w >> 2) == qr && (w & 1) == 1) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) X[(acc4_col(nb) - 64) * XLD + (acc4_row(mb, r) - 64 * qr)] = acc.c[mb][nb][r];
  }
}

// Both triangular products out_r(m, n) = sum_q S_r(m, q) Dinv[n][q], S_r = A_r - acc
// of quadrant (r, 0) (A_r column-major, null: S_r = -acc), r = 0, 1 (`two`):
// stages S_r at lds + r * 64 * SLD (row-major; A_r added with coalesced reads),
// wave w computes row block w & 3 of both tiles against column blocks {0, 3}
// (w < 4) or {1, 2} (20 + 20 MFMAs); returns with the products in o[r][0..1].
__device__ __forceinline__ void post_right4x2(const Quad8& acc, double* lds, const double* Dj, bool two,
                                              const GenTile* A0, const GenTile* A1, d4 (&o)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int mb = w & 3, nA = (w >> 2) ? 1 : 0, nB = 3 - nA;
  if ((w & 1) == 0) {
    const int qr = w >> 2;
    if (qr == 0 || two) {
      double* S = lds + qr * NB * SLD;
#pragma unroll
      for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int r = 0; r < 4; ++r) S[(acc4_row(m2, r) - 64 * qr) * SLD + acc4_col(nb)] = -acc.c[m2][nb][r];
    }
  }
  // (the accumulators are dead from here on)
  // B(k, n) = Dinv[n][k] at Dj[k*64 + n]: this wave's column blocks nA, nB, k-steps kk <= 4 nX + 3
  double bA[8], bB[16];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) bA[kk] = kk <= 4 * nA + 3 ? gld(Dj + (4 * kk + fk) * NB + 16 * nA + fr) : 0.0;
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) bB[kk] = kk <= 4 * nB + 3 ? gld(Dj + (4 * kk + fk) * NB + 16 * nB + fr) : 0.0;
  if (A0) {  // S_r += A_r, A_r generated: element (m, q), 8 per thread and tile.  A
    // wave-instruction covers 32 rows m x 2 columns q (lane l: m = m0 + l/2, q = q0 + l%2):
    // S[m*SLD + q] (bank 4m + 2q) hits 64 distinct banks per 32-lane read and 32 per
    // 16-lane write (2m + q distinct mod 16)
    double av[8], bv[8];
    int ix[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int g = t + GEMM_THREADS * u, b = g >> 6, l = g & 63;
      const int m = 32 * (b & 1) + (l >> 1), q = 2 * (b >> 1) + (l & 1);
      ix[u] = m * SLD + q;
      av[u] = (*A0)(m, q);
      bv[u] = two ? (*A1)(m, q) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      lds[ix[u]] += av[u];
      if (two) lds[NB * SLD + ix[u]] += bv[u];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    o[r][0] = (d4){0.0, 0.0, 0.0, 0.0};
    o[r][1] = o[r][0];
    if (r == 1 && !two) break;
    const double* S = lds + r * NB * SLD;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const double a = S[(16 * mb + fr) * SLD + 4 * kk + fk];
      if (kk <= 4 * nA + 3) o[r][0] = MFMA64(a, bA[kk < 8 ? kk : 7], o[r][0]);
      if (kk <= 4 * nB + 3) o[r][1] = MFMA64(a, bB[kk], o[r][1]);
    }
  }
}

// out tile r (o[r]) staged as X[n*XLD + m] (emit_copy / fwd_update / alpha_update layout)
__device__ __forceinline__ void stage_post4(const d4 (&o)[2][2], int r, double* X) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, mb = w & 3, nA = (w >> 2) ? 1 : 0, nB = 3 - nA;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = 16 * mb + (lane >> 4) + 4 * q;
    X[(16 * nA + fr) * XLD + m] = o[r][0][q];
    X[(16 * nB + fr) * XLD + m] = o[r][1][q];
  }
}

__global__ __launch_bounds__(GEMM_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_panel4(const OiCell* __restrict__ cells, const int32_t* __restrict__ list, int j, int gx, int ncell,
              int fuse) {
  __shared__ __attribute__((aligned(16))) double lds[GEMM4_LDS];
  __shared__ SiteBlk sb[4];  // sites of block rows i1, i2 and block columns j, j+1 (80 KiB in all: 2 per CU)
  static_assert(2 * NB * SLD <= GEMM4_LDS && 2 * NB * XLD <= GEMM4_LDS, "panel4 staging must fit");
  int ci, x;
  if (!xcd_cell_slot(gx, ncell, ci, x)) return;
  const OiCell& c = cells[list[ci]];
  const int T = c.T;
  if (j >= T || *c.status != OI_OK) return;
  const int nfp = nslot4_factor(T, j);
  const bool has_next = j + 1 < T;
  const double* Dj = tileD(c, j);
  const int rT = c.n - NB * (T - 1);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  Quad8 acc;
  quad8_zero(acc);
  d4 o[2][2];
  if (x < nfp) {
    const int i1 = j + 1 + 2 * x, i2 = i1 + 1;
    const bool two = i2 < T;
    const int ti = wr >= 2 ? i2 : i1, tj = wc ? j + 1 : j;
    unsigned skip = 0;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const int m0 = 32 * (wr & 1) + 16 * mb, n0 = 16 * nb;
        const bool off = ti >= T || (ti == T - 1 && m0 >= rT) || (tj == T - 1 && n0 >= rT) ||
                         (x == 0 && wr < 2 && wc == 1 && m0 + 15 < n0);
        if (off) skip |= 1u << (4 * mb + nb);
      }
    auto fpair = [=, &c](int p, const double*& a0, const double*& a1, const double*& b0, const double*& b1) {
      a0 = tileL(c, i1, p);
      a1 = two ? tileL(c, i2, p) : g_zero_tile;
      b0 = tileL(c, j, p);
      b1 = tileL(c, j + 1, p);
    };
    const bool masked = x == 0 || i2 >= T - 1 || j + 1 == T - 1;
    stage_sites(c, i1, &sb[0], t, GEMM_THREADS);  // read after the GEMM's barriers
    stage_sites(c, i2, &sb[1], t, GEMM_THREADS);
    stage_sites(c, j, &sb[2], t, GEMM_THREADS);
    stage_sites(c, j + 1, &sb[3], t, GEMM_THREADS);
    if (masked)
      gemm4_kmajor<true>(acc, lds, 4 * j, skip, fpair);
    else
      gemm4_kmajor<false>(acc, lds, 4 * j, 0u, fpair);
    __syncthreads();  // the GEMM's last LDS reads are done (and the sites are staged)
    const GenTile A1j = gen_tile(c, &sb[0], i1, &sb[2], j), A2j = gen_tile(c, &sb[1], i2, &sb[2], j);
    const GenTile A1n = gen_tile(c, &sb[0], i1, &sb[3], j + 1), A2n = gen_tile(c, &sb[1], i2, &sb[3], j + 1);
    // column j+1: partial updates of A_{i_r, j+1} (x = 0: the diagonal tile, whose
    // L_{j+1,j} L_{j+1,j}^T part follows once that tile is final); at j = 0 the
    // sums are empty and A - 0 is A bit for bit: no round trip through HBM
    if (j > 0) {
      stage4_q1(acc, 0, lds);
      if (two) stage4_q1(acc, 1, lds + NB * XLD);
      __syncthreads();
      emit_copy(lds, tileL(c, i1, j + 1), EMIT_GENSUB, &A1n);
      if (two) emit_copy(lds + NB * XLD, tileL(c, i2, j + 1), EMIT_GENSUB, &A2n);
      __syncthreads();
    }
    post_right4x2(acc, lds, Dj, two, &A1j, two ? &A2j : nullptr, o);
    const double pre1 = fwd_preload(c, i1, j);
    const double pre2 = two ? fwd_preload(c, i2, j) : 0.0;
    __syncthreads();
    stage_post4(o, 0, lds);  // L_{i1,j}
    __syncthreads();
    emit_copy(lds, tileL(c, i1, j), EMIT_STORE);
    fwd_update<GEMM_THREADS>(c, lds, XLD, i1, pre1, lds + NB * XLD);
    if (x == 0) {
      // A_{j+1,j+1} -= L_{j+1,j} L_{j+1,j}^T: the fresh tile is staged as X[q*XLD + m]
      // = L[m][q]; its 10 lower 16x16 blocks go to the 8 waves (blocks w, w + 8)
      double* Y = lds + NB * XLD;
      __syncthreads();  // fwd_update's scratch (= Y) is free
      for (int e = t; e < OI_TILE; e += GEMM_THREADS) Y[(e >> 6) * XLD + (e & 63)] = 0.0;
      __syncthreads();
      const int fr = lane & 15, fk = lane >> 4;
      for (int bidx = w; bidx < 10; bidx += 8) {
        const int bm = bidx >= 6 ? 3 : bidx >= 3 ? 2 : bidx >= 1 ? 1 : 0, bn = bidx - bm * (bm + 1) / 2;
        d4 s = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int kk = 0; kk < NB / 4; ++kk) {
          const int q = 4 * kk + fk;
          s = MFMA64(lds[q * XLD + 16 * bm + fr], lds[q * XLD + 16 * bn + fr], s);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Y[(16 * bn + fr) * XLD + 16 * bm + (lane >> 4) + 4 * r] = s[r];
      }
      __syncthreads();
      // j > 0: the tile holds A - (sum over k < j) from above; j = 0: still pristine
      if (j > 0)
        emit_copy(Y, tileL(c, i1, i1), EMIT_SUB);
      else
        emit_copy(Y, tileL(c, i1, i1), EMIT_GENSUB, &A1n);
    }
    if (two) {
      __syncthreads();
      stage_post4(o, 1, lds);  // L_{i2,j}
      __syncthreads();
      emit_copy(lds, tileL(c, i2, j), EMIT_STORE);
      fwd_update<GEMM_THREADS>(c, lds, XLD, i2, pre2, lds + NB * XLD);
    }
    if (x == 0 && fuse) {  // the diagonal tile j+1 is final: factor it here (no k_diag_factor4w launch)
      __syncthreads();
      diag_tile(c, i1, lds);
    }
    return;
  }
  const int y = x - nfp;
  if (c.mode != OI_MODE_EVAL || 2 * y >= j) return;
  const int jj1 = 2 * y, jj2 = jj1 + 1;
  const int tj = wc ? j + 1 : j;
  unsigned skip = 0;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int n0 = 16 * nb;
      if ((wc == 1 && !has_next) || (tj == T - 1 && n0 >= rT)) skip |= 1u << (4 * mb + nb);
    }
  auto wpair = [=, &c](int p, const double*& a0, const double*& a1, const double*& b0, const double*& b1) {
    const int k = jj1 + p;
    a0 = tileW(c, k, jj1);
    a1 = k >= jj2 ? tileW(c, k, jj2) : g_zero_tile;
    b0 = tileL(c, j, k);
    b1 = has_next ? tileL(c, j + 1, k) : g_zero_tile;
  };
  if (j >= T - 2)
    gemm4_kmajor<true>(acc, lds, 4 * (j - jj1), skip, wpair);
  else
    gemm4_kmajor<false>(acc, lds, 4 * (j - jj1), 0u, wpair);
  __syncthreads();
  if (has_next) {  // Vneg of W_{j+1, jj_r}
    stage4_q1(acc, 0, lds);
    stage4_q1(acc, 1, lds + NB * XLD);
    __syncthreads();
    emit_copy(lds, tileW(c, j + 1, jj1), EMIT_NEG);
    emit_copy(lds + NB * XLD, tileW(c, j + 1, jj2), EMIT_NEG);
    __syncthreads();
  }
  post_right4x2(acc, lds, Dj, true, nullptr, nullptr, o);
  const double apre1 = alpha_preload(c, jj1, j);
  const double apre2 = alpha_preload(c, jj2, j);
  __syncthreads();
  stage_post4(o, 0, lds);  // W_{j,jj1}^T
  __syncthreads();
  emit_copy(lds, tileW(c, j, jj1), EMIT_STORE);
  alpha_update<GEMM_THREADS>(c, lds, XLD, jj1, apre1, lds + NB * XLD);
  __syncthreads();
  stage_post4(o, 1, lds);  // W_{j,jj2}^T
  __syncthreads();
  emit_copy(lds, tileW(c, j, jj2), EMIT_STORE);
  alpha_update<GEMM_THREADS>(c, lds, XLD, jj2, apre2, lds + NB * XLD);
}

// ------------------------------------------------------ k_lauum_grad
// Tile (i, j) of K^-1 = W^T W (K^-1_ij = sum_{k>=i} W_ki^T W_kj), one 256-thread
// workgroup per lower tile (40 KiB LDS -> 4 workgroups per CU), fused with
// sum over the tile of (K^-1 - alpha alpha^T) o {dK_0, dK_1, dK_2, 2K} and the
// trace (GPR:130-138); K and dK are regenerated from the coordinates.
// Strictly-lower entries count twice.
__device__ __forceinline__ void lauum_tile(const OiCell& c, int tile, double* lds) {
  const int T = c.T;
  int i, j;
  if (!decode_tri(tile, T, i, j)) return;
  if (*c.status != OI_OK || c.mode != OI_MODE_EVAL) return;
  Quad acc;
  quad_zero(acc);
  // k rows of the last tile beyond n are padding (exact zeros of W off the
  // padded identity): the last pair's chunks stop at the cell's last row
  const int n = c.n, rT = n - NB * (T - 1);
  const int nch = 4 * (T - i - 1) + (rT + KC - 1) / KC;
  // 16x16 accumulator blocks this wave may drop: the upper triangle of a
  // diagonal tile (never read below) and padding rows / columns
  const int w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  unsigned skip = 0;
  for (int mb = 0; mb < 2; ++mb)
    for (int nb = 0; nb < 2; ++nb) {
      const int m0 = 32 * wr + 16 * mb, n0 = 32 * wc + 16 * nb;
      const bool upper = i == j && m0 + 15 < n0;
      const bool pad = (i == T - 1 && m0 >= rT) || (j == T - 1 && n0 >= rT);
      if (upper || pad) skip |= 1u << (2 * mb + nb);
    }
  auto wpair = [=, &c](int p, const double*& a, const double*& b) {
    a = tileW(c, i + p, i);
    b = tileW(c, i + p, j);
  };
  // pair k = i: A = W_ii^T (A(m, k) = 0 for k < m), and B = W_ii too on the diagonal
  auto cm = [=](int ch) { return ch < 4 ? rows_below(ch, 32 * wr) | (i == j ? cols_below(ch, 32 * wc) : 0u) : 0u; };
  gemm1_kmajor<true>(acc, lds, nch, skip, wpair, cm);
  double* uQ = lds;            // [3][128]: rows 0..63, columns 64..127
  double* uq = lds + 3 * 128;  // [3][128]
  double* al = lds + 6 * 128;  // [128]
  double* dl = lds + 7 * 128;  // [128] site weights d
  double* red = lds + 8 * 128;
  const int t = threadIdx.x;
  __syncthreads();  // the GEMM's last LDS reads are done before the epilogue reuses lds
  if (t < 128) {
    const int a = t < 64 ? i * NB + t : j * NB + (t - 64);
    for (int d = 0; d < 3; ++d) {
      const double xv = a < n ? c.xyt[3 * a + d] : 0.0;
      uQ[d * 128 + t] = (SQRT3 * xv) / c.hyp[d];
      uq[d * 128 + t] = SQRT3 * (xv / c.hyp[d]);
    }
    al[t] = c.vec[T * NB + a];
    dl[t] = a < n ? c.dw[a] : 0.0;
  }
  __syncthreads();
  const double sf2 = c.hyp[3];
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int mb = 0; mb < 2; ++mb)
    for (int nb = 0; nb < 2; ++nb)
      for (int r = 0; r < 4; ++r) {
        const int m = acc1_row(mb, r), nn = acc1_col(nb);
        const int a = i * NB + m, b = j * NB + nn;
        if (a >= n || b >= n || (i == j && m < nn)) continue;
        const double wgt = (a == b) ? 1.0 : 2.0;
        const double w0 = acc.c[mb][nb][r] - al[m] * al[64 + nn];  // (M^-1 - aa^T)_st
        const double w = (dl[m] * dl[64 + nn]) * w0;                // (D M^-1 D - uu^T)_st
        const double d0 = uQ[0 * 128 + m] - uQ[0 * 128 + 64 + nn];
        const double d1 = uQ[1 * 128 + m] - uQ[1 * 128 + 64 + nn];
        const double d2 = uQ[2 * 128 + m] - uQ[2 * 128 + 64 + nn];
        const double Q = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double e = exp(-Q);
        const double K = sf2 * ((1.0 + Q) * e);
        const double q0 = uq[0 * 128 + m] - uq[0 * 128 + 64 + nn];
        const double q1 = uq[1 * 128 + m] - uq[1 * 128 + 64 + nn];
        const double q2 = uq[2 * 128 + m] - uq[2 * 128 + 64 + nn];
        s[0] += wgt * (w * (sf2 * ((q0 * q0) * e)));
        s[1] += wgt * (w * (sf2 * ((q1 * q1) * e)));
        s[2] += wgt * (w * (sf2 * ((q2 * q2) * e)));
        s[3] += wgt * (w * (2.0 * K));
        if (a == b) s[4] += w0;
      }
  block_sum<5, 4>(s, red);
  if (t == 0) {
    double* pp = c.part + OI_PART_GRAD(0) + 5 * (size_t)tile;
    for (int q = 0; q < 5; ++q) pp[q] = s[q];
  }
}

__global__ __launch_bounds__(256) void k_lauum_grad1(const OiCell* __restrict__ cells,
                                                    const int32_t* __restrict__ list, int gx,
                                                    int ncell) {
  __shared__ __attribute__((aligned(16))) double lds[GEMM1_LDS];
  int ci, tile;
  if (!xcd_cell_slot(gx, ncell, ci, tile)) return;
  lauum_tile(cells[list[ci]], tile, lds);
}

// ---------------------------------------------------------- k_finalize
// nlZ = r.alpha/2 + sum log diag L + n log(2 pi)/2 (GPR:128); dnlZ (GPR:131-138)
__device__ __forceinline__ void finalize_cell(const OiCell& c) {
  __shared__ double red[4 * 7];
  const int t = threadIdx.x, T = c.T, ntile = T * (T + 1) / 2;
  // the round's status rides home in the result row (one D2H copy per round)
  if (t == 0) c.out[OI_OUT_STATUS] = (double)*c.status;
  if (c.mode == OI_MODE_PREDICT) {
    // GPR:178-182 from the forward substitution run inside the factorisation:
    // z = L^-1 r, v = L^-1 k*: k*^T K^-1 r = v.z, k*^T K^-1 k* = v.v, r^T K^-1 r = z.z
    if (*c.status != OI_OK) {
      if (t < 3) c.out[t] = NAN;
      return;
    }
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = t; k < T; k += 256) {
      const double* pp = c.part + OI_PART_PRED(ntile, T) + 3 * k;
      p[0] += pp[0];
      p[1] += pp[1];
      p[2] += pp[2];
      p[3] += c.part[OI_PART_LOGDET(ntile, T) + k];
    }
    block_sum<4, 4>(p, red);
    if (t == 0) {
      const double sf2 = c.hyp[3], sn2 = c.hyp[4], nm = (double)(c.n_obs - c.n);
      c.out[0] = c.mean + p[1];
      c.out[1] = sqrt(sf2 - p[2]);
      // the duplicate-site terms only where sites repeat (nm > 0): without
      // repeats they are exact zeros, and at sn2 = 0 (exp underflow, GPR:122)
      // 0 / 0 and 0 * log 0 would turn the reference's finite lZ into NaN
      if (nm > 0.0)
        c.out[2] = ((-(p[0] + c.ssw / sn2)) / 2 - (p[3] + (nm / 2) * log(sn2))) - (c.n_obs * LOG2PI) / 2;
      else
        c.out[2] = ((-p[0]) / 2 - p[3]) - (c.n_obs * LOG2PI) / 2;
    }
    return;
  }
  const int nslot = ntile;
  if (*c.status != OI_OK) {
    if (t < 7) c.out[t] = INFINITY;
    return;
  }
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int x = t; x < nslot; x += 256)
    for (int q = 0; q < 5; ++q) v[q] += c.part[OI_PART_GRAD(ntile) + 5 * x + q];
  for (int k = t; k < T; k += 256) {
    v[5] += c.part[OI_PART_PRED(ntile, T) + 3 * k];  // r^T alpha = z^T z, z = L^-1 r
    v[6] += c.part[OI_PART_LOGDET(ntile, T) + k];
  }
  block_sum<7, 4>(v, red);
  if (t == 0) {
    // site form (oi_device.h): r^T alpha = SSW/sn2 + v^T M^-1 v,
    // sum log diag L = log det M / 2 + (n - m)/2 log sn2, tr Q += (n - m)/sn2 - SSW/sn2^2
    const double quad = v[5], logdet = v[6], sn2 = c.hyp[4];
    const double nm = (double)(c.n_obs - c.n);
    // (n - m) and SSW terms only where sites repeat: without repeats they are
    // exact zeros, and at sn2 = 0 (exp underflow of the CG's trial point,
    // GPR:122) 0 / 0 and 0 * log 0 would give NaN where the reference's nlZ and
    // sn2 tr Q (= 0) are finite
    if (nm > 0.0)
      c.out[0] = ((quad + c.ssw / sn2) / 2 + (logdet + (nm / 2) * log(sn2))) + (c.n_obs * LOG2PI) / 2;
    else
      c.out[0] = (quad / 2 + logdet) + (c.n_obs * LOG2PI) / 2;
    c.out[1] = v[0] / 2;
    c.out[2] = v[1] / 2;
    c.out[3] = v[2] / 2;
    c.out[4] = v[3] / 2;
    c.out[5] = nm > 0.0 ? sn2 * ((v[4] + nm / sn2) - c.ssw / (sn2 * sn2)) : sn2 * v[4];
    c.out[6] = 0.0;
  }
}

// The result rows live in fine-grained pinned host memory (no D2H copy per
// round).  With `flag` set, the workgroup that finishes last stores `seq` to
// the group's host flag after every row has reached host memory, and the host
// spins on that word instead of a stream synchronise (config 1's lone cell
// waits for ~90 of these round trips: 7 us spinning vs 12 us synchronising,
// + 3 us for the copy, tools/sync_probe.hip).
__global__ __launch_bounds__(256) void k_finalize(const OiCell* __restrict__ cells,
                                                  const int32_t* __restrict__ list, unsigned* done,
                                                  unsigned long long* flag, unsigned long long seq,
                                                  int ncell) {
  finalize_cell(cells[list[blockIdx.x]]);
  if (flag == nullptr) return;
  __threadfence_system();  // this thread's result stores are in host memory
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(done, 1u) == (unsigned)(ncell - 1)) {
    *done = 0u;  // for the group's next round (stream order)
    __threadfence_system();
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ------------------------------------------------------------- k_dedup
// Distinct observation sites of each cell (oi_device.h, "Duplicate sites"),
// one workgroup per cell, once per submitted batch.  Site s = the s-th first
// occurrence in observation order; prev[a] = the latest earlier observation
// with bitwise-equal (x, y, t), nxt the reverse link, so every site's
// observations are walked in observation order: fixed-order sums, results
// independent of the batch.  Coordinates are staged in LDS for n <= 4096
// (36 B per observation with the links), read from global memory above.
#define DEDUP_LDS_N 4096
#define DEDUP_MAX_N 13000  // 8 B x 13000 <= 36 B x 4096
__global__ __launch_bounds__(256) void k_dedup(const double* __restrict__ xyt,
                                               const double* __restrict__ r,
                                               const int64_t* __restrict__ offs, int nodup,
                                               double* __restrict__ sites, double* __restrict__ v,
                                               double* __restrict__ dw, int32_t* __restrict__ mcount,
                                               double* __restrict__ ssw) {
  extern __shared__ double sh[];
  __shared__ int scan[256];
  __shared__ double red[4];
  const int c = blockIdx.x, t = threadIdx.x;
  const int64_t a0 = offs[c];
  const int n = (int)(offs[c + 1] - a0);
  const double* X = xyt + 3 * a0;
  const double* R = r + a0;
  const bool single = nodup || n > DEDUP_MAX_N;  // every observation its own site
  const bool in_lds = !single && n <= DEDUP_LDS_N;
  double* cx = sh;
  double* cy = sh + n;
  double* ct = sh + 2 * n;
  int* prev = (int*)(sh + (in_lds ? 3 * n : 0));
  int* nxt = prev + n;
  if (in_lds)
    for (int b = t; b < n; b += 256) {
      cx[b] = X[3 * b];
      cy[b] = X[3 * b + 1];
      ct[b] = X[3 * b + 2];
    }
  if (!single)
    for (int a = t; a < n; a += 256) nxt[a] = -1;
  __syncthreads();
  if (!single) {
    for (int a = t; a < n; a += 256) {
      int p = -1;
      if (in_lds) {
        const double xa = cx[a], ya = cy[a], ta = ct[a];
        for (int b = a - 1; b >= 0; --b)
          if (cx[b] == xa && cy[b] == ya && ct[b] == ta) {
            p = b;
            break;
          }
      } else {
        const double xa = X[3 * a], ya = X[3 * a + 1], ta = X[3 * a + 2];
        for (int b = a - 1; b >= 0; --b)
          if (X[3 * b] == xa && X[3 * b + 1] == ya && X[3 * b + 2] == ta) {
            p = b;
            break;
          }
      }
      prev[a] = p;
    }
    __syncthreads();
    for (int a = t; a < n; a += 256)
      if (prev[a] >= 0) nxt[prev[a]] = a;
  }
  // exclusive scan of first-occurrence flags over contiguous segments
  const int seg = (n + 255) / 256, s0 = min(n, t * seg), s1 = min(n, s0 + seg);
  int cnt = 0;
  for (int a = s0; a < s1; ++a) cnt += (single || prev[a] < 0) ? 1 : 0;
  scan[t] = cnt;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int q = 0; q < 256; ++q) {
      const int x = scan[q];
      scan[q] = acc;
      acc += x;
    }
    mcount[c] = acc;
  }
  __syncthreads();
  int s = scan[t];
  double part = 0.0;
  for (int a = s0; a < s1; ++a) {
    if (!(single || prev[a] < 0)) continue;
    double rs = 0.0, cntd = 0.0;
    if (single) {
      rs = R[a];
      cntd = 1.0;
    } else {
      for (int b = a; b >= 0; b = nxt[b]) {
        rs += R[b];
        cntd += 1.0;
      }
      const double rbar = rs / cntd;
      for (int b = a; b >= 0; b = nxt[b]) {
        const double e = R[b] - rbar;
        part += e * e;
      }
    }
    const double d = sqrt(cntd);
    const int64_t o = a0 + s;
    sites[3 * o] = X[3 * a];
    sites[3 * o + 1] = X[3 * a + 1];
    sites[3 * o + 2] = X[3 * a + 2];
    v[o] = rs / d;
    dw[o] = d;
    ++s;
  }
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_down(part, o, 64);
  if ((t & 63) == 0) red[t >> 6] = part;
  __syncthreads();
  if (t == 0) ssw[c] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" int oi_launch_dedup(const double* xyt, const double* r, const int64_t* offs, int ncell,
                               int maxn, int nodup, double* sites, double* v, double* dw,
                               int32_t* mcount, double* ssw, void* stream) {
  if (ncell <= 0) return 0;
  // LDS: coordinates + links (36 B per observation) for n <= DEDUP_LDS_N,
  // links only (8 B) above; cells beyond DEDUP_MAX_N run without deduplication
  size_t lds = 0;
  if (!nodup && maxn > 0)
    lds = maxn <= DEDUP_LDS_N ? (size_t)36 * maxn
                              : (size_t)36 * DEDUP_LDS_N;  // >= 8 * DEDUP_MAX_N
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)k_dedup, hipFuncAttributeMaxDynamicSharedMemorySize,
                              36 * DEDUP_LDS_N);
    attr = true;
  }
  hipLaunchKernelGGL(k_dedup, dim3(ncell), dim3(256), lds, (hipStream_t)stream, xyt, r, offs, nodup,
                     sites, v, dw, mcount, ssw);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------- k_residual
__global__ void k_residual(const double* __restrict__ y, const double* __restrict__ mX,
                           double mean, double* __restrict__ r, int64_t N) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a < N) r[a] = y[a] - (mX ? mX[a] : 1.0 * mean);
}

// ------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }
static inline int ret() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static inline unsigned grid1(int gx, int ncell) { return (unsigned)gx * (unsigned)((ncell + 7) & ~7); }

// sizeof(OiCell) as compiled, for the ctypes mirror of tests/dense_ref.py
extern "C" int oi_test_sizeof_cell(void) { return (int)sizeof(OiCell); }

extern "C" int oi_launch_diag_factor(const OiCell* cells, const int32_t* list, int ncell, int j,
                                     void* stream) {
  if (ncell <= 0) return 0;
  hipLaunchKernelGGL(k_diag_factor4w, dim3(ncell), dim3(256), 0, S(stream), cells, list, j);
  return ret();
}

extern "C" int oi_launch_chol_panel(const OiCell* cells, const int32_t* list, int ncell, int maxT,
                                    int j, int with_trtri, int fuse_diag, void* stream) {
  if (j < 1) return -1;  // the kernel streams pair k = j - 1
  const int gx = (maxT - 1 - j) + (with_trtri ? j : 0);
  if (ncell <= 0 || gx <= 0) return 0;
  const dim3 g(grid1(gx, ncell));
  auto k = j == 1 ? (fuse_diag ? k_chol_panel<true, true> : k_chol_panel<true, false>)
                  : (fuse_diag ? k_chol_panel<false, true> : k_chol_panel<false, false>);
  hipLaunchKernelGGL(k, g, dim3(256), 0, S(stream), cells, list, j, gx, ncell);
  return ret();
}

extern "C" int oi_launch_panel_even(const OiCell* cells, const int32_t* list, int ncell, int maxT,
                                    int j, int with_trtri, int fuse_diag, void* stream) {
  const int gx = (maxT - 1 - j) + (with_trtri ? j : 0);
  if (ncell <= 0 || gx <= 0) return 0;
  if (fuse_diag)
    hipLaunchKernelGGL(k_panel_even<true>, dim3(grid1(gx, ncell)), dim3(GEMM_THREADS), 0, S(stream), cells, list, j,
                       gx, ncell);
  else
    hipLaunchKernelGGL(k_panel_even<false>, dim3(grid1(gx, ncell)), dim3(GEMM_THREADS), 0, S(stream), cells, list, j,
                       gx, ncell);
  return ret();
}

extern "C" int oi_launch_panel4(const OiCell* cells, const int32_t* list, int ncell, int maxT, int j,
                                int with_trtri, int fuse_diag, void* stream) {
  const int gx = nslot4_factor(maxT, j) + (with_trtri ? j / 2 : 0);
  if (ncell <= 0 || gx <= 0) return 0;
  hipLaunchKernelGGL(k_panel4, dim3(grid1(gx, ncell)), dim3(GEMM_THREADS), 0, S(stream), cells, list, j, gx,
                     ncell, fuse_diag);
  return ret();
}

extern "C" int oi_launch_lauum_grad(const OiCell* cells, const int32_t* list, int ncell, int maxT,
                                    void* stream) {
  if (ncell <= 0 || maxT <= 0) return 0;
  const int gx = maxT * (maxT + 1) / 2;  // one 64x64 tile per 256-thread workgroup
  hipLaunchKernelGGL(k_lauum_grad1, dim3(grid1(gx, ncell)), dim3(256), 0, S(stream), cells, list, gx, ncell);
  return ret();
}

extern "C" int oi_launch_finalize(const OiCell* cells, const int32_t* list, int ncell, unsigned* done,
                                  unsigned long long* flag, unsigned long long seq, void* stream) {
  if (ncell <= 0) return 0;
  hipLaunchKernelGGL(k_finalize, dim3(ncell), dim3(256), 0, S(stream), cells, list, done, flag, seq, ncell);
  return ret();
}

extern "C" int oi_launch_residual(const double* y, const double* mX, double mean, double* r,
                                  int64_t N, void* stream) {
  if (N <= 0) return 0;
  hipLaunchKernelGGL(k_residual, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, S(stream), y, mX,
                     mean, r, N);
  return ret();
}
