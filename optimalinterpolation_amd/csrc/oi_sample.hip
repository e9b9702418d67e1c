// Joint posterior draws per cell at given hypers: oi_gpr_sample.  With
// fs and cov = Kxs - v'v exactly as oi_gpr_predict_multi forms them:
//
//   C = cov + (noise ? sn2 : 0) I + jitter I = Lc Lc'
//   samples[t, s] = fs[t] + sum_u Lc[t, u] Xi[u, s]
//
// The front half and k_pm_reduce of oi_predict.hip run unchanged (oi_dense.h;
// fs and sd are bit for bit oi_gpr_predict_multi's).  k_ps_cgen writes the lower tiles of Kxs plus the
// diagonal term into a padded Ntp x Ntp buffer, Ntp = nt rounded up to 64,
// with an identity on the pad and zeros in the strict upper triangle of the
// diagonal tiles; oila::gemm (tri = 3) subtracts X[:nt] X[:nt]' and
// oila::cholesky factors in place, neither touching those zeros.  k_ps_draw
// fills the result with fs and, without the caller's Xi, writes the normals
// (Philox4x32-10, Box-Muller; ps_normal).  The cell's block of samples, row-major
// [nt x nsamp], is the column-major nsamp x nt matrix Xi' Lc', one oila::gemm
// with tri = 2 (Lc' is upper triangular) and beta = 1 on top of fs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "oi_dense.h"
#include "oi_matern.h"

#pragma clang fp contract(off)

using namespace oi_dense;

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
  const int64_t T = toffs[ncell];
  const char* missing = T > 0 && !xs ? "null xs" : T > 0 && nsamp > 0 && !samples ? "null samples" : nullptr;
  // Xi and the samples are operands of oila's as well
  if (int rc = dense_check(xyt, z, offs, toffs, ncell, hyp, status, missing, {.X = true, .C = true, .nsamp = nsamp}))
    return rc;
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    Front fr(o, xyt, z, offs, hyp, mean, false, kSampleStage, P_COUNT);
    const std::vector<int64_t> cuts = fr.plan(ncell, SAMPLE_SLACK, "sampling", [&](int64_t c) {
      return sample_cell_doubles(offs[c + 1] - offs[c], toffs[c + 1] - toffs[c], nsamp, fr.in.host);
    });
    hipStream_t st = fr.st;
    Carver& cv = fr.cv;
    std::vector<SCell> scells;
    std::vector<oila::Gemm> syrk, prod;
    std::vector<oila::Chol> cchol;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
      const int64_t c0 = cuts[q], c1 = cuts[q + 1], nc = c1 - c0, t0 = toffs[c0], tt = toffs[c1] - t0;
      const int64_t ee = tt * nsamp;
      fr.begin(c0, c1, xs + t0 * 3, tt, -1);
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
        PCell& p = fr.add(c, nt, tq, a);
        p.cov = nullptr;
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
      const PCell* dc = fr.factor("oi_gpr_sample", P_GEN, P_CHOL, P_SOLVE);
      const SCell* ds = fr.la.put(scells);
      const unsigned gz = (unsigned)nc, Tt = blocks(fr.ntmax, 64), ge = std::max(1u, blocks(emax, 256));
      fr.reduce(P_REDUCE, by_red, dc);
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
