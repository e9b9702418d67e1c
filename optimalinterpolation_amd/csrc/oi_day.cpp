// C ABI of the day-level device steps (include/oi.h, "day pipeline"):
//   oi_smooth_fields  <- smooth() GPR_CS2S3.py:65-76 (called 5x, GPR:303-307)
//   oi_ball_query     <- X_tree.query_ball_point(X[index], r) GPR:159, batched
//   oi_gather_rows    <- inputs / outputs gathering GPR:160-161, batched
// Kernels: oi_day.hip.  Host mode copies through the library; with
// opts->device_inputs = 1 the array arguments are device pointers (HBM
// resident) and nothing crosses PCIe except the small host-side arrays named
// in oi.h (vmax, kern, offs).  Every device buffer lives for one call and is
// stream-ordered (DevBuf(bytes, stream)): a radius query issued between a
// session's rounds (bench.py's timed day) must not drain the rounds in flight
// on the session's streams, as a synchronous hipFree would.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/oi.h"
#include "oi_host.h"

extern "C" {
int oi_launch_smooth(const double* in, double* out, int nf, int64_t ny, int64_t nx,
                     const double* vmax, const double* kern, int ks, const double* mask,
                     void* stream);
int oi_launch_ball_count(const double* pts, int64_t M, double* bbox, const double* q, int64_t Q,
                         double r2, int64_t* counts, void* stream);
int oi_launch_ball_fill(const double* pts, int64_t M, const double* bbox, const double* q,
                        int64_t Q, double r2, const int64_t* offs, int64_t* idx, void* stream);
int oi_launch_gather_rows(const double* xt, const double* yt, const double* tt, const double* zt,
                          const int64_t* idx, int64_t N, int64_t M, double* xyt, double* zout,
                          void* stream);
}

namespace {

// numpy's pairwise_sum of a[0 .. n): leaves of <= 128 elements with 8
// accumulators, halves rounded down to multiples of 8.  n <= 8192 is one of
// np.sum's iterator buffers, so this is arr.sum() for the ks*ks <= 4225 kernel
// entries (oracle/day_oracle.py::numpy_pairwise_sum is the restatement).
double np_pairwise_sum(const double* a, size_t n) {
  if (n < 8) {
    double res = 0.0;
    for (size_t i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    size_t i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  size_t n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// astropy Gaussian2DKernel(x_stddev=std): Gaussian2D(amplitude 1/(2 pi std^2),
// theta 0) sampled at integer offsets, size 8*std rounded up to odd, / sum, the
// sum in numpy's order (arr.sum()).  What is left against numpy's array is
// libm's exp against numpy's: entries within 4 ulp (tests/test_day_ref.py).
std::vector<double> gaussian_kernel(double std_, int& ks) {
  int i = (int)std::ceil(8.0 * std_);
  ks = (i % 2 == 0) ? i + 1 : i;
  const int h = (ks - 1) / 2;
  const double a = 0.5 * (1.0 / (std_ * std_)), amp = 1.0 / (2 * M_PI * std_ * std_);
  std::vector<double> k((size_t)ks * ks);
  for (int y = -h; y <= h; ++y)
    for (int x = -h; x <= h; ++x)
      k[(size_t)(y + h) * ks + (x + h)] =
          amp * std::exp(-((a * (double)(x * x)) + (a * (double)(y * y))));
  const double s = np_pairwise_sum(k.data(), k.size());
  for (double& v : k) v /= s;
  return k;
}

// the std values oi_smooth_fields(kern = NULL) accepts (NaN refused)
bool std_ok(double std_) { return std_ > 0.0 && std_ <= 8.0; }

}  // namespace

extern "C" {

int oi_smooth_fields(const double* fields, int32_t nf, int64_t ny, int64_t nx, const double* vmax,
                     const double* mask, double std_, const double* kern, int32_t ks, double* out,
                     const oi_options* opts) {
  if (nf < 0 || ny < 0 || nx < 0) return oi_set_last_error(OI_E_ARG, "negative size");
  if (nf == 0 || ny == 0 || nx == 0) return 0;
  if (!fields || !vmax || !mask || !out) return oi_set_last_error(OI_E_ARG, "null pointer");
  std::vector<double> kv;
  if (kern) {
    if (ks <= 0 || ks % 2 == 0 || ks > 65) return oi_set_last_error(OI_E_ARG, "kernel size must be odd, <= 65");
    kv.assign(kern, kern + (size_t)ks * ks);
  } else {
    if (!std_ok(std_)) return oi_set_last_error(OI_E_ARG, "std must be in (0, 8]");
    kv = gaussian_kernel(std_, ks);
  }
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  hipStream_t st = (hipStream_t)o.stream;
  return oi_guarded([&] {
    const size_t npix = (size_t)ny * nx, fb = (size_t)nf * npix * 8;
    DevBuf dk(kv.size() * 8, st), dv((size_t)nf * 8, st);
    HC(hipMemcpyAsync(dk.p, kv.data(), kv.size() * 8, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(dv.p, vmax, (size_t)nf * 8, hipMemcpyHostToDevice, st));
    if (o.device_inputs) {
      if (oi_launch_smooth(fields, out, nf, ny, nx, dv.as<double>(), dk.as<double>(), ks, mask, st))
        throw HipErr{"smooth kernel launch failed"};
      HC(hipStreamSynchronize(st));
      return 0;
    }
    DevBuf din(fb, st), dout(fb, st), dm(npix * 8, st);
    HC(hipMemcpyAsync(din.p, fields, fb, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(dm.p, mask, npix * 8, hipMemcpyHostToDevice, st));
    if (oi_launch_smooth(din.as<double>(), dout.as<double>(), nf, ny, nx, dv.as<double>(),
                         dk.as<double>(), ks, dm.as<double>(), st))
      throw HipErr{"smooth kernel launch failed"};
    HC(hipMemcpyAsync(out, dout.p, fb, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    return 0;
  });
}

int oi_ball_query(const double* pts, int64_t M, const double* q, int64_t Q, double r,
                  int64_t* offs, int64_t* idx, int64_t cap, const oi_options* opts) {
  if (M < 0 || Q < 0 || cap < 0) return oi_set_last_error(OI_E_ARG, "negative size");
  if (!offs) return oi_set_last_error(OI_E_ARG, "null offs");
  offs[0] = 0;
  if (Q == 0) return 0;
  if (!q || (M > 0 && !pts)) return oi_set_last_error(OI_E_ARG, "null pointer");
  if (!(r >= 0.0)) return oi_set_last_error(OI_E_ARG, "radius must be >= 0");
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  hipStream_t st = (hipStream_t)o.stream;
  return oi_guarded([&] {
    const double r2 = r * r;
    const bool dev = o.device_inputs != 0;
    DevBuf dpts(dev ? 0 : (size_t)M * 16, st), dq(dev ? 0 : (size_t)Q * 16, st);
    const double* P = dev ? pts : dpts.as<double>();
    const double* Qp = dev ? q : dq.as<double>();
    if (!dev) {
      if (M) HC(hipMemcpyAsync(dpts.p, pts, (size_t)M * 16, hipMemcpyHostToDevice, st));
      HC(hipMemcpyAsync(dq.p, q, (size_t)Q * 16, hipMemcpyHostToDevice, st));
    }
    DevBuf bbox((size_t)((M + 255) / 256 + 1) * 32, st), cnt((size_t)Q * 8, st);
    if (oi_launch_ball_count(P, M, bbox.as<double>(), Qp, Q, r2, cnt.as<int64_t>(), st))
      throw HipErr{"ball count launch failed"};
    std::vector<int64_t> h((size_t)Q);
    HC(hipMemcpyAsync(h.data(), cnt.p, (size_t)Q * 8, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    for (int64_t k = 0; k < Q; ++k) offs[k + 1] = offs[k] + h[(size_t)k];
    const int64_t total = offs[Q];
    if (!idx || total > cap || total == 0) return 0;  // caller sizes idx from offs[Q]
    DevBuf doffs((size_t)(Q + 1) * 8, st);
    HC(hipMemcpyAsync(doffs.p, offs, (size_t)(Q + 1) * 8, hipMemcpyHostToDevice, st));
    DevBuf didx(dev ? 0 : (size_t)total * 8, st);
    int64_t* I = dev ? idx : didx.as<int64_t>();
    if (oi_launch_ball_fill(P, M, bbox.as<double>(), Qp, Q, r2, doffs.as<int64_t>(), I, st))
      throw HipErr{"ball fill launch failed"};
    if (!dev) HC(hipMemcpyAsync(idx, didx.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    return 0;
  });
}

int oi_gather_rows(const double* x_train, const double* y_train, const double* t_train,
                   const double* z, int64_t M, const int64_t* idx, int64_t N, double* xyt,
                   double* zout, const oi_options* opts) {
  if (N < 0 || M < 0) return oi_set_last_error(OI_E_ARG, "negative size");
  if (N == 0) return 0;
  if (!x_train || !y_train || !t_train || !z || !idx || !xyt || !zout)
    return oi_set_last_error(OI_E_ARG, "null pointer");
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  hipStream_t st = (hipStream_t)o.stream;
  return oi_guarded([&] {
    if (o.device_inputs) {
      if (oi_launch_gather_rows(x_train, y_train, t_train, z, idx, N, M, xyt, zout, st))
        throw HipErr{"gather launch failed"};
      HC(hipStreamSynchronize(st));
      return 0;
    }
    for (int64_t k = 0; k < N; ++k)
      if (idx[k] < 0 || idx[k] >= M) return oi_set_last_error(OI_E_ARG, "index out of range");
    DevBuf dx((size_t)M * 8, st), dy((size_t)M * 8, st), dt((size_t)M * 8, st), dz((size_t)M * 8, st),
        di((size_t)N * 8, st), dxyt((size_t)N * 24, st), dzo((size_t)N * 8, st);
    HC(hipMemcpyAsync(dx.p, x_train, (size_t)M * 8, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(dy.p, y_train, (size_t)M * 8, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(dt.p, t_train, (size_t)M * 8, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(dz.p, z, (size_t)M * 8, hipMemcpyHostToDevice, st));
    HC(hipMemcpyAsync(di.p, idx, (size_t)N * 8, hipMemcpyHostToDevice, st));
    if (oi_launch_gather_rows(dx.as<double>(), dy.as<double>(), dt.as<double>(), dz.as<double>(),
                              di.as<int64_t>(), N, M, dxyt.as<double>(), dzo.as<double>(), st))
      throw HipErr{"gather launch failed"};
    HC(hipMemcpyAsync(xyt, dxyt.p, (size_t)N * 24, hipMemcpyDeviceToHost, st));
    HC(hipMemcpyAsync(zout, dzo.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    return 0;
  });
}

// Test hook (not in oi.h): the kernel oi_smooth_fields(kern = NULL, std) builds.
// Returns ks and writes the ks*ks entries when cap holds them; -1 for a std
// that entry point refuses.  No GPU needed.
int32_t oi_test_gaussian_kernel(double std_, double* out, int32_t cap) {
  if (!std_ok(std_)) return -1;
  int ks = 0;
  const std::vector<double> k = gaussian_kernel(std_, ks);
  if (out && (int64_t)cap >= (int64_t)k.size()) std::memcpy(out, k.data(), k.size() * 8);
  return ks;
}

}  // extern "C"
