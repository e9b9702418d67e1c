// Host plumbing shared by every entry point of liboi.so: error reporting, the
// exception-to-code ladder, option / device set-up, the RAII device buffer and
// the per-stage event profiler.  Host code only; needs the HIP runtime, so the
// optimiser's files (cg.cpp, cg.hpp, cg_abi.cpp, task.hpp) do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/oi.h"

extern "C" {
// defined in oi_engine.cpp: the thread's last error text (returns `code`), and
// per-stage timings summed by name into oi_profile_json
int oi_set_last_error(int code, const char* msg);
void oi_profile_add(const char* name, int64_t launches, double ms, double flops, double bytes);
}

struct HipErr {  // a HIP call failed (or a launch could not be made): OI_E_HIP
  std::string msg;
};
struct NoMem {  // the device workspace cannot hold the request: OI_E_NOMEM
  std::string msg;
};

#define HC(expr)                                                                           \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) throw HipErr{std::string(#expr) + ": " + hipGetErrorString(e_)}; \
  } while (0)
#define KCHK() HC(hipGetLastError())

// Runs f and returns its value; an exception becomes its OI_E_* code with the
// text left for oi_last_error().
template <class F>
auto oi_guarded(F&& f) -> decltype(f()) {
  try {
    return f();
  } catch (const HipErr& e) {
    return oi_set_last_error(OI_E_HIP, e.msg.c_str());
  } catch (const NoMem& e) {
    return oi_set_last_error(OI_E_NOMEM, e.msg.c_str());
  } catch (const std::bad_alloc&) {
    return oi_set_last_error(OI_E_NOMEM, "host allocation failed");
  }
}

// the defaults overlaid with the caller's options
inline oi_options oi_resolve(const oi_options* opts) {
  oi_options o;
  oi_options_default(&o);
  if (opts) o = *opts;
  return o;
}

// makes o.device the calling thread's device; 0 or an error code
inline int oi_select_device(const oi_options& o) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return oi_set_last_error(OI_E_NODEV, "no HIP device available");
  if (o.device < 0 || o.device >= ndev) return oi_set_last_error(OI_E_ARG, "bad device ordinal");
  if (hipSetDevice(o.device) != hipSuccess) return oi_set_last_error(OI_E_HIP, "hipSetDevice failed");
  return 0;
}

inline unsigned blocks(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }
inline int64_t up(int64_t v, int64_t q) { return (v + q - 1) / q * q; }

// Device buffer.  Plain (hipMalloc / hipFree), or stream-ordered
// (hipMallocAsync / hipFreeAsync on the given stream) where freeing must not
// wait for the whole device: hipFree synchronises it, which would drain the
// rounds a session has in flight on its other streams.
struct DevBuf {
  void* p = nullptr;
  hipStream_t st = nullptr;
  bool async = false;
  DevBuf() = default;
  explicit DevBuf(size_t bytes) { alloc(bytes); }
  DevBuf(size_t bytes, hipStream_t s) { alloc_async(bytes, s); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void alloc(size_t bytes) {
    if (bytes) HC(hipMalloc(&p, bytes));
  }
  void alloc_async(size_t bytes, hipStream_t s) {
    st = s;
    async = true;
    if (bytes) HC(hipMallocAsync(&p, bytes, s));
  }
  ~DevBuf() {
    if (p) (void)(async ? hipFreeAsync(p, st) : hipFree(p));
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// opts.profile: HIP events around each stage on one stream, summed per stage
// (names[kind]) into oi_profile_json with the stage's algorithmic flops / bytes.
struct StageTimer {
  bool on = false;
  hipStream_t st = nullptr;
  StageTimer(const char* const* names, int count) : names_(names), count_(count) {}
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  void begin(int kind, double flops, double bytes) {
    if (!on) return;
    kind_.push_back(kind);
    fl_.push_back(flops);
    by_.push_back(bytes);
    rec();
  }
  void end() {
    if (on) rec();
  }
  void flush() {  // after the stream has been synchronised
    if (!on) return;
    std::vector<double> ms(count_, 0.0), f(count_, 0.0), b(count_, 0.0);
    std::vector<int64_t> n(count_, 0);
    for (size_t q = 0; q < kind_.size(); ++q) {
      float t = 0.f;
      HC(hipEventElapsedTime(&t, ev_[2 * q], ev_[2 * q + 1]));
      ms[kind_[q]] += t;
      f[kind_[q]] += fl_[q];
      b[kind_[q]] += by_[q];
      n[kind_[q]] += 1;
    }
    for (int k = 0; k < count_; ++k)
      if (n[k]) oi_profile_add(names_[k], n[k], ms[k], f[k], b[k]);
    drop();
    kind_.clear();
    fl_.clear();
    by_.clear();
  }
  ~StageTimer() { drop(); }

 private:
  void rec() {
    hipEvent_t e;
    HC(hipEventCreate(&e));
    ev_.push_back(e);
    HC(hipEventRecord(e, st));
  }
  void drop() {
    for (auto e : ev_) (void)hipEventDestroy(e);
    ev_.clear();
  }
  const char* const* names_;
  int count_;
  std::vector<hipEvent_t> ev_;
  std::vector<int> kind_;
  std::vector<double> fl_, by_;
};
