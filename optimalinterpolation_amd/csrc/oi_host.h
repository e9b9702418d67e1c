// Host plumbing shared by every entry point of liboi.so: error reporting, the
// exception-to-code ladder, option / device set-up, the ragged-offsets
// validator, the RAII device / pinned buffers and owned stream, the workspace
// chunk planner and the per-stage event profiler.  Host code only; needs the HIP runtime, so the
// optimiser's files (cg.cpp, cg.hpp, cg_abi.cpp, task.hpp) do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
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

// The ragged offsets `name` of ncell >= 0 cells: non-null, starting at 0, every
// cell with at least min_n rows (0: merely non-decreasing).  0 or OI_E_ARG.
inline int oi_check_offs(const int64_t* offs, int64_t ncell, int64_t min_n, const char* name) {
  const std::string s(name);
  if (ncell < 0) return oi_set_last_error(OI_E_ARG, "negative ncell");
  if (!offs) return oi_set_last_error(OI_E_ARG, ("null " + s).c_str());
  if (offs[0] != 0) return oi_set_last_error(OI_E_ARG, (s + "[0] must be 0").c_str());
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t n = offs[c + 1] - offs[c];
    if (n < 0) return oi_set_last_error(OI_E_ARG, (s + " must be non-decreasing").c_str());
    if (n < min_n) return oi_set_last_error(OI_E_ARG, (s + ": every cell needs n >= 1").c_str());
  }
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
  void reserve(size_t bytes) {  // plain buffers: grow to at least `bytes`, contents dropped
    if (bytes <= n) return;
    if (p) HC(hipFree(p));
    p = nullptr;
    HC(hipMalloc(&p, bytes));
    n = bytes;
  }
  ~DevBuf() {
    if (p) (void)(async ? hipFreeAsync(p, st) : hipFree(p));
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }

 private:
  size_t n = 0;  // what reserve() holds
};

// Pinned host buffer.
struct HostBuf {
  void* p = nullptr;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  void reserve(size_t bytes, unsigned flags = hipHostMallocDefault) {
    if (bytes <= n) return;
    if (p) HC(hipHostFree(p));
    p = nullptr;
    HC(hipHostMalloc(&p, bytes, flags));
    n = bytes;
  }
  ~HostBuf() {
    if (p) (void)hipHostFree(p);
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }

 private:
  size_t n = 0;
};

// A non-blocking stream of our own; destroyed (not synchronised) with its owner.
struct OwnStream {
  hipStream_t s = nullptr;
  OwnStream() = default;
  OwnStream(const OwnStream&) = delete;
  OwnStream& operator=(const OwnStream&) = delete;
  void create() { HC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~OwnStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

// Carves 256-byte-aligned arrays of doubles out of one workspace.  A path
// writes its arrays once, as a layout function over a Carver; without a base
// the same function only counts (take returns null, off is the size), so a
// workspace's size is never a second description of it.  quantum 1 counts a
// cell's share of chunk-wide arrays, which hold the cells' parts back to back
// and are rounded once per chunk (the planner's slack).
struct Carver {
  double* base = nullptr;
  int64_t off = 0;
  int64_t quantum = 32;
  double* take(int64_t doubles) {
    double* p = base ? base + off : nullptr;
    off += up(doubles, quantum);
    return p;
  }
};

// `count` doubles of a host array into the workspace (asynchronous on st);
// null, with nothing taken, for an empty array
inline double* stage_host(Carver& cv, const double* src, int64_t count, hipStream_t st) {
  if (count <= 0) return nullptr;
  double* p = cv.take(count);
  if (p) HC(hipMemcpyAsync(p, src, count * 8, hipMemcpyHostToDevice, st));
  return p;
}

// A cell's workspace in doubles, from the path's layout on a counting Carver
// (oi_svgp_predict.hip, oi_nystrom.hip); the test hook oi_test_cell_doubles
// in oi_predict.hip hands them out with its own two.
int64_t oi_svgp_cell_doubles(int M, int64_t n, bool cov, bool host_inputs, bool elbo);
int64_t oi_nystrom_multi_cell_doubles(int64_t n, int64_t M, int64_t nt, bool cov);

// The workspace budget in doubles: opts.pool_bytes, or 60 % of the free HBM.
inline int64_t oi_workspace_budget(const oi_options& o) {
  if (o.pool_bytes > 0) return o.pool_bytes / 8;
  size_t fr = 0, tot = 0;
  HC(hipMemGetInfo(&fr, &tot));
  return (int64_t)((double)fr * 0.6) / 8;
}

// Chunks of consecutive cells whose workspace (cell_doubles(c) each, plus
// `slack` per chunk) fits `budget` doubles, at most opts.max_pool (when set)
// and `max_cells` cells each: chunk q is cells cuts[q] .. cuts[q + 1], and the
// largest chunk needs `biggest` doubles.  `what` names the workspace in the
// OI_E_NOMEM text of a cell that fits no chunk.
struct ChunkPlan {
  std::vector<int64_t> cuts;
  int64_t biggest = 0;
};
template <class F>
ChunkPlan plan_chunks(int64_t ncell, const oi_options& o, int64_t slack, int64_t max_cells, const char* what,
                      F&& cell_doubles) {
  const int64_t budget = oi_workspace_budget(o);
  const int64_t cap = o.max_pool > 0 ? std::min<int64_t>(o.max_pool, max_cells) : max_cells;
  ChunkPlan p;
  p.cuts.push_back(0);
  int64_t cur = slack;
  for (int64_t c = 0; c < ncell; ++c) {
    const int64_t d = cell_doubles(c);
    if (slack + d > budget) throw NoMem{std::string("a cell's ") + what + " workspace does not fit pool_bytes"};
    if (cur + d > budget || c - p.cuts.back() >= cap) {
      p.cuts.push_back(c);
      cur = slack;
    }
    cur += d;
    p.biggest = std::max(p.biggest, cur);
  }
  p.cuts.push_back(ncell);
  return p;
}

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
