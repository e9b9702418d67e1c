// What the Nystrom entry points share on the host (oi_nystrom.hip: objective,
// prediction, many targets per cell; oi_nystrom_fit.hip: the fit, one-shot and
// as a session): the validated batch and its device copy, the cell table's
// row, the environment knobs, the layouts of a Runner's two workspaces and of
// the many-target scratch, and the Runner.  Host declarations only; the
// kernels and the Runner's methods are in oi_nystrom.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "oi_host.h"
#include "oi_linalg.h"

namespace oi_nys {

// opts.profile: HIP events around each stage of each cell, summed per stage
// into oi_profile_json (algorithmic flops / bytes per stage alongside)
enum { S_BUILD, S_EIGH, S_EIGH_VEC, S_EIGH_ORTH, S_EIGH_BACK, S_PANEL, S_KI, S_APPLY, S_LOGDET, S_GRAD,
       S_PRED, S_PREDM, S_COUNT };
extern const char* const kStage[S_COUNT];
// per-cell device results: [r.A, sum log diag(L) + sum log st / 2, g0..g4 raw
// sums, k*.A, |k*|^2, |W k*|^2]
constexpr int NRES = 10;
// per-cell infos: [eigh, potrf(B)] (LAPACK's info semantics)
constexpr int NINFO = 2;

// Validated ragged batch + the device-side state of one liboi call.
struct Batch {
  const double* xyt;
  const double* y;
  const int64_t* offs;
  int64_t ncell;
  const int64_t* sel;
  const int64_t* soffs;
  int64_t nmax = 0, mmax = 0;
};
int check_batch(Batch& b);
// the LINEAR hypers of ncell cells (5 each)
int check_hypers(const double* hyp, int64_t ncell);

// One cell's inputs on the device: the row of the cell table a Runner reads.
struct CellSrc {
  const double* x;     // n x 3
  const double* y;     // n (outputs minus the prior mean, as NB1 passes them)
  const int64_t* sel;  // M inducing rows, 0-based within the cell
  const double* xs;    // 3 (prediction target) or null
  int64_t n, M;
};

// Outcome of one cell at one hyper point (host side).
struct CellOut {
  double nlz, grad[5], fs, sd, sprior;
  int status;
};

// Device copy of one validated batch (inputs when they came from the host,
// inducing rows, targets) and its rows of the cell table.
// Allocated and filled on stream `st` (stream-ordered; the constructor
// returns once the copies are done) and freed on it: a session orders `st`
// after every group's last use before dropping a batch.
struct BatchDev {
  DevBuf hx, hy, dsel, dxs;
  std::vector<CellSrc> rows;
  BatchDev(const Batch& b, const double* xs, bool device_inputs, hipStream_t st);
};

// Many-target prediction of one call (oi_nystrom_predict_multi): the targets
// and outputs of every cell on the device, and the scratch of one cell (sized
// for the call's largest, reused from cell to cell in stream order).
struct MultiDev {
  const double* xs = nullptr;      // [T x 3] targets (device)
  const int64_t* toffs = nullptr;  // [ncell + 1] (host): cell c owns rows toffs[c] .. toffs[c+1]-1
  const int64_t* coffs = nullptr;  // [ncell + 1] (host): cell c's covariance starts at coffs[c]
  double* fs = nullptr;            // [T]
  double* var = nullptr;           // [T] diag(Kxs - err)
  double* cov = nullptr;           // [coffs[ncell]] or null
  double *ts = nullptr, *KxT = nullptr, *VT = nullptr, *Kp = nullptr, *Vp = nullptr;

  // One cell's scratch in doubles, array by array: scaled targets, Kxsx'
  // (nt x n), V' (nt x M) and their zero-padded k-major tiles.
  struct Scratch {
    int64_t ts = 0, KxT = 0, VT = 0, Kp = 0, Vp = 0;
    void grow(int64_t n, int64_t M, int64_t nt) {
      const int64_t Tt = (nt + 63) / 64;
      ts = std::max(ts, 3 * nt), KxT = std::max(KxT, nt * n), VT = std::max(VT, nt * M);
      Kp = std::max(Kp, (n + 63) / 64 * Tt * 4096), Vp = std::max(Vp, (M + 63) / 64 * Tt * 4096);
    }
  };
  // The workspace, described once: the call's T targets and outputs (covd
  // covariance elements, none if negative), then one cell's scratch.  On a
  // counting Carver: the size of the call, or (T = 0) of one cell's scratch.
  void layout(Carver& cv, int64_t T, int64_t covd, const Scratch& s, const double* xs_host, hipStream_t st) {
    xs = stage_host(cv, xs_host, 3 * T, st);
    fs = cv.take(T);
    var = cv.take(T);
    cov = covd >= 0 ? cv.take(covd) : nullptr;
    ts = cv.take(s.ts);
    KxT = cv.take(s.KxT);
    VT = cv.take(s.VT);
    Kp = cv.take(s.Kp);
    Vp = cv.take(s.Vp);
  }
  static int64_t doubles(int64_t T, int64_t covd, const Scratch& s) {
    Carver cv;
    MultiDev().layout(cv, T, covd, s, nullptr, nullptr);
    return cv.off;
  }
};

// The path's environment knobs, read once: by each Runner when it is built, by
// the one-shot fit per call and by a session when it is created.
struct Knobs {
  // objective pass: fused MFMA kernel (default) or, with OI_NYS_FUSED=0, the
  // n x n product forming Ki (oila::gemm) followed by k_nys_grad
  bool fused = true;
  // padding quantum (OI_NYS_PAD, default 32; 0 = no padding): K_mm and B of a
  // cell are factored as diag(A, d I) of size Mp = M rounded up (the slot
  // strides of the chunk arrays; results equal the unpadded path to rounding)
  int padq = 32;
  // the fit's groups of cells (OI_NYS_GROUPS), each with a stream and Runner of its own
  int groups = 2;
  // resident fitting cells per group of a session (OI_NYS_CAP): the batched
  // eigensolver's per-column launches cost the same for 32 or 64 matrices, so a
  // bigger chunk amortises them -- 5.46 / 6.69 / 6.63 cells/s at 32 / 64 / 128
  // (--workload nystrom, one box, profiles/r05/nystrom_cap/)
  int64_t cap = 64;
  Knobs() {
    if (const char* e = getenv("OI_NYS_FUSED")) fused = atoi(e) != 0;
    if (const char* e = getenv("OI_NYS_PAD")) padq = std::max(0, atoi(e));
    if (const char* e = getenv("OI_NYS_GROUPS")) groups = std::max(1, atoi(e));
    if (const char* e = getenv("OI_NYS_CAP")) cap = std::max(1, atoi(e));
  }
};
inline int64_t padded(int64_t M, int padq) { return padq > 0 ? up(M, padq) : M; }

// A Runner's device memory is two workspaces, each described once by a layout
// function (on a counting Carver: its size).
//
// Fixed: what one Runner owns for its lifetime -- the results and infos of an
// evaluation's cells (at most cap) and phase 5's per-cell scratch, reused from
// cell to cell in stream order.
struct Fixed {
  double* res;           // [cap x NRES]
  int32_t* info;         // [cap x NINFO]
  double *Av, *tv;       // A (n), W r (M)
  double *Wp, *Ki;       // objective: W' packed (fused) or Ki (n x n), the other null
  double* part;          // objective: the tiles' partial sums
  double *ks, *kv, *xsc; // predict: k*, W k*, the scaled target
  void layout(Carver& cv, int64_t nmax, int64_t mmax, int64_t cap, bool obj, bool pred, bool fused) {
    const int64_t nt = blocks(nmax, 64);
    res = cv.take(cap * NRES);
    info = reinterpret_cast<int32_t*>(cv.take((cap * NINFO + 1) / 2));
    Av = cv.take(nmax);
    tv = cv.take(mmax);
    Wp = obj && fused ? cv.take(blocks(mmax, 64) * nt * 4096) : nullptr;
    Ki = obj && !fused ? cv.take(nmax * nmax) : nullptr;
    part = obj ? cv.take(5 * nt * nt) : nullptr;
    ks = pred ? cv.take(nmax) : nullptr;
    kv = pred ? cv.take(mmax) : nullptr;
    xsc = pred ? cv.take(3) : nullptr;
  }
  static int64_t doubles(int64_t nmax, int64_t mmax, int64_t cap, bool obj, bool pred, bool fused) {
    Carver cv;
    Fixed().layout(cv, nmax, mmax, cap, obj, pred, fused);
    return cv.off;
  }
};

// Slots: the per-slot state of a chunk of ch cells (scaled inputs, K_mm -> u,
// s, st, C -> W', B -> L, the eigensolver's workspace, the Cholesky's
// diagonal-block inverses, K_nm, U1 -> ut), each array ch slots of one stride;
// Mp is the padded mmax.
struct Slots {
  struct Arr {
    double* p = nullptr;
    int64_t stride = 0;
    double* slot(int64_t q) const { return p + q * stride; }
  };
  Arr sc, sq, Kmm, eval, stl, C, B, EW, Dinv, Knm, U1;
  void layout(Carver& cv, int64_t ch, int64_t nmax, int64_t Mp) {
    auto arr = [&](int64_t stride) { return Arr{cv.take(ch * stride), stride}; };
    sc = arr(3 * nmax);
    sq = arr(3 * nmax);
    Kmm = arr(Mp * Mp);
    eval = arr(Mp);
    stl = arr(Mp);
    C = arr(nmax * Mp);
    B = arr(Mp * Mp);
    EW = arr((int64_t)oila::eigh_workspace_doubles((int)Mp));
    Dinv = arr((Mp + 63) / 64 * 4096);
    Knm = arr(nmax * Mp);
    U1 = arr(nmax * Mp);
  }
  // quantum 1 with ch = 1: one slot's share, what sizes a chunk
  static int64_t doubles(int64_t ch, int64_t nmax, int64_t Mp, int64_t quantum = 32) {
    Carver cv{nullptr, 0, quantum};
    Slots().layout(cv, ch, nmax, Mp);
    return cv.off;
  }
};

// Evaluates any subset of a validated batch's cells at given LINEAR hypers.
//
// The eigensolver runs one workgroup per matrix and the blocked Cholesky one
// launch sequence for many matrices, so a run is phase-major over CHUNKS of
// cells (sorted by M): (1) K_mm of every cell, (2) one batched eigh per
// equal-padded-M group, (3) the n x M panels and B of every cell, (4) one
// batched Cholesky per group, (5) the triangular solve, objective and
// prediction of every cell.
// Everything is launched on the Runner's one stream; what overlaps is the
// Runners of different groups.  Per-slot state (scaled inputs, K_mm -> u, s,
// st, K_nm, U1 -> ut, C, B -> L) lives in chunk-sized slot arrays; the
// per-cell scratch of phase 5 is reused from cell to cell in stream order.
class Runner {
 public:
  // Reads cells from *tab (rows indexed by cell id; the table may grow between
  // calls); every cell has n <= nmax, M <= mmax; at most `cap` cells per
  // evaluation.  What every evaluation computes is fixed here: the objective
  // (obj), the prediction at the cell's target (pred), both in one pass, or
  // neither (only what set_multi adds).  own_stream: work on a private stream
  // (several Runners then overlap); otherwise on the caller's opts.stream
  Runner(const std::vector<CellSrc>* tab, int64_t nmax, int64_t mmax, int64_t cap, const oi_options& o, bool obj,
         bool pred, bool own_stream = false);
  ~Runner();

  // every later evaluation also predicts cell id c at its targets m->toffs[c] ..
  // (fs, var, cov of *m, which must outlive those evaluations)
  void set_multi(const MultiDev* m) { multi_ = m; }

  // cells[k] at LINEAR hypers hyp[k*5 ..]; results into out[k].  `mean` is the
  // prior mean a prediction adds back; the objective never reads it
  void run(const std::vector<int64_t>& cells, const double* hyp, double mean, CellOut* out);
  // the table's cells 0 .. ncell - 1
  void run_all(int64_t ncell, const double* hyp, double mean, CellOut* out);

  // queue one evaluation of cells[k] at hyp[k*5 ..] (copied) without waiting:
  // the rounds of a fit, which predict nothing and are given no mean
  void enqueue(const std::vector<int64_t>& cells, const double* hyp);
  // wait for the queued evaluation; out[k] for the enqueued cells[k]
  void collect(CellOut* out);

 private:
  int64_t Mof(int64_t c) const { return (*tab_)[c].M; }
  int64_t Mp(int64_t M) const { return padded(M, kn_.padq); }

  struct CellRefs {
    int64_t c, k, n, M, Mp;
    int in, iM, iMp;
    double dn, dM;
    const double* x;
    const double* r;
    const int64_t* sl;
    const double* hp;
    double *sc, *sq, *Kmm, *s, *stl, *C, *B, *rs, *dinv;
  };
  CellRefs refs(int64_t p, int64_t slot);
  void phase1(int64_t p, int64_t slot);
  void batched(int64_t p0, int64_t p1, int which);
  void batched3(int64_t p0, int64_t p1);
  void phase5(int64_t p, int64_t slot);
  void predict_multi(const CellRefs& R, const double* Wt, const double* Av);

  const std::vector<CellSrc>* tab_;
  int64_t cap_ = 0;
  const Knobs kn_;
  OwnStream own_;  // declared before every buffer: destroyed after them
  hipStream_t st_;
  const bool obj_, pred_;
  DevBuf fixed_, slots_;  // the two workspaces
  Fixed fx_;              // ... and their arrays
  Slots sl_;
  int64_t chunk_ = 1;
  oila::Stager la_;
  StageTimer sg_{kStage, S_COUNT};
  std::vector<int64_t> order_;
  std::vector<int64_t> cellv_;  // the queued evaluation's cells and hypers
  std::vector<double> hypv_;
  int64_t ncq_ = 0;
  double mean_ = 0.0;
  const MultiDev* multi_ = nullptr;
  HostBuf hres_, hinfo_;  // pinned: the result copies stay asynchronous
  double* hr_ = nullptr;
  int32_t* hi_ = nullptr;
};

}  // namespace oi_nys
