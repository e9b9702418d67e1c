// What the dense-GP entry points share on the host (oi_predict.hip: many
// targets per cell; oi_cv.hip: leave-one-out and leave-group-out; oi_sample.hip:
// posterior draws; oi_grad.hip: the posterior of the field's gradient): the
// per-cell descriptor, the workspace layout of a chunk and of a cell, the
// argument checks, and Front, which runs a chunk up to the solved X.  Host
// declarations only; the kernels that read a PCell and Front's methods are in
// oi_predict.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "oi_host.h"
#include "oi_linalg.h"

namespace oi_dense {

constexpr double LOG2PI = 1.8378770664093453;  // np.log(2 * np.pi)

// One cell of a chunk (device pointers; the row of the descriptor array that
// every k_pm_* kernel indexes with its block's cell coordinate).
struct PCell {
  const double* x;   // n x 3 inputs
  const double* z;   // n observations
  const double* xs;  // nt x 3 targets
  double* sc;        // n x 3 scaled inputs
  double* xsc;       // nt x 3 scaled targets
  double* K;         // Np x Np: K + sn2 I, then its Cholesky factor (lower)
  double* X;         // (rpt nt + 1) x n, leading dimension rpt nt + 1 (rpt rows per target: 1, the gradient's 4)
  double* cov;       // nt x nt (leading dimension nt) or null
  double* fs;        // nt
  double* sd;        // nt
  double* lz;        // 1
  int32_t* info;     // the Cholesky's info
  int32_t* status;   // 1
  int n, nt, Np;
  double l0, l1, l2, sf2, sn2, mean;
};

constexpr int64_t CHUNK_SLACK = 8 * 32;  // rounding of the chunk-wide arrays (doubles)
constexpr int64_t CHUNK_CELLS = 4096;    // cells per chunk at most (launch grids, descriptor arrays)

// The two layout functions below are the one description of every entry
// point's shared workspace.  A cell's size for the chunk planner is the same
// functions on counting Carvers: its own arrays rounded to 32 doubles (256
// bytes), plus its unrounded share of the chunk-wide arrays (the cells' parts
// back to back).
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
                       int64_t no, int64_t nc, int64_t cc);
// One cell's own: scaled inputs 3 n and targets 3 nt, K Np^2, the factor's
// diagonal-block inverses 64 Np, X (rpt nt + 1) n; leave-one-out adds their
// transposes 64 Np and the lpl partials Np / 64 (the sweep writes the panels of
// W' into K above the diagonal blocks and needs no n x n array of its own).
struct DenseCell {
  double *sc, *xsc, *K, *dinv, *wdt, *X, *part;
};
DenseCell dense_cell(Carver& cv, int64_t n, int64_t nt, bool loo, int64_t rpt = 1);
// with cov the chunk-wide share holds the cell's (rpt nt)^2
int64_t dense_cell_doubles(int64_t n, int64_t nt, bool cov, bool host_inputs, bool loo, int64_t rpt = 1);

// The checks every entry makes after its offsets, in their order: null status,
// null hyp, null xyt / z with observations, then `missing` (the entry's own
// null-pointer message, or null), then every cell's arrays against oila's
// 32-bit byte offsets: K always, and what `lim` names of X (rpt nt + 1) n (and
// its row count rpt nt + 1 alone, which a cell without observations must keep
// an int as well), cov
// (rpt nt)^2, the padded C Ntp^2 and nt nsamp.  toffs may be null (no targets).
struct DenseLimits {
  bool X, cov, C;
  int64_t nsamp;    // < 0: no samples
  int64_t rpt = 1;  // rows of X (and of cov) per target
};
int dense_check(const double* xyt, const double* z, const int64_t* offs, const int64_t* toffs, int64_t ncell,
                const double* hyp, const int32_t* status, const char* missing, const DenseLimits& lim);

// An entry's own generator of X: launches on st over the chunk's nc cells (dc),
// none of which has more than nmax observations or ntmax targets
using XGen = void (*)(const PCell* dc, int64_t nmax, int64_t ntmax, unsigned nc, hipStream_t st);

// What the entries share per chunk: the workspace, staging, carving, the PCell
// descriptors, generation, Cholesky and solve; status copy and hand-over.
struct Front {
  const oi_options o;
  const DenseIn in;
  const int64_t* offs;
  const double* hyp;
  const double mean;
  const bool loo;
  const int64_t rpt;  // rows of X per target
  const XGen xgen;    // the caller's X generator, or null: k_pm_xgen
  hipStream_t st = in.st;
  oila::Stager la;
  StageTimer sg;
  DevBuf ws;
  Carver cv;  // the chunk's; an entry carves its own arrays from it as well
  int64_t biggest = 0;
  std::vector<PCell> cells;
  std::vector<oila::Chol> chol;
  std::vector<oila::TrsmRLT> trsm;
  DenseChunk k;    // the chunk's arrays
  int64_t c0, nc;  // its cells
  int64_t nmax, ntmax, pts, xel;
  double fl_chol, fl_solve, by_gen;

  Front(const oi_options& o, const double* xyt, const double* z, const int64_t* offs, const double* hyp, double mean,
        bool loo, const char* const* stages, int count, int64_t rpt = 1, XGen xgen = nullptr);
  // the chunks' cuts (plan_chunks) and the workspace that holds the largest
  template <class F>
  std::vector<int64_t> plan(int64_t ncell, int64_t slack, const char* what, F&& cell_doubles) {
    ChunkPlan p = plan_chunks(ncell, o, slack, CHUNK_CELLS, what, cell_doubles);
    biggest = p.biggest;
    ws.alloc((size_t)biggest * 8);
    return p.cuts;
  }
  // cells c0 .. c1 - 1 with their tt targets at xs and cc covariance elements
  void begin(int64_t c0, int64_t c1, const double* xs, int64_t tt, int64_t cc);
  // the chunk's next cell c with nt targets from target toff of the chunk: its
  // arrays into a, and its descriptor but for cov
  PCell& add(int64_t c, int64_t nt, int64_t toff, DenseCell& a);
  // descriptors up (returned), then generate, factor and solve under the
  // caller's stage ids; `entry` names the caller should the layout have
  // outgrown the planner's estimate
  const PCell* factor(const char* entry, int s_gen, int s_chol, int s_solve);
  // fs, sd, lZ and status from the solved X (k_pm_reduce) as stage `stage`
  void reduce(int stage, double by_red, const PCell* dc);
  // after the caller's tail; the next chunk reuses the workspace and the descriptor ring
  void finish(int32_t* status);
};

}  // namespace oi_dense
