// The Nystrom fit (NB1 code cell 5: SMLII(approx=True) under scipy's CG per
// cell, then GPR(approx=True) at the fitted hypers), as one call
// (oi_nystrom_fit_batch) and as a session that batches continuously across
// calls (oi_nystrom_session_*).  Host code only: the objective and the
// prediction are evaluated by the Runners of oi_nystrom.hip (oi_nystrom.h).
//
// Both entries schedule the fit with one FitLoop -- G groups, each a Runner
// that keeps up to `cap` cells fitting and refills from a queue -- and differ
// in those two numbers and in when they predict.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <deque>
#include <functional>
#include <memory>
#include <vector>

#include "oi_host.h"
#include "oi_nystrom.h"

#pragma clang fp contract(off)

using namespace oi_nys;

namespace {

// ---- the steps of one cell's fit (NB1 SMLII + scipy CG)

// A cell's restated scipy CG at x0 (6-slot; the sixth gradient is 0, which
// leaves scipy's iteration unchanged) and its first requested point (req, 6).
// Returns whether the cell wants an evaluation.
bool cg_start(oi_cg*& cg, const double* x0, double gtol, int32_t maxiter, double* req) {
  const double x6[6] = {x0[0], x0[1], x0[2], x0[3], x0[4], 0.0};
  cg = oi_cg_create(x6, gtol, maxiter);
  if (!cg) throw std::bad_alloc();
  const int rc = oi_cg_step(cg, req);
  if (rc < 0) throw HipErr{"oi_cg_step failed"};
  return rc == 1;
}

// Feeds one evaluation to the cell's CG; the next requested point into req.
// Returns whether the cell wants another evaluation.
bool cg_advance(oi_cg* cg, const CellOut& r, double* req) {
  const double g6[6] = {r.grad[0], r.grad[1], r.grad[2], r.grad[3], r.grad[4], 0.0};
  if (oi_cg_feed(cg, r.nlz, g6) != 0) throw HipErr{"oi_cg_feed failed"};
  const int rc = oi_cg_step(cg, req);
  if (rc < 0) throw HipErr{"oi_cg_step failed"};
  return rc == 1;
}

// The fitted LINEAR hypers (5) of a finished cell; info[4] = (nit, status,
// nfev, nobj) when asked for.
void cg_readout(oi_cg* cg, double* hyp, int32_t* info) {
  double xf[6], fun;
  int32_t nit, cst;
  int64_t nfev, njev, nobj;
  oi_cg_result(cg, xf, &fun, &nit, &cst, &nfev, &njev, &nobj);
  if (info) {
    info[0] = nit;
    info[1] = cst;
    info[2] = (int32_t)nfev;
    info[3] = (int32_t)nobj;
  }
  for (int q = 0; q < 5; ++q) hyp[q] = std::exp(xf[q]);
}

// out[8] = (fs, sd, prior sd, the 5 fitted hypers): NB1 code cell 5's row
void write_fit(const CellOut& r, const double* hyp, double* out, int32_t* status) {
  *status = r.status;
  out[0] = r.fs;
  out[1] = r.sd;
  out[2] = r.sprior;
  for (int q = 0; q < 5; ++q) out[3 + q] = hyp[q];
}

// The fit's scheduling.  Cells are independent: `groups` groups, each with a
// Runner for the objective (on a stream of its own when there are several, so
// one group's latency-bound batched eigh overlaps the other's panels /
// objective pass), keep up to `cap` cells fitting.  A pass feeds each group's
// finished round to its cells' CG, refills the group from the queue and
// launches its next round at once.  Per-cell arithmetic never depends on the
// other resident cells, so any grouping gives the same results bit for bit.
class FitLoop {
 public:
  // Cell ids are rows of *tab (which may grow between calls); on_fitted(c) is
  // called, from pump or resize, the moment cell c's CG has ended.
  FitLoop(const std::vector<CellSrc>* tab, int groups, int64_t cap, const oi_options& o,
          std::function<void(int64_t)> on_fitted = nullptr)
      : tab_(tab), cap_(cap), o_(o), maxiter_(o.maxiter < 0 ? 1000 : o.maxiter),  // scipy: len(x0) * 200 for NB1's 5 hypers
        on_fitted_(std::move(on_fitted)), grp_(groups) {}
  ~FitLoop() {
    for (Cell& c : cells_)
      if (c.cg) oi_cg_destroy(c.cg);
  }

  // the Runners' sizes: 0 until the first resize
  int64_t nmax() const { return nmax_; }
  int64_t mmax() const { return mmax_; }

  // every group idle (their rounds collected and fed)
  void drain() {
    for (Grp& g : grp_) feed(g);
  }

  // Runners for cells of up to nmax x mmax (and what they held before), once
  // no round is in flight over the old Runners' workspaces
  void resize(int64_t nmax, int64_t mmax) {
    drain();
    nmax_ = std::max(nmax_, nmax);
    mmax_ = std::max(mmax_, mmax);
    for (Grp& g : grp_) g.R.reset(new Runner(tab_, nmax_, mmax_, cap_, o_, true, false, grp_.size() > 1));
  }

  // queue cell c to start from x0 (5, read at admission); `owner` is the
  // caller's own link.  pin >= 0: only that group may admit it
  void add(int64_t c, const double* x0, int64_t owner, int pin = -1) {
    if (c >= (int64_t)cells_.size()) cells_.resize(c + 1);
    cells_[c].x0 = x0;
    cells_[c].owner = owner;
    cells_[c].pin = pin;
    queue_.push_back(c);
  }
  int64_t owner(int64_t c) const { return cells_[c].owner; }

  // one pass over the groups; whether any round is in flight after it
  bool pump() {
    bool any = false;
    for (size_t g = 0; g < grp_.size(); ++g) {
      feed(grp_[g]);
      admit(grp_[g], (int)g);
      launch(grp_[g]);
      any = any || grp_[g].inflight;
    }
    return any;
  }

  // a fitted cell's LINEAR hypers and info (cg_readout); release: its CG is no longer needed
  void readout(int64_t c, double* hyp, int32_t* info) const { cg_readout(cells_[c].cg, hyp, info); }
  void release(int64_t c) {
    oi_cg_destroy(cells_[c].cg);
    cells_[c].cg = nullptr;
  }

 private:
  struct Cell {
    oi_cg* cg = nullptr;         // null before admission and after release
    double req[6] = {};          // the requested point
    const double* x0 = nullptr;  // the start point
    int64_t owner = 0;
    int pin = -1;
    bool fitted = false;
  };
  struct Grp {
    std::unique_ptr<Runner> R;
    std::vector<int64_t> live;  // admitted, still fitting: the cells of every round
    bool inflight = false;      // a round of `live` is queued on R
    std::vector<CellOut> res;   // ... and its results, once collected
  };

  void finish(int64_t c) {
    cells_[c].fitted = true;
    if (on_fitted_) on_fitted_(c);
  }

  void feed(Grp& g) {  // collect a group's round, advance its cells' CG
    if (!g.inflight) return;
    g.res.resize(g.live.size());
    g.R->collect(g.res.data());
    g.inflight = false;
    for (size_t k = 0; k < g.live.size(); ++k) {
      const int64_t c = g.live[k];
      if (!cg_advance(cells_[c].cg, g.res[k], cells_[c].req)) finish(c);
    }
    std::vector<int64_t> keep;
    for (int64_t c : g.live)
      if (!cells_[c].fitted) keep.push_back(c);
    g.live.swap(keep);
  }

  void admit(Grp& g, int gi) {  // from the queue's front, in order, while there is room
    while ((int64_t)g.live.size() < cap_ && !queue_.empty()) {
      const int64_t c = queue_.front();
      if (cells_[c].pin >= 0 && cells_[c].pin != gi) break;
      queue_.pop_front();
      if (cg_start(cells_[c].cg, cells_[c].x0, o_.gtol, maxiter_, cells_[c].req))
        g.live.push_back(c);
      else
        finish(c);
    }
  }

  void launch(Grp& g) {  // one evaluation round of the group's live cells
    if (g.live.empty()) return;
    std::vector<double> hyp;
    for (int64_t c : g.live)
      for (int q = 0; q < 5; ++q) hyp.push_back(std::exp(cells_[c].req[q]));  // NB1 SMLII
    g.R->enqueue(g.live, hyp.data());
    g.inflight = true;
  }

  const std::vector<CellSrc>* tab_;
  const int64_t cap_;
  const oi_options o_;
  const int32_t maxiter_;
  const std::function<void(int64_t)> on_fitted_;
  int64_t nmax_ = 0, mmax_ = 0;  // the Runners' sizes
  std::vector<Cell> cells_;      // by cell id
  std::deque<int64_t> queue_;    // added, not admitted
  std::vector<Grp> grp_;
};

}  // namespace

extern "C" int oi_nystrom_fit_batch(const double* xyt, const double* y, const int64_t* offs,
                                    int64_t ncell, const int64_t* sel, const int64_t* soffs,
                                    const double* x0, const double* xs, double mean, double* out,
                                    int32_t* status, int32_t* info, const oi_options* opts) {
  Batch b{xyt, y, offs, ncell, sel, soffs};
  if (int rc = check_batch(b)) return rc;
  if (ncell == 0) return 0;
  if (!x0 || !xs || !out || !status) return oi_set_last_error(OI_E_ARG, "null pointer");
  const oi_options o = oi_resolve(opts);
  if (int rc = oi_select_device(o)) return rc;
  return oi_guarded([&] {
    BatchDev bd(b, xs, o.device_inputs != 0, (hipStream_t)o.stream);
    std::vector<double> hyp(ncell * 5);
    {
      // G groups (OI_NYS_GROUPS, default 2) that hold all their cells from the
      // first round on: group g the cells c = g mod G, in ascending order
      const int G = (int)std::min<int64_t>(Knobs().groups, ncell);
      FitLoop loop(&bd.rows, G, (ncell + G - 1) / G, o);
      loop.resize(b.nmax, b.mmax);
      for (int g = 0; g < G; ++g)
        for (int64_t c = g; c < ncell; c += G) loop.add(c, x0, 0, g);
      while (loop.pump()) {
      }
      for (int64_t c = 0; c < ncell; ++c) loop.readout(c, hyp.data() + c * 5, info ? info + c * 4 : nullptr);
    }  // the groups' Runners and workspaces are gone before the predict Runner is built
    Runner R(&bd.rows, b.nmax, b.mmax, ncell, o, false, true);
    // NB1 code cell 5: GPR(approx=True) at the fitted hypers
    std::vector<CellOut> res(ncell);
    R.run_all(ncell, hyp.data(), mean, res.data());
    for (int64_t c = 0; c < ncell; ++c) write_fit(res[c], hyp.data() + c * 5, out + c * 8, status + c);
    return 0;
  });
}

// ---- Nystrom fit session: continuous batching across calls (NB1 code cell 5
// as a stream of batches).  Every submitted batch joins one queue of cells;
// each of the G groups (own stream, Runner) keeps up to CAP cells fitting and
// refills from the queue as cells finish, so a call's slowest cells overlap
// the next calls' cells instead of idling the GPU (the one-shot fit waits for
// its slowest cell).  A ticket completes when its last cell is fitted; its
// predictions (GPR(approx=True) at the fitted hypers) run then.  Per-cell
// arithmetic never depends on the other resident cells, so results equal
// oi_nystrom_fit_batch's bit for bit.
namespace {
struct NysTicket {
  std::unique_ptr<BatchDev> dev;
  int64_t first = 0, count = 0, unfitted = 0;
  double x0[5] = {};
  double mean = 0.0;
  double* out = nullptr;
  int32_t* status = nullptr;
  int32_t* info = nullptr;
  bool done = false;
};
}  // namespace

struct oi_nystrom_session {
  const oi_options o;
  const Knobs kn;  // as the environment was at create: kn.groups groups of up to kn.cap fitting cells
  std::vector<CellSrc> tab;  // every submitted cell, by global id
  std::vector<std::unique_ptr<NysTicket>> tickets;
  std::unique_ptr<FitLoop> loop;
  std::unique_ptr<Runner> pred;  // predictions of completed tickets
  // inputs of submitted batches are allocated, copied and freed on this stream
  // (stream-ordered): dropping a completed batch never drains the groups'
  // rounds in flight (a ticket's cells are in no round by then)
  OwnStream io;

  explicit oi_nystrom_session(const oi_options& opts)
      : o(opts), loop(new FitLoop(&tab, kn.groups, kn.cap, o, [this](int64_t c) { finished(c); })) {
    io.create();
  }
  ~oi_nystrom_session() {
    loop.reset();
    pred.reset();
    tickets.clear();
    if (io.s) (void)hipStreamSynchronize(io.s);
  }

  void build_runners(int64_t nm, int64_t mm) {
    loop->resize(nm, mm);
    pred.reset(new Runner(&tab, loop->nmax(), loop->mmax(), kn.cap, o, false, true, true));
  }

  void finished(int64_t c) {
    NysTicket& t = *tickets[loop->owner(c)];
    if (--t.unfitted == 0) complete(t);
  }

  void complete(NysTicket& t) {
    // GPR(approx=True) at the fitted hypers, in chunks of the Runner capacity
    Runner& R = *pred;
    const int64_t cap = kn.cap;
    std::vector<CellOut> res(cap);
    for (int64_t a = 0; a < t.count; a += cap) {
      const int64_t b = std::min(t.count, a + cap);
      std::vector<int64_t> cells(b - a);
      std::vector<double> hyp((b - a) * 5);
      for (int64_t k = a; k < b; ++k) {
        cells[k - a] = t.first + k;
        loop->readout(t.first + k, hyp.data() + (k - a) * 5, t.info ? t.info + k * 4 : nullptr);
      }
      R.run(cells, hyp.data(), t.mean, res.data());
      for (int64_t k = a; k < b; ++k)
        write_fit(res[k - a], hyp.data() + (k - a) * 5, t.out + k * 8, t.status + k);
    }
    for (int64_t k = 0; k < t.count; ++k) loop->release(t.first + k);
    t.done = true;
    t.dev.reset();  // no round reads the batch any more: freed in io-stream order
  }

  // rounds until ticket t (all work when t < 0) is complete
  void wait(int64_t t) {
    while (!(t >= 0 && tickets[t]->done))
      if (!loop->pump()) {
        if (t >= 0 && !tickets[t]->done) throw HipErr{"nystrom session: ticket cannot complete"};
        return;
      }
  }
};

extern "C" oi_nystrom_session* oi_nystrom_session_create(const oi_options* opts) {
  const oi_options o = oi_resolve(opts);
  if (oi_select_device(o)) return nullptr;
  std::unique_ptr<oi_nystrom_session> s;
  if (oi_guarded([&] {
        s = std::make_unique<oi_nystrom_session>(o);
        return 0;
      }))
    return nullptr;
  return s.release();
}

extern "C" int64_t oi_nystrom_session_submit(oi_nystrom_session* s, const double* xyt, const double* y,
                                             const int64_t* offs, int64_t ncell, const int64_t* sel,
                                             const int64_t* soffs, const double* x0, const double* xs,
                                             double mean, double* out, int32_t* status, int32_t* info) {
  if (!s) return oi_set_last_error(OI_E_ARG, "null session");
  Batch b{xyt, y, offs, ncell, sel, soffs};
  if (int rc = check_batch(b)) return rc;
  if (ncell > 0 && (!x0 || !xs || !out || !status)) return oi_set_last_error(OI_E_ARG, "null pointer");
  int64_t ticket = -1;
  const int rc = oi_guarded([&] {
    HC(hipSetDevice(s->o.device));
    auto t = std::make_unique<NysTicket>();
    t->first = (int64_t)s->tab.size();
    t->count = ncell;
    t->unfitted = ncell;
    t->mean = mean;
    t->out = out;
    t->status = status;
    t->info = info;
    ticket = (int64_t)s->tickets.size();
    if (ncell > 0) {
      std::copy(x0, x0 + 5, t->x0);
      t->dev.reset(new BatchDev(b, xs, s->o.device_inputs != 0, s->io.s));
      if (b.nmax > s->loop->nmax() || b.mmax > s->loop->mmax())  // the first batch always: every cell has n >= 1
        s->build_runners(b.nmax, b.mmax);
      for (int64_t c = 0; c < ncell; ++c) {
        s->tab.push_back(t->dev->rows[c]);
        s->loop->add(t->first + c, t->x0, ticket);
      }
    } else {
      t->done = true;
    }
    s->tickets.push_back(std::move(t));
    return 0;
  });
  return rc ? rc : ticket;
}

extern "C" int oi_nystrom_session_wait(oi_nystrom_session* s, int64_t ticket) {
  if (!s) return oi_set_last_error(OI_E_ARG, "null session");
  if (ticket >= (int64_t)s->tickets.size()) return oi_set_last_error(OI_E_ARG, "unknown ticket");
  return oi_guarded([&] {
    HC(hipSetDevice(s->o.device));
    s->wait(ticket);
    return 0;
  });
}

extern "C" void oi_nystrom_session_destroy(oi_nystrom_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->o.device);
  try {
    s->loop->drain();
  } catch (...) {
  }
  delete s;
}
