/* liboi -- MI355X-native per-grid-cell full-GP regression (C ABI).
 *
 * Drop-in boundary for the hot path of William-gregory/OptimalInterpolation,
 * 2021_paper_production/GPR_CS2S3.py (abbreviated GPR: below):
 *
 *   oi_gpr_batch        replaces the per-cell loops GPR:258-261 (pass 1,
 *                       GPR3D(index) with opt=True) and GPR:316-319 (pass 2,
 *                       GPR3D(index, opt=False)): one call fits / predicts a
 *                       ragged batch of cells.  Per cell it computes exactly
 *                       what GPR3D (GPR:143-191) returns.
 *   oi_gpr_predict_multi  the predict step (GPR:173-182) at many targets per
 *                       cell, as GP_example.ipynb's GPR() takes them (xs of
 *                       size ns x 3), with the full posterior covariance.
 *   oi_nlml_grad_batch  replaces SMLII (GPR:107-141) for a batch of cells at
 *                       given log-hyper-parameters.
 *   oi_cg_*             the host optimiser on its own: scipy's
 *                       minimize(method='CG', jac=True) as called at GPR:166,
 *                       driven by caller-supplied objective values.
 *
 * Conventions: plain host pointers, row-major arrays, fp64 throughout.  The
 * library owns all device memory.  Functions return 0 on success or a
 * negative OI_E* code (API misuse / HIP failure; message via oi_last_error).
 * Per-cell numerical failure is NOT an error: as in GPR:139-140 and
 * GPR:187-191, a non-positive-definite covariance gives nlZ = +inf / gradient
 * +inf (objective) or NaN outputs (GPR3D), with status[c] = 1.
 * A cell with zero observations is valid (GPR3D returns (mean, sqrt(sf2), -0, ...)).
 */
#ifndef OI_H
#define OI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OI_VERSION 1

#define OI_E_ARG (-1)    /* invalid argument */
#define OI_E_HIP (-2)    /* HIP runtime / kernel launch failure */
#define OI_E_NOMEM (-3)  /* a single cell does not fit the device workspace */
#define OI_E_NODEV (-4)  /* no usable GPU */

typedef struct oi_options {
  int32_t device;      /* HIP device ordinal (default 0) */
  int32_t maxiter;     /* CG maxiter; <0 => len(x0)*200 = 1200 (scipy default) */
  double gtol;         /* CG gradient tolerance (scipy default 1e-5) */
  void* stream;        /* hipStream_t to launch on; NULL => the library's stream */
  int64_t pool_bytes;  /* device workspace budget; 0 => 60% of free HBM */
  int32_t max_pool;    /* max cells resident at once; 0 => automatic */
  int32_t profile;     /* 1 => record per-kernel HIP-event timings (oi_profile_json) */
  int32_t device_inputs; /* 1 => xyt / z / y / mX are DEVICE pointers already resident
                            in HBM on `device` (offs, xs, x0, hyp, h stay on the host) */
} oi_options;

/* Fill *o with defaults. */
void oi_options_default(oi_options* o);

/* Per-cell GP regression for a ragged batch (GPR3D semantics, GPR:143-191).
 *   xyt    [N x 3]  neighbour inputs (x [m], y [m], t [day]) of all cells,
 *                   cell c owning rows offs[c] .. offs[c+1]-1, in the order
 *                   the caller's neighbour query returned them (GPR:159-160)
 *   z      [N]      observations (GPR:161)
 *   offs   [ncell+1] row offsets, offs[0] = 0, non-decreasing
 *   xs     [ncell x 3] prediction targets (cx, cy, T_mid)  (GPR:164)
 *   mean   prior mean (GPR:212); mX = mean * ones(n)      (GPR:163)
 *   x0     [6] initial log-hyper-parameters (GPR:217); used when opt != 0
 *   opt    1: fit hypers by CG then predict (GPR:166-168)
 *          0: predict with given hypers hyp (GPR:170-172)
 *   hyp    [ncell x 5] (lx, ly, lt, sf2, sn2) when opt == 0, else NULL
 *   out    [ncell x 8] (fs, sd, lZ, lx, ly, lt, sf2, sn2); for opt == 0
 *                   only fs, sd, lZ are meaningful (hyp echoed in 3..7)
 *   status [ncell]   0 ok, 1 covariance not positive definite (NaN outputs)
 *   info   [ncell x 4] or NULL: (nit, cg_status, nfev, n_objective_evals)
 */
int oi_gpr_batch(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                 const double* xs, double mean, const double* x0, int32_t opt,
                 const double* hyp, double* out, int32_t* status, int32_t* info,
                 const oi_options* opts);

/* Workspace of the engine entries (oi_gpr_batch, oi_nlml_grad_batch,
 * oi_session_*): opts->pool_bytes is the device arena the resident cells'
 * tiles are carved from and opts->max_pool the number of cells resident at
 * once; a batch is refused at submission, before any launch, with OI_E_NOMEM
 * ("a cell needs ...") when its largest cell alone exceeds the pool.  A batch
 * that passes this check completes, in a pool of exactly that cell too: cells
 * wait their turn for slots and memory, and the batch's staged inputs, which
 * share the arena while it has room, may live outside the pool. */

/* Stream ordering (opts->device_inputs = 1): device inputs are read on
 * opts->stream when it is set; with stream == NULL the library's own stream
 * first waits for the legacy NULL stream (PyTorch's default stream), so any
 * producer of xyt / z / y / mX queued there has finished.  A producer on
 * another stream must pass that stream.  Host outputs are complete on return. */

/* Prediction at many targets per cell, with the posterior covariance: the
 * notebook's GPR(x, y, xs, ell, sf2, sn2, mean) (GP_example.ipynb, code cell 1)
 * with xs of size ns x 3 -- GPR3D's predict step (GPR:173-182) with ns columns
 * -- for a ragged batch at given hypers (as the opt == 0 call above).
 *   xyt, z, offs, mean  as above (device pointers with opts->device_inputs)
 *   xs     [T x 3]  targets of all cells, cell c owning rows
 *                   toffs[c] .. toffs[c+1]-1; no target (nt = 0) is valid
 *   toffs  [ncell+1] target offsets, toffs[0] = 0, non-decreasing
 *   hyp    [ncell x 5] LINEAR (lx, ly, lt, sf2, sn2)
 *   fs     [T]      mean + Kxsx' A                              (GPR:180)
 *   sd     [T]      sqrt(diag(Kxs - v'v)); NaN where the argument is
 *                   negative, as np.sqrt                        (GPR:181)
 *   lz     [ncell] or NULL: the log marginal likelihood         (GPR:179)
 *   cov    or NULL: Kxs - v'v in full (GPR:181 before its diagonal is taken),
 *                   cell c's nt x nt matrix symmetric, row-major, at offset
 *                   sum_{k<c} nt_k^2; the diagonal of Kxs is sf2 exactly
 *   status [ncell]  0 ok, 1 covariance not positive definite: that cell's fs,
 *                   sd, lz and cov are NaN (GPR:187-191)
 * A cell with no observations gives fs = mean, sd = sqrt(sf2), lz = -0,
 * cov = Kxs.  Cells are worked in chunks that fit opts->pool_bytes (0 => 60%
 * of the free HBM); a cell that does not fit alone is OI_E_NOMEM.  A cell's
 * results do not depend on the other cells of the call or on the chunking. */
int oi_gpr_predict_multi(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                         const double* xs, const int64_t* toffs, double mean, const double* hyp,
                         double* fs, double* sd, double* lz, double* cov,
                         int32_t* status, const oi_options* opts);

/* Leave-one-out prediction of every observation of every cell from the cell's
 * other observations, at given LINEAR hypers (Rasmussen & Williams, GPML
 * 5.4.2), from one factorisation per cell:
 *   r = z - mean, K~ = K + sn2 I = L L', alpha = K~^-1 r, q_i = [K~^-1]_ii
 *   mu_i = z_i - alpha_i / q_i, sd_i = sqrt(1 / q_i)
 *   lpl  = sum_i [ -log(2 pi)/2 - log sd_i - (z_i - mu_i)^2 / (2 sd_i^2) ]
 * mu_i and sd_i are the predictive mean and standard deviation of OBSERVATION
 * i (noise included: sd_i^2 is the latent variance + sn2); the standardised
 * residual is (z_i - mu_i) / sd_i.
 *   xyt, z, offs  the ragged batch, as oi_gpr_batch (a cell may be empty)
 *   hyp    [ncell x 5] LINEAR (ell_x, ell_y, ell_t, sf2, sn2)
 *   mu, sd [N]      in the observations' own order
 *   lpl    [ncell]  or NULL: the log pseudo-likelihood; 0 for an empty cell
 *   status [ncell]  0 ok, 1 the Cholesky failed: that cell's mu, sd and lpl
 *                   are NaN
 * n = 1 gives the prior: mu = mean, sd = sqrt(sf2 + sn2).  hyp, offs and all
 * outputs are host arrays; with opts->device_inputs xyt and z are device
 * pointers.  opts->stream, pool_bytes, max_pool and profile act as in
 * oi_gpr_predict_multi; a cell's results depend neither on the other cells
 * of the call nor on the chunking.  OI_E_ARG (before any device is touched):
 * bad offs, a null pointer, a cell whose padded n x n matrix reaches 2 GiB.
 * OI_E_NOMEM: a cell whose workspace (about 8 n^2 bytes) exceeds
 * opts->pool_bytes (0 => 60% of the free HBM), with no output written. */
int oi_gpr_loo(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
               double mean, const double* hyp, double* mu, double* sd, double* lpl,
               int32_t* status, const oi_options* opts);

/* Leave-group-out prediction: every group of observations of a cell (a site,
 * a pass, a day, a satellite) is predicted jointly from the cell's observations
 * outside it, at given LINEAR hypers, from one factorisation per cell
 * (Rasmussen & Williams, GPML 5.4.2, in block form):
 *   r = z - mean, K~ = K + sn2 I, alpha = K~^-1 r, Q = K~^-1
 * and for a group G of g observations, Q_GG = C C',
 *   Sigma_G = Q_GG^-1           the predictive covariance of the group's
 *                               OBSERVATIONS (noise included) given the others
 *   mu_G = z_G - Q_GG^-1 alpha_G,  sd_i = sqrt([Q_GG^-1]_ii)
 *   d2_G = alpha_G' Q_GG^-1 alpha_G        (chi^2 with g degrees under the model)
 *   lpd_G = log N(z_G | mu_G, Sigma_G) = -d2_G / 2 + sum_k log C_kk - g log(2 pi) / 2
 *   lpl = sum_G lpd_G
 * A group of one is leave-one-out (oi_gpr_loo); a group that is the whole cell
 * gives the prior: mu = mean, Sigma = K~.
 *   xyt, z, offs  the ragged batch, as oi_gpr_batch (a cell may be empty)
 *   group  [N]      the label of each observation.  Labels are compared only
 *                   inside a cell and only for equality: any int64 is a label,
 *                   and the same label in two cells means nothing.  Groups are
 *                   taken in the order of their first appearance in the cell,
 *                   members in observation order, so results depend on the
 *                   partition and never on the label values.
 *   hyp    [ncell x 5] LINEAR (ell_x, ell_y, ell_t, sf2, sn2)
 *   mu, sd [N]      in the observations' own order
 *   lpd, d2 [N]     or NULL: the value of the observation's group, repeated for
 *                   every member
 *   lpl    [ncell]  or NULL; 0 for an empty cell
 *   status [ncell]  0 ok; 1 the cell's Cholesky failed: all of that cell's
 *                   outputs are NaN; 2 some group's Q_GG failed to factor: those
 *                   groups' rows and the cell's lpl are NaN, other groups' rows
 *                   are valid
 * n = 1 gives the prior: mu = mean, sd = sqrt(sf2 + sn2).  group, hyp, offs and
 * all outputs are host arrays; with opts->device_inputs xyt and z are device
 * pointers (group stays a host array).  opts->stream, pool_bytes, max_pool and
 * profile act as in oi_gpr_loo; a cell's results depend neither on the other
 * cells of the call nor on the chunking.  OI_E_ARG (before any device is
 * touched): bad offs, a null pointer, a cell whose padded n x n matrix reaches
 * 2 GiB.  OI_E_NOMEM: a cell whose workspace exceeds opts->pool_bytes (0 => 60%
 * of the free HBM), with no output written; a cell needs oi_gpr_loo's
 * workspace (about 8 n^2 bytes) plus, per group, 8 (gp^2 + 64 gp + (g + 1) g)
 * bytes with gp = g rounded up to 64 -- about three times oi_gpr_loo's when the
 * cell is one group. */
int oi_gpr_lgo(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
               const int64_t* group, double mean, const double* hyp, double* mu, double* sd,
               double* lpd, double* d2, double* lpl, int32_t* status, const oi_options* opts);

/* nsamp joint draws from every cell's GP posterior at the cell's own targets,
 * at given LINEAR hypers.  Per cell, with fs and cov = Kxs - v'v exactly as
 * oi_gpr_predict_multi forms them:
 *   C = cov + (noise ? sn2 : 0) I + jitter I = Lc Lc'
 *   samples[t, s] = fs[t] + sum_u Lc[t, u] Xi[u, s]
 *   xyt, z, offs  the ragged batch, as oi_gpr_batch (a cell may be empty: the
 *                 prior is drawn)
 *   xs, toffs     targets [T x 3], cell c owning rows toffs[c] .. toffs[c + 1];
 *                 T = toffs[ncell]; a cell may have none
 *   hyp     [ncell x 5] LINEAR (ell_x, ell_y, ell_t, sf2, sn2)
 *   nsamp   draws per cell, >= 0
 *   noise   0: the latent field; 1: a new observation (sn2 on the diagonal)
 *   jitter  >= 0, an absolute variance added to the diagonal of C
 *   xi      NULL, or host [T x nsamp] standard normals, row toffs[c] + u and
 *           column s holding Xi[u, s] of cell c: the deterministic mode
 *   seed, streams  with xi == NULL, Xi is generated on the device by
 *           Philox4x32-10 with key = (seed lo, seed hi): element e = s nt + u
 *           of a cell comes from block b = e >> 1 with counter (b lo, b hi,
 *           stream lo, stream hi); with the output words w0 .. w3,
 *           u1 = (((w0 << 21) | (w1 >> 11)) + 1) 2^-53,
 *           u2 = ((w2 << 21) | (w3 >> 11)) 2^-53, r = sqrt(-2 log u1),
 *           theta = 2 pi u2; an even e is r cos theta, an odd e r sin theta.
 *           streams [ncell] holds the cells' stream ids; NULL: the cell's index
 *           in the call.  A cell's draws depend only on (seed, its stream, nt,
 *           the columns asked for): the first S columns of a longer call are
 *           the call with S draws.
 *   samples [T x nsamp] row-major, rows aligned with fs and sd
 *   fs, sd  [T] or NULL: bit for bit those of oi_gpr_predict_multi
 *   status  [ncell]  0 ok; 1 the cell's Cholesky failed: fs, sd and samples
 *           are NaN; 2 the factorisation of C met a pivot <= 0: samples are
 *           NaN, fs and sd valid
 * hyp, offs, toffs, xs, xi, streams and all outputs are host arrays; with
 * opts->device_inputs xyt and z are device pointers.  opts->stream,
 * pool_bytes, max_pool and profile act as in oi_gpr_predict_multi (stages
 * ps_*); a cell's results depend neither on the other cells of the call nor on
 * the chunking.  OI_E_ARG (before any device is touched): bad offs / toffs, a
 * null required pointer, nsamp < 0, noise not 0 or 1, jitter negative or not
 * finite, a cell whose K, X, padded C or nt nsamp reaches 2 GiB.  OI_E_NOMEM:
 * a cell whose workspace exceeds opts->pool_bytes (0 => 60% of the free HBM),
 * with no output written. */
int oi_gpr_sample(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                  const double* xs, const int64_t* toffs, double mean, const double* hyp,
                  int64_t nsamp, int32_t noise, double jitter,
                  uint64_t seed, const uint64_t* streams, const double* xi,
                  double* samples, double* fs, double* sd, int32_t* status,
                  const oi_options* opts);

/* ---- session: continuous batching across calls ------------------------
 * The per-cell loops GPR:258-261 / GPR:316-319 as a stream of batches: every
 * submitted batch (same arguments and semantics as oi_gpr_batch) joins one
 * queue; cells are admitted largest-n first within a batch and FIFO across
 * batches, so cells of the next batch fill the GPU while the previous one's
 * slowest cells finish.  Per-cell results are bitwise the same as one
 * oi_gpr_batch call's (they never depend on which cells share a round).
 *   oi_session_submit  returns a ticket >= 0 (or a negative OI_E* code).  Host
 *                      metadata (offs, xs, x0, hyp) and host inputs are copied
 *                      before it returns; DEVICE inputs and all outputs must
 *                      stay valid until the ticket completes.
 *   oi_session_wait    runs rounds until the ticket completes (ticket < 0: all
 *                      submitted work); it may return with later batches'
 *                      rounds still in flight on the device.
 *   oi_session_set_stream  the stream whose queued work later submissions'
 *                      DEVICE inputs are ordered after (default: opts->stream
 *                      at creation, NULL = the legacy NULL stream); the
 *                      session's rounds keep running on their own stream.
 *   oi_session_done    1 if the ticket has completed, else 0.
 *   oi_session_destroy waits for in-flight rounds and frees the session
 *                      (unfinished cells are dropped, outputs left unwritten).
 * A session is used from one thread at a time. */
typedef struct oi_session oi_session;
oi_session* oi_session_create(const oi_options* opts);
int64_t oi_session_submit(oi_session* s, const double* xyt, const double* z, const int64_t* offs,
                          int64_t ncell, const double* xs, double mean, const double* x0,
                          int32_t opt, const double* hyp, double* out, int32_t* status,
                          int32_t* info);
int oi_session_set_stream(oi_session* s, void* stream);
int oi_session_wait(oi_session* s, int64_t ticket);
int oi_session_done(oi_session* s, int64_t ticket);
void oi_session_destroy(oi_session* s);

/* SMLII (GPR:107-141) for a batch of cells at fixed log-hypers.
 *   xyt, offs as above; y [N] outputs; mX [N] prior mean per observation
 *   h   [ncell x 6] log-hypers (lx, ly, lt, sf2, sn2, unused)
 *   nlz [ncell] ; grad [ncell x 6] (reference gradient incl. its factor-2
 *   components 3 and 4 and the zero 6th component); status [ncell] or NULL
 */
int oi_nlml_grad_batch(const double* xyt, const double* y, const double* mX,
                       const int64_t* offs, int64_t ncell, const double* h, double* nlz,
                       double* grad, int32_t* status, const oi_options* opts);

/* ---- day pipeline: the steps either side of the per-cell loops ----------
 * With opts->device_inputs = 1 every array argument below is a DEVICE pointer
 * on opts->device except vmax, kern and offs, which are always host arrays. */

/* smooth() (GPR:65-76) of nf fields at once -- the five calls GPR:303-307.
 *   fields [nf x ny x nx]  (the reference's 2-D grids, row-major)
 *   vmax   [nf]            clip values (GPR:303-307: 2*radius*1000, .., T, 0.1, 0.05)
 *   mask   [ny x nx]       SIE grid; NaN entries are set to NaN in the output
 *   kern   [ks x ks] or NULL: the Gaussian2DKernel(x_stddev=std) array, ks odd,
 *                          <= 65 (std is then ignored).  NULL => built here from
 *                          std in (0, 8] by astropy's definition, normalised by a
 *                          sum taken in numpy's order (arr.sum()): every entry is
 *                          within 4 ulp of numpy's array (libm's exp against
 *                          numpy's; bit-equal at std = 1 where the two agree).
 *                          The smoothing is bit-exact against the CPU
 *                          restatement FOR THE KERNEL USED: a caller who needs
 *                          bit parity with a numpy / astropy pipeline passes
 *                          that pipeline's array.
 *   out    [nf x ny x nx]
 * inf -> NaN, clip at vmax, astropy convolve() defaults (fill 0 boundary,
 * NaN-interpolating renormalised kernel), zeros -> np.nanmean, mask. */
int oi_smooth_fields(const double* fields, int32_t nf, int64_t ny, int64_t nx, const double* vmax,
                     const double* mask, double std, const double* kern, int32_t ks, double* out,
                     const oi_options* opts);

/* X_tree.query_ball_point(X[index], r) (GPR:159) for Q targets at once.
 *   pts [M x 2] training (x, y); q [Q x 2] targets; r radius (same units)
 *   offs [Q+1] (host) always written: target k owns idx[offs[k] .. offs[k+1])
 *   idx  [cap] written only when cap >= offs[Q] (call once with idx = NULL to
 *        size it).  Indices ascending within a target (sorted(ID)); the test
 *        is scipy cKDTree's p=2 one: (dx*dx + dy*dy) <= r*r. */
int oi_ball_query(const double* pts, int64_t M, const double* q, int64_t Q, double r,
                  int64_t* offs, int64_t* idx, int64_t cap, const oi_options* opts);

/* inputs = [x_train, y_train, t_train][ID], outputs = z[ID] (GPR:160-161) for a
 * ragged index list (e.g. oi_ball_query's idx): xyt [N x 3], zout [N].
 * Out-of-range indices are an OI_E_ARG error (host mode) or NaN rows (device). */
int oi_gather_rows(const double* x_train, const double* y_train, const double* t_train,
                   const double* z, int64_t M, const int64_t* idx, int64_t N, double* xyt,
                   double* zout, const oi_options* opts);

/* ---- Nystrom variant (GP_example.ipynb code cell 1: Nystroem, SMLII and GPR
 * with approx=True) -- the rank-M approximation of the notebook -----------
 * Per cell c (rows offs[c] .. offs[c+1]-1):
 *   xyt [N x 3] inputs, y [N] outputs minus the prior mean (NB1 passes
 *       outputs - mX to both SMLII and GPR; GPR adds `mean` back to fs)
 *   sel [soffs[ncell]] inducing rows of each cell, 0-based within the cell
 *       (NB1 Nystroem: sorted(np.random.choice(range(n), M, replace=False))
 *       after np.random.seed(20); the caller draws them)
 *   hyp [ncell x 5] LINEAR (ell_x, ell_y, ell_t, sf2, sn2) as GPR() takes them
 *       (SMLII's log-hypers exponentiated by the caller)
 *   xs  [ncell x 3] prediction targets (needed with pred)
 *   nlz [ncell], grad [ncell x 5]: SMLII(approx=True) (NULL both to skip)
 *   pred [ncell x 3]: (fs = mean + k*.A, sd, prior sd)  (NULL to skip)
 *   status [ncell]: 0 ok, 1 eigh / Cholesky failed (NB1 LinAlgError):
 *       nlZ = grad = +inf, fs = sd = NaN
 * 1 <= M <= n per cell.  With opts->device_inputs xyt and y are device pointers. */
int oi_nystrom_batch(const double* xyt, const double* y, const int64_t* offs, int64_t ncell,
                     const int64_t* sel, const int64_t* soffs, const double* hyp,
                     const double* xs, double mean, double* nlz, double* grad, double* pred,
                     int32_t* status, const oi_options* opts);

/* NB1 GPR(x, y, xs, ell, sf2, sn2, mean, approx=True, M) with xs of size
 * ns x 3: the Nystrom prediction at many targets per cell with the posterior
 * covariance Kxs - Kxsx' Ki Kxsx that NB1 forms before taking its diagonal.
 * The per-cell set-up (K_mm, eigh, the n x M panels, chol(B), W' = C L^-T, A)
 * runs once per cell, not once per target.
 *   xyt, y, offs, sel, soffs, hyp  as oi_nystrom_batch (LINEAR hypers, y the
 *          residual outputs, 1 <= M <= n)
 *   xs     [T x 3]  targets of all cells, cell c owning rows
 *                   toffs[c] .. toffs[c+1]-1; no target (nt = 0) is valid
 *   toffs  [ncell+1] target offsets, toffs[0] = 0, non-decreasing
 *   fs     [T]      mean + Kxsx' A
 *   sd     [T]      sqrt(diag(Kxs - err)), the root of the returned diagonal bit
 *                   for bit; NaN where the argument is negative, as np.sqrt
 *   cov    or NULL: Kxs - err, err = Kxsx'Kxsx / sn2 - (W Kxsx)'(W Kxsx); cell
 *                   c's nt x nt matrix symmetric, row-major, at offset
 *                   sum_{k<c} nt_k^2; Kxs has the diagonal sf2 exactly.  With
 *                   NULL no nt x nt array exists anywhere and fs, sd are bitwise
 *                   those of a call with cov
 *   status [ncell]  0 ok, 1 eigh / Cholesky failed (NB1 LinAlgError): that
 *                   cell's fs, sd and cov are NaN
 * NB1's Nystrom err routinely exceeds Kxs: NaN entries of sd and a cov that is
 * not positive semi-definite are the reference's results, with status 0.
 * xs, toffs, hyp, sel, soffs and all outputs are host arrays; with
 * opts->device_inputs xyt and y are device pointers.  A cell's results depend
 * neither on the other cells of the call nor on its other targets.  A cell
 * whose scratch (n x nt, M x nt, nt x nt) exceeds opts->pool_bytes (0 => 60%
 * of the free HBM) is OI_E_NOMEM, with no output written. */
int oi_nystrom_predict_multi(const double* xyt, const double* y, const int64_t* offs, int64_t ncell,
                             const int64_t* sel, const int64_t* soffs, const double* hyp,
                             const double* xs, const int64_t* toffs, double mean,
                             double* fs, double* sd, double* cov, int32_t* status,
                             const oi_options* opts);

/* NB1 code cell 5 for a ragged batch: minimize(SMLII, x0, args=(x, y, True, M),
 * method='CG', jac=True) per cell (the restated scipy CG, maxiter <0 => 1000 =
 * len(x0)*200; gtol from opts), then GPR(approx=True, returnprior=True) at the
 * fitted hypers.
 *   x0  [5] initial log-hypers (NB1: log 25e3, log 25e3, 0, 0, log .1)
 *   out [ncell x 8] (fs, sd, prior sd, ell_x, ell_y, ell_t, sf2, sn2)
 *   status [ncell] as above at the fitted hypers; info [ncell x 4] or NULL:
 *   (nit, cg_status, nfev, n_objective_evals).  Other arguments as above. */
int oi_nystrom_fit_batch(const double* xyt, const double* y, const int64_t* offs, int64_t ncell,
                         const int64_t* sel, const int64_t* soffs, const double* x0,
                         const double* xs, double mean, double* out, int32_t* status,
                         int32_t* info, const oi_options* opts);

/* Nystrom fits as a stream of batches (continuous batching across calls, as
 * oi_session_* for the full GP): every submitted batch (oi_nystrom_fit_batch's
 * arguments; host copies of offs, sel, soffs, x0, xs are taken, DEVICE inputs
 * and all outputs must stay valid until the ticket completes) joins one queue;
 * up to OI_NYS_CAP (64) cells per stream group fit at once and finished cells
 * are replaced from the queue, so a batch's slowest cells overlap later
 * batches.  Per-cell results equal oi_nystrom_fit_batch's bit for bit.
 *   submit returns a ticket >= 0 (or a negative OI_E* code); wait runs rounds
 *   until the ticket completes (ticket < 0: all submitted work). */
typedef struct oi_nystrom_session oi_nystrom_session;
oi_nystrom_session* oi_nystrom_session_create(const oi_options* opts);
int64_t oi_nystrom_session_submit(oi_nystrom_session* s, const double* xyt, const double* y,
                                  const int64_t* offs, int64_t ncell, const int64_t* sel,
                                  const int64_t* soffs, const double* x0, const double* xs, double mean,
                                  double* out, int32_t* status, int32_t* info);
int oi_nystrom_session_wait(oi_nystrom_session* s, int64_t ticket);
void oi_nystrom_session_destroy(oi_nystrom_session* s);

/* ---- SVGP variant (dev/sparseGP_example.ipynb code cell 5: GPflow SVGP with a
 * Matern32 kernel, Gaussian likelihood, Constant mean, whitened q(u), trained
 * by TF2 Adam on minibatches, then predict_f) -- one workgroup per cell runs
 * the whole training in one launch --------------------------------------
 *   xyt [N x 3], y [N]: the cell's inputs and RAW outputs (the Constant mean
 *       function holds the prior mean, as in the notebook)
 *   Z0  [ncell x M x 3] initial inducing inputs (NB2: per-dimension linspace)
 *   init [ncell x 6]: lengthscales (3), kernel variance, noise variance, mean
 *   batch (<= 256) rows per minibatch, iterations Adam steps (TF2 Adam, lr),
 *   log_every: the notebook's training_loss() call after every log_every-th
 *       step (draws one extra minibatch; 0 = none); elbo [ncell x
 *       ceil(iterations/log_every)] receives those ELBO values (or NULL)
 *   seed: minibatch stream of cell c keyed by seed + c (a deterministic
 *       per-epoch permutation; tf.data's shuffle is not reproducible)
 *   xs [ncell x 3] targets; pred [ncell x 2] = predict_f mean, variance of f
 *   params [ncell x oi_svgp_param_count(M)] final unconstrained parameters
 *       (ls_raw[3], var_raw, lik_raw, c, Z[M x 3], q_mu[M], tril(q_sqrt)) or NULL
 *   status [ncell]: 1 if a K_uu Cholesky failed during training
 * 1 <= M <= 64. */
int32_t oi_svgp_param_count(int32_t M);
int oi_svgp_batch(const double* xyt, const double* y, const int64_t* offs, int64_t ncell,
                  const double* Z0, int32_t M, const double* init, int32_t batch,
                  int32_t iterations, int32_t log_every, uint64_t seed, double lr,
                  const double* xs, double* pred, double* params, double* elbo, int32_t* status,
                  const oi_options* opts);

/* A trained model put to use: GPflow's SVGP.predict_f / predict_y at any number
 * of targets per cell, from the `params` rows oi_svgp_batch returned (or any
 * rows of that layout).  Nothing is trained.
 *   params [ncell x oi_svgp_param_count(M)] host; 1 <= M <= 64
 *   xs     [T x 3]  targets of all cells, cell c owning rows
 *                   toffs[c] .. toffs[c+1]-1 (a device pointer with
 *                   opts->device_inputs); no target (nt = 0) is valid
 *   toffs  [ncell+1] target offsets, toffs[0] = 0, non-decreasing
 *   with_noise  0: predict_f;  1: predict_y of the Gaussian likelihood, i.e.
 *                   softplus(lik_raw) + 1e-6 added to var (cov must be NULL:
 *                   GPflow has no full-covariance predict_y)
 *   mean   [T]      c + A'q_mu,  A = L^-1 K_us,  L = chol(K_uu + 1e-6 I)
 *   var    [T]      kvar - sum A^2 + sum (q_sqrt' A)^2   (full_cov=False)
 *   cov    or NULL: K_ss - A'A + (S'A)'(S'A) in full, cell c's nt x nt matrix
 *                   row-major at offset sum_{k<c} nt_k^2; symmetric bit for
 *                   bit, its diagonal bit for bit `var` (the diagonal of K_ss
 *                   is kvar exactly); nt^2 doubles must stay below 2 GiB
 *   status [ncell]  0 ok, 1 the K_uu Cholesky met a pivot that is not positive
 *                   (non-finite parameters included): that cell's mean, var
 *                   and cov are NaN, the other cells are untouched
 * Cells are worked in chunks that fit opts->pool_bytes (0 => 60% of the free
 * HBM); a cell that does not fit alone is OI_E_NOMEM.  A result depends on the
 * cell and the target alone: not on the other cells or targets of the call,
 * the chunking, or host / device inputs. */
int oi_svgp_predict(const double* params, int32_t M, int64_t ncell, const double* xs,
                    const int64_t* toffs, int32_t with_noise, double* mean, double* var,
                    double* cov, int32_t* status, const oi_options* opts);

/* GPflow's model.elbo((X, Y)) on ALL of each cell's data at the given params:
 *   elbo[c] = sum_i [-log(2 pi)/2 - log(s2)/2 - ((y_i - mean_i)^2 + var_i)/(2 s2)]
 *             - (q_mu.q_mu + sum S^2 - M - sum log S_ii^2) / 2
 * -- the number two trained models are compared by (oi_svgp_batch's `elbo` log
 * holds minibatch estimates of it).
 *   xyt, y, offs as in oi_svgp_batch (device pointers with opts->device_inputs);
 *   every cell needs n >= 1.  status as above; a failed cell's elbo is NaN. */
int oi_svgp_elbo(const double* params, int32_t M, const double* xyt, const double* y,
                 const int64_t* offs, int64_t ncell, double* elbo, int32_t* status,
                 const oi_options* opts);

/* ---- host optimiser (scipy 1.15 CG restated; see csrc/cg.hpp) ---- */
typedef struct oi_cg oi_cg;
/* x0: 6 log-hypers. gtol/maxiter as in oi_options (maxiter < 0 => 1200). */
oi_cg* oi_cg_create(const double* x0, double gtol, int32_t maxiter);
/* Advance until the optimiser needs an objective value: returns 1 and writes
 * the requested point to x_req[6]; returns 0 when finished; <0 on misuse. */
int oi_cg_step(oi_cg* h, double* x_req);
/* Supply f and g[6] at the last requested point. */
int oi_cg_feed(oi_cg* h, double f, const double* g);
/* Result after oi_cg_step returned 0: x[6], fun, nit, status (scipy codes),
 * nfev/njev (scipy counters) and nobj (objective evaluations made). */
int oi_cg_result(oi_cg* h, double* x, double* fun, int32_t* nit, int32_t* status,
                 int64_t* nfev, int64_t* njev, int64_t* nobj);
void oi_cg_destroy(oi_cg* h);

/* ---- diagnostics ---- */
const char* oi_last_error(void);  /* thread-local message of the last failure */
int32_t oi_version(void);
/* JSON with per-kernel {launches, total_ms, flops} since the last reset
 * (requires opts.profile=1 on the timed calls). Returns bytes needed. */
int64_t oi_profile_json(char* buf, int64_t len);
void oi_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* OI_H */
