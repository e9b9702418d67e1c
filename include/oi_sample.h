/* liboi -- joint posterior draws per cell (C ABI).
 *
 * An entry point that include/oi.h does not declare itself; conventions,
 * error codes and oi_options are those of include/oi.h, which this header
 * includes.  Python: optimalinterpolation_amd/_lib.py binds it from
 * SIGNATURES_SAMPLE. */
#ifndef OI_SAMPLE_H
#define OI_SAMPLE_H

#include "oi.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif

#endif /* OI_SAMPLE_H */
