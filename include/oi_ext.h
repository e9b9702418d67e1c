/* liboi -- additions to the C ABI of oi.h.
 *
 * oi.h is closed at its 36 entry points; every later entry is declared here.
 * Conventions, options and error codes are oi.h's.
 *
 *   oi_gpr_predict_grad  the posterior of the field AND of its gradient
 *                        (df/dx, df/dy, df/dt) at many targets per cell, from
 *                        the one factorisation oi_gpr_predict_multi does.
 */
#ifndef OI_EXT_H
#define OI_EXT_H

#include "oi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Posterior of u = (f, df/dx, df/dy, df/dt) at many targets per cell, at given
 * LINEAR hypers.  The Matern-3/2 covariance k = sf2 (1 + Q) exp(-Q) of
 * SGPkernel (GPR:78-93) is twice differentiable in its argument, so the
 * derivative process exists, is jointly Gaussian with f and has the prior
 * variance 3 sf2 / ell_k^2.  With c_k = sqrt(3) / ell_k, d = c o (a - b),
 * Q = |d| and e = exp(-Q):
 *
 *   k(a, b)           = sf2 (1 + Q) e
 *   d k / d a_k       = -sf2 e d_k c_k              (0 at Q = 0)
 *   d k / d b_l       = +sf2 e d_l c_l
 *   d2 k / d a_k d b_l = sf2 e c_k c_l ((k == l) - d_k d_l / Q)   (d_k d_l / Q := 0 at Q = 0)
 *
 * C [(4 nt) x n] holds in row 4 t + k the covariance of component k of target
 * t with the observations, P [(4 nt) x (4 nt)] the joint prior, and
 *
 *   L = chol(K + sn2 I);  zt = L^-1 (z - mean);  V = L^-1 C'
 *   E[u] = (mean, 0, 0, 0) per target + V' zt;   Cov[u] = P - V'V
 *
 *   xyt, z, offs, xs, toffs, mean, hyp   as oi_gpr_predict_multi (device
 *                   pointers xyt / z with opts->device_inputs); a cell may be
 *                   empty, and a cell may have no targets
 *   grad   [T x 3]  posterior mean of (df/dx, df/dy, df/dt) at each target, in
 *                   the inputs' units (m/m, m/m, m/day)
 *   gsd    [T x 3]  their standard deviations, sqrt of the matching diagonal
 *                   entries of blk; NaN where the argument is negative, as
 *                   np.sqrt (no clamping)
 *   fs, sd [T] or NULL: bit for bit those of oi_gpr_predict_multi
 *   blk    [T x 16] or NULL: per target the 4 x 4 posterior covariance of u_t,
 *                   row-major, symmetric bit for bit
 *   cov    or NULL: Cov[u] of the whole cell, (4 nt) x (4 nt) with index
 *                   4 t + k, row-major, symmetric bit for bit, cell c's at
 *                   offset sum_{k<c} 16 nt_k^2
 *   status [ncell]  0 ok, 1 covariance not positive definite: every output of
 *                   that cell is NaN; the other cells are untouched
 * A cell with no observations gives the prior: grad = 0, gsd_k = sqrt(sf2
 * c_k^2), fs = mean, sd = sqrt(sf2), blk and cov = P.  OI_E_ARG, before any
 * device is touched: bad offs / toffs, null status / hyp, null xyt / z with
 * observations, null xs / grad / gsd with targets, a cell whose K, X ((4 nt +
 * 1) n doubles, or 4 nt + 1 alone) or, when asked for, cov (16 nt^2) reaches
 * 2 GiB.  Cells are worked in chunks that fit opts->pool_bytes; a cell that
 * does not fit alone is OI_E_NOMEM, with no output written.  A cell's results
 * depend neither on the other cells of the call nor on the chunking.
 * opts->profile records the stages pg_generate, pg_cholesky, pg_solve,
 * pg_reduce and pg_cov (oi_profile_json). */
int oi_gpr_predict_grad(const double* xyt, const double* z, const int64_t* offs, int64_t ncell,
                        const double* xs, const int64_t* toffs, double mean, const double* hyp,
                        double* grad, double* gsd, double* fs, double* sd,
                        double* blk, double* cov, int32_t* status, const oi_options* opts);

#ifdef __cplusplus
}
#endif

#endif /* OI_EXT_H */
