/* liboi -- leave-one-out cross-validation per cell (C ABI).
 *
 * An entry point that include/oi.h does not declare itself; conventions,
 * error codes and oi_options are those of include/oi.h, which this header
 * includes.  Python: optimalinterpolation_amd/_lib.py binds it from
 * SIGNATURES_LOO. */
#ifndef OI_LOO_H
#define OI_LOO_H

#include "oi.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif

#endif /* OI_LOO_H */
