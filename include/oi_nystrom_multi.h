/* liboi -- the Nystrom prediction at many targets per cell (C ABI).
 *
 * The one entry point that include/oi.h does not declare itself; conventions,
 * error codes and oi_options are those of include/oi.h, which this header
 * includes.  Python: optimalinterpolation_amd/_lib.py binds it from
 * SIGNATURES_NYSTROM_MULTI. */
#ifndef OI_NYSTROM_MULTI_H
#define OI_NYSTROM_MULTI_H

#include "oi.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif

#endif /* OI_NYSTROM_MULTI_H */
