"""Leave-one-out cross-validation of one cell in plain numpy: the reference of
``oi_gpr_loo`` (tests/test_gpu_loo.py), on ``oracle.gp_oracle.matern32``.

``loo_closed`` evaluates the closed form (Rasmussen & Williams, GPML 5.4.2)
    r = z - mean, K~ = K + sn2 I = L L', alpha = K~^-1 r, q_i = [K~^-1]_ii
    mu_i = z_i - alpha_i / q_i, sd_i = sqrt(1 / q_i)
    lpl = sum_i [ -log(2 pi)/2 - log sd_i - (z_i - mu_i)^2 / (2 sd_i^2) ]
and ``loo_brute`` what it stands for: n fits of n - 1 observations, each
predicting the one held out (noise included).  Both return (mu [n], sd [n],
lpl) and let ``np.linalg.LinAlgError`` propagate.
"""
import numpy as np

from oracle import gp_oracle as O


def _split(hyp):
    return list(hyp[:3]), hyp[3], hyp[4]


def _lpl(z, mu, sd):
    return float(np.sum(-0.5 * np.log(2 * np.pi) - np.log(sd) - (z - mu) ** 2 / (2 * sd ** 2)))


def loo_closed(x, z, mean, hyp):
    ell, sf2, sn2 = _split(hyp)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    n = len(z)
    if n == 0:
        return np.zeros(0), np.zeros(0), 0.0
    L = np.linalg.cholesky(O.matern32(x, ell, sf2) + np.eye(n) * sn2)
    W = np.linalg.solve(L, np.eye(n))             # L^-1
    r = z - np.ones(n) * mean
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, r))
    q = (W * W).sum(axis=0)                       # q_i = sum_k (L^-1)_ki^2
    mu = z - alpha / q
    sd = np.sqrt(1 / q)
    return mu, sd, _lpl(z, mu, sd)


def loo_brute(x, z, mean, hyp):
    ell, sf2, sn2 = _split(hyp)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    n = len(z)
    K = O.matern32(x, ell, sf2) + np.eye(n) * sn2 if n else np.zeros((0, 0))
    np.linalg.cholesky(K)                         # a non-PD cell fails as a whole, as the closed form does
    mu, sd = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        if n == 1:                                # nothing left: the prior
            mu[i], sd[i] = mean, np.sqrt(sf2 + sn2)
            continue
        L = np.linalg.cholesky(K[np.ix_(keep, keep)])
        k = K[keep, i]
        A = np.linalg.solve(L.T, np.linalg.solve(L, z[keep] - mean))
        v = np.linalg.solve(L, k)
        mu[i] = mean + np.dot(k, A)
        sd[i] = np.sqrt(sf2 + sn2 - np.dot(v, v))
    return mu, sd, _lpl(z, mu, sd)
