"""Shared cases for the tests of the Nystrom prediction at many targets
(tests/test_gpu_nystrom_predict_multi.py on the GPU,
tests/test_nystrom_predict_multi_wform.py on the CPU): the cells of
tests/nystrom_cases.py, a grid of targets OFF the observation sites, and the
float64 reference per case, built from the oracle's own functions and cached.
A plain module (tests import it); it holds no test.
"""
import numpy as np
from numpy.linalg import multi_dot as mdot

import nystrom_cases as NC
from nystrom_cases import N, matern32

# (n, M): with nt below, tile-row decodes of 1 / 2 / 3 tiles, off-diagonal
# tiles with mirrors, a partial last tile, 1..4 k-tiles for both products
SHAPES = ((5, 5), (70, 31), (129, 65), (130, 129), (193, 96))
HNAMES = ('H1', 'H2')
NTS = (1, 63, 64, 65, 130)
MEAN = NC.MEAN

# 162 targets (a + 12.5 km, b + 12.5 km, t), t in {3.5, 4.5}, a, b on the
# lattice's 9 x 9 grid, in the order t, a, b: none coincides with a site
_G = np.arange(-4, 5) * 25e3
TGRID = np.array([(a + 12.5e3, b + 12.5e3, t) for t in (3.5, 4.5) for a in _G for b in _G], dtype=np.float64)
assert TGRID.shape == (162, 3)


def targets(n, nt):
    """A case's nt targets: TGRID[default_rng(7 n + nt).permutation(162)[:nt]]."""
    return TGRID[np.random.default_rng(7 * n + nt).permutation(162)[:nt]]


def linear(hname):
    """(ell [3], sf2, sn2) of NC.HYPERS[hname]."""
    h = np.exp(NC.HYPERS[hname])
    return list(h[:3]), float(h[3]), float(h[4])


def case_cell(n, M):
    return NC.cell(n, NC.cell_seed(n, M))


_KI = {}    # (n, M, hname) -> (Ki, A) of the oracle
_REF = {}   # (n, M, hname, nt) -> (fs_ref [nt], cov_ref [nt x nt])


def reference(n, M, hname, nt):
    """(fs_ref, cov_ref) of the oracle's functions at the case's targets:
    Ki, A = nystroem(...); k = matern32(x, xs=xs);
    cov_ref = matern32(xs) - k' Ki k; fs_ref = MEAN + k' A.  Computed once."""
    key = (n, M, hname, nt)
    if key not in _REF:
        ell, sf2, sn2 = linear(hname)
        x, y = case_cell(n, M)
        if key[:3] not in _KI:
            _KI[key[:3]] = N.nystroem(x, y, M=M, ell=ell, sf2=sf2, sn2=sn2)
        Ki, A = _KI[key[:3]]
        xs = targets(n, nt)
        k = matern32(x, ell, sf2, xs=xs)
        cov = matern32(xs, ell, sf2) - mdot([k.T, Ki, k])
        fs = MEAN + np.dot(k.T, A).ravel()
        for a in (fs, cov):
            a.setflags(write=False)
        _REF[key] = (fs, cov)
    return _REF[key]


def wform(x, y, xs, ell, sf2, sn2, M):
    """(fs - MEAN + MEAN, cov) by the algebra of oi_nystrom_predict_multi in
    NumPy: W' = C L^-T, A = y / sn2 - W'(W y), V = W Kxsx,
    cov = Kxs - (Kxsx'Kxsx / sn2 - V'V)."""
    n = len(y)
    sel = N.inducing_indices(n, M)
    Kmm = matern32(x[sel, :], ell, sf2)
    Knm = matern32(x, ell, sf2, xs=x[sel, :])
    s, u = np.linalg.eigh(Kmm)
    s[s <= 0] = 1e-12
    st = n * s / M
    ut = np.sqrt(M / n) * np.dot(Knm, u) / s
    C = ut / sn2
    L = np.linalg.cholesky(np.diag(1 / st) + np.dot(ut.T, C))
    W = np.linalg.solve(L, C.T)                       # M x n
    A = y / sn2 - np.dot(W.T, np.dot(W, y))
    k = matern32(x, ell, sf2, xs=xs)                  # n x nt
    V = np.dot(W, k)
    cov = matern32(xs, ell, sf2) - (np.dot(k.T, k) / sn2 - np.dot(V.T, V))
    return MEAN + np.dot(k.T, A), cov
