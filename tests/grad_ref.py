"""The posterior of a cell's field and of its gradient in plain numpy: the
reference of ``oi_gpr_predict_grad`` (include/oi_ext.h;
tests/test_gpu_predict_grad.py), its ragged batch and the checks against it.

For target t the joint vector is u_t = (f, df/dx, df/dy, df/dt)(xs_t),
component k = 0..3, index 4 t + k.  With c_k = sqrt(3) / ell_k,
d = c o (a - b), Q = |d| and e = exp(-Q):

    k(a, b)            = sf2 (1 + Q) e
    d k / d a_k        = -sf2 e d_k c_k
    d k / d b_l        = +sf2 e d_l c_l
    d2 k / d a_k d b_l = sf2 e c_k c_l ((k == l) - d_k d_l / Q)     (d_k d_l / Q := 0 at Q = 0)

    L = chol(K + sn2 I),  zt = L^-1 (z - mean),  V = L^-1 C'
    E[u] = (mean, 0, 0, 0) per target + V' zt,   Cov[u] = P - V'V

``K`` is ``oracle.gp_oracle.matern32``; the value rows of ``C`` repeat its
cross-covariance expression (tests/test_grad_ref.py compares them).
"""
import numpy as np
from scipy.spatial.distance import cdist

from oracle import gp_oracle as O

RTOL = 1e-10        # T1, as tests/test_gpu_predict_multi.py
MIN_RATIO = 1e-4    # posterior / prior variance every input must keep, so that every sd is well conditioned


def joint_cov(a, b, ell, sf2):
    """[na x 4 x nb x 4]: the covariance of u_k(a_i) with u_l(b_j)."""
    ell = np.asarray(ell, dtype=np.float64)
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    c = O.SQRT3 / ell
    sa, sb = O.SQRT3 * a / ell, O.SQRT3 * b / ell
    J = np.zeros((len(a), 4, len(b), 4))
    if len(a) == 0 or len(b) == 0:
        return J
    Q = cdist(sa, sb, 'euclidean')
    e = np.exp(-Q)
    d = sa[:, None, :] - sb[None, :, :]
    J[:, 0, :, 0] = sf2 * ((1 + Q) * e)
    for k in range(3):
        J[:, k + 1, :, 0] = -sf2 * e * d[:, :, k] * c[k]
        J[:, 0, :, k + 1] = sf2 * e * d[:, :, k] * c[k]
        for l in range(3):
            with np.errstate(invalid='ignore', divide='ignore'):
                r = np.where(Q > 0, d[:, :, k] * d[:, :, l] / Q, 0.0)
            J[:, k + 1, :, l + 1] = sf2 * e * (c[k] * c[l]) * ((1.0 if k == l else 0.0) - r)
    return J


def cross(x, xs, ell, sf2):
    """C [4 nt x n]: row 4 t + k is the covariance of u_k(xs_t) with the observations."""
    return joint_cov(xs, x, ell, sf2)[:, :, :, 0].reshape(4 * len(xs), len(x))


def prior(xs, ell, sf2):
    """P [4 nt x 4 nt]."""
    return joint_cov(xs, xs, ell, sf2).reshape(4 * len(xs), 4 * len(xs))


def scales(hyp):
    """s = (sqrt(sf2), sqrt(3 sf2) / ell_x, sqrt(3 sf2) / ell_y, sqrt(3 sf2) / ell_t): the prior sd of u's components."""
    hyp = np.asarray(hyp, dtype=np.float64)
    return np.concatenate([[np.sqrt(hyp[3])], np.sqrt(3 * hyp[3]) / hyp[:3]])


def ref_cell(x, y, xs, mean, hyp):
    """(mean4 [4 nt], J [4 nt x 4 nt]) of one cell; LinAlgError propagates."""
    ell, sf2, sn2 = list(hyp[:3]), hyp[3], hyp[4]
    x, xs = np.asarray(x, dtype=np.float64).reshape(-1, 3), np.asarray(xs, dtype=np.float64).reshape(-1, 3)
    n, nt = len(y), len(xs)
    base = np.tile([mean, 0.0, 0.0, 0.0], nt)
    P = prior(xs, ell, sf2)
    if n == 0:
        return base, P
    L = np.linalg.cholesky(O.matern32(x, ell, sf2) + np.eye(n) * sn2)
    if nt == 0:
        return base, P
    zt = np.linalg.solve(L, y - np.ones(n) * mean)
    V = np.linalg.solve(L, cross(x, xs, ell, sf2).T)
    return base + np.dot(V.T, zt), P - np.dot(V.T, V)


def lattice(centre, nt, spacing=25e3):
    """nt targets on a square lattice (25 km) centred on ``centre``, at its t."""
    side = int(np.ceil(np.sqrt(max(nt, 1))))
    g = (np.arange(side) - (side - 1) / 2) * spacing
    gx, gy = np.meshgrid(g, g, indexing='ij')
    p = np.stack([centre[0] + gx.ravel(), centre[1] + gy.ravel(), np.full(side * side, centre[2])], axis=1)
    return p[:nt]


class Batch:
    """A ragged batch with a list of targets per cell, and its reference."""

    def __init__(self, cells, mean):
        # cells: list of (x [n x 3], y [n], xs [nt x 3], hyp [5])
        self.cells = cells
        self.mean = float(mean)
        self.xyt = np.ascontiguousarray(np.concatenate([c[0].reshape(-1, 3) for c in cells]))
        self.z = np.concatenate([c[1] for c in cells])
        self.xs = np.ascontiguousarray(np.concatenate([c[2].reshape(-1, 3) for c in cells]))
        self.offs = np.concatenate([[0], np.cumsum([len(c[1]) for c in cells])]).astype(np.int64)
        self.toffs = np.concatenate([[0], np.cumsum([len(c[2]) for c in cells])]).astype(np.int64)
        self.hyp = np.stack([c[3] for c in cells])
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = [ref_cell(c[0], c[1], c[2], self.mean, c[3]) for c in self.cells]
        return self._ref

    def run(self, blk=True, cov=True, **kw):
        from optimalinterpolation_amd import _lib
        return _lib.gpr_predict_grad(self.xyt, self.z, self.offs, self.xs, self.toffs, self.mean, self.hyp, blk=blk,
                                     cov=cov, **kw)

    def subset(self, idx):
        return Batch([self.cells[i] for i in idx], self.mean)


def same(a, b):
    """Bit for bit (NaN equal to NaN; None equal to None)."""
    return all((x is None and y is None) or
               (x is not None and y is not None and np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True))
               for x, y in zip(a, b))


def cell_slices(b, res, c):
    """Cell c's part of a result of ``Batch.run(blk=True, cov=True)``, as run returns it for the cell alone."""
    from optimalinterpolation_amd import _lib
    grad, gsd, fs, sd, blk, cov, st = res
    t0, t1 = b.toffs[c], b.toffs[c + 1]
    return (grad[t0:t1], gsd[t0:t1], fs[t0:t1], sd[t0:t1], blk[t0:t1], _lib.split_jcov(cov, b.toffs)[c].ravel(),
            st[c:c + 1])


def well_conditioned(b):
    """The condition every input of the GPU tests keeps: on the reference, the
    smallest posterior / prior variance ratio over all components."""
    worst = np.inf
    for c, (_, J) in enumerate(b.ref()):
        if len(J):
            s = np.tile(scales(b.hyp[c]), len(J) // 4)
            worst = min(worst, (J.diagonal() / (s * s)).min())
    return worst


def check_against_ref(b, res):
    """Every output of a run with blk and cov within the bounds of the
    reference: mean components and sd |gpu - ref| <= RTOL max(s_k, |ref|),
    blk / cov entries <= RTOL max(s_a s_b, |ref|).  Prints and returns the
    worst scaled errors (mean, sd, blk, cov)."""
    from optimalinterpolation_amd import _lib
    grad, gsd, fs, sd, blk, cov, st = res
    covs = _lib.split_jcov(cov, b.toffs)
    assert not st.any()
    worst = np.zeros(4)
    for c, (rm, rJ) in enumerate(b.ref()):
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        nt = t1 - t0
        s = scales(b.hyp[c])
        s4 = np.tile(s, nt)
        m4 = np.concatenate([fs[t0:t1, None], grad[t0:t1]], axis=1).ravel()
        sd4 = np.concatenate([sd[t0:t1, None], gsd[t0:t1]], axis=1).ravel()
        rsd4 = np.sqrt(rJ.diagonal())
        rblk = np.stack([rJ[4 * t:4 * t + 4, 4 * t:4 * t + 4] for t in range(nt)]) if nt else np.zeros((0, 4, 4))
        dblk = np.stack([covs[c][4 * t:4 * t + 4, 4 * t:4 * t + 4] for t in range(nt)]) if nt else np.zeros((0, 4, 4))
        e = [np.abs(m4 - rm) / np.maximum(s4, np.abs(rm)),
             np.abs(sd4 - rsd4) / np.maximum(s4, np.abs(rsd4)),
             np.abs(blk[t0:t1] - rblk) / np.maximum(np.outer(s, s), np.abs(rblk)),
             np.abs(covs[c] - rJ) / np.maximum(np.outer(s4, s4), np.abs(rJ)),
             np.abs(dblk - rblk) / np.maximum(np.outer(s, s), np.abs(rblk))]
        w = np.array([v.max(initial=0.0) for v in e])
        print(f"cell {c}: n {len(b.cells[c][1])} nt {nt} scaled |dmean| {w[0]:.3e} |dsd| {w[1]:.3e} "
              f"|dblk| {w[2]:.3e} |dcov| {w[3]:.3e}")
        for v in e:
            assert not np.isnan(v).any() and np.all(v <= RTOL), c
        worst = np.maximum(worst, w[:4])
    print("worst scaled errors (mean, sd, blk, cov):", ' '.join(f"{v:.3e}" for v in worst))
    return worst
