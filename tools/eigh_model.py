"""NumPy model of the hand-written batched eigensolver (csrc/oi_linalg.hip)
used by the Nystrom variant in place of LAPACK/rocSOLVER syevd
(GP_example.ipynb's ``np.linalg.eigh(Kmm)``): the same algorithm step for
step, so its accuracy can be checked against numpy on the CPU before the
kernels run.

  1. blocked Householder tridiagonalisation (LAPACK dsytrd / dlatrd, lower):
     panels of NBT columns, per column the symv with the panel's corrections,
     rank-2 NBT trailing update per panel; V (unit lower) and T (dlarft,
     forward columnwise) kept per panel for the back-transform;
  2. eigenvalues of the tridiagonal by bisection on Sturm counts (dstebz);
  3. eigenvectors of the tridiagonal by inverse iteration with partial
     pivoting (dlagtf / dlagts), a pseudo-random start per eigenvalue;
  4. block classical Gram-Schmidt twice (BCGS2) over blocks of 128 and
     panels of 32 vectors,
     Cholesky QR twice inside a panel; where a column keeps little of its
     norm (numerically repeated eigenvalues) Gram-Schmidt column by column: a
     weak column is projected out of every earlier column, a collapsed one is
     replaced by a fresh start vector put through inverse iteration (dstein
     inside a cluster);
  5. back-transform U = Q Z, one block reflector I - V T V' per panel.
"""
import numpy as np

NBT = 32


def sytrd(A0, nbt=NBT):
    A = np.array(A0, dtype=float)
    M = A.shape[0]
    d, e, tau = np.zeros(M), np.zeros(max(M - 1, 0)), np.zeros(max(M - 1, 0))
    panels = []
    p = 0
    while p < M - 1:
        nb = min(nbt, M - 1 - p)
        V = np.zeros((M, nb))
        W = np.zeros((M, nb))
        for i in range(nb):
            g = p + i
            # (1) bring column g up to date with the panel so far (rows g..M-1)
            if i > 0:
                A[g:, g] -= V[g:, :i] @ W[g, :i] + W[g:, :i] @ V[g, :i]
            # (2) reflector annihilating A(g+2:, g)
            alpha = A[g + 1, g]
            xn = np.sqrt(np.sum(A[g + 2:, g] ** 2))
            if xn == 0.0:
                t, beta = 0.0, alpha
                v = np.zeros(M)
                v[g + 1] = 1.0
            else:
                beta = -np.copysign(np.hypot(alpha, xn), alpha)
                t = (beta - alpha) / beta
                v = np.zeros(M)
                v[g + 1] = 1.0
                v[g + 2:] = A[g + 2:, g] / (alpha - beta)
            e[g], tau[g] = beta, t
            d[g] = A[g, g]
            # (3) w = tau (A22 v - V (W'v) - W (V'v)); w += -tau/2 (w'v) v
            L = np.tril(A[g + 1:, g + 1:])
            A22 = L + np.tril(L, -1).T
            y = A22 @ v[g + 1:]
            wv_, vv_ = W[g + 1:, :i].T @ v[g + 1:], V[g + 1:, :i].T @ v[g + 1:]
            # w'v from the dots (round 5, k_sy_w: no reduction over w):
            # w'v = tau (y'v - 2 (W'v).(V'v))
            a2 = -0.5 * t * (t * (y @ v[g + 1:] - 2.0 * (wv_ @ vv_)))
            y -= V[g + 1:, :i] @ wv_ + W[g + 1:, :i] @ vv_
            w = np.zeros(M)
            w[g + 1:] = t * y + a2 * v[g + 1:]
            V[:, i], W[:, i] = v, w
        # trailing update (rows / columns from p + nb)
        q = p + nb
        A[q:, q:] -= V[q:] @ W[q:].T + W[q:] @ V[q:].T
        # T of the block reflector: H_p ... H_{p+nb-1} = I - V T V'
        T = np.zeros((nb, nb))
        for i in range(nb):
            T[i, i] = tau[p + i]
            if i:
                T[:i, i] = -tau[p + i] * (T[:i, :i] @ (V[:, :i].T @ V[:, i]))
        panels.append((p, V, T))
        p = q
    d[M - 1] = A[M - 1, M - 1]
    return d, e, panels


def sturm_count(d, e2, x, pivmin):
    """#eigenvalues < x, for every entry of the vector x at once."""
    q = d[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    c = (q < 0).astype(int)
    for i in range(1, len(d)):
        q = d[i] - x - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        c += q < 0
    return c


def stebz(d, e):
    M = len(d)
    e2 = e ** 2
    ae = np.abs(np.r_[0.0, e]) + np.abs(np.r_[e, 0.0])
    gl, gu = np.min(d - ae), np.max(d + ae)
    tnorm = max(abs(gl), abs(gu))
    pivmin = np.finfo(float).tiny * max(1.0, np.max(e2) if M > 1 else 1.0)
    gl -= 2.1 * tnorm * np.finfo(float).eps * M + 2.1 * pivmin
    gu += 2.1 * tnorm * np.finfo(float).eps * M + 2.1 * pivmin
    eps = np.finfo(float).eps
    # eigenvalue k (0-based): count(x) <= k  <=>  x <= lambda_k; the M
    # bisections run side by side (each one's steps are those of a scalar loop)
    k = np.arange(M)
    lo, hi = np.full(M, gl), np.full(M, gu)
    live = np.ones(M, dtype=bool)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        live &= ~((hi - lo <= 2 * eps * np.maximum(np.abs(lo), np.abs(hi)) + pivmin) | (mid == lo) | (mid == hi))
        if not live.any():
            break
        below = sturm_count(d, e2, mid, pivmin) <= k
        lo = np.where(live & below, mid, lo)
        hi = np.where(live & ~below, mid, hi)
    return 0.5 * (lo + hi), tnorm


def start_vector(k, M):
    i = np.arange(M, dtype=np.uint64)
    with np.errstate(over='ignore'):  # arithmetic modulo 2^64, as the kernel's
        h = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(k + 1) * np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(31)
        h = h * np.uint64(0x94D049BB133111EB)
    h ^= h >> np.uint64(29)
    return (h >> np.uint64(11)).astype(float) / 2.0 ** 53 * 2.0 - 1.0


def lagtf(d, e, lam):
    """T - lam I = P L U (dlagtf): a diag of U, b first / c second superdiagonal, l multipliers, piv.
    lam may be a vector: the factors are then M x len(lam), one column per shift."""
    M = len(d)
    lam = np.atleast_1d(np.asarray(lam, dtype=float))
    K = len(lam)
    a = d[:, None] - lam[None, :]
    b = np.repeat(np.r_[e, 0.0][:, None], K, axis=1)
    c = np.zeros((M, K))
    l = np.zeros((M, K))
    piv = np.zeros((M, K), dtype=bool)
    sub = np.r_[e, 0.0]
    for k in range(M - 1):
        keep = np.abs(a[k]) >= np.abs(sub[k])
        with np.errstate(divide='ignore', invalid='ignore'):
            m_keep = np.where(a[k] != 0.0, sub[k] / a[k], 0.0)
            m_swap = a[k] / sub[k]
        l[k] = np.where(keep, m_keep, m_swap)
        piv[k] = ~keep
        t = a[k + 1].copy()
        with np.errstate(invalid='ignore'):  # the branch not taken may be inf * 0
            a[k + 1] = np.where(keep, t - m_keep * b[k], b[k] - m_swap * t)
            a[k] = np.where(keep, a[k], sub[k])
            if k < M - 2:
                c[k] = np.where(keep, 0.0, b[k + 1])
                b[k + 1] = np.where(keep, b[k + 1], -m_swap * b[k + 1])
        b[k] = np.where(keep, b[k], t)
    return a, b, c, l, piv


def lagts(a, b, c, l, piv, y, tol):
    """Solve with the factors of lagtf (dlagts, job = -1: tiny pivots perturbed to
    +-tol); y is M x K like the factors (or a vector for a single shift)."""
    M = len(a)
    vec = y.ndim == 1
    y = np.array(y.reshape(M, -1), dtype=float)
    for k in range(M - 1):
        yk, yn = y[k].copy(), y[k + 1].copy()
        y[k] = np.where(piv[k], yn, yk)
        y[k + 1] = np.where(piv[k], yk - l[k] * yn, yn - l[k] * yk)
    for k in range(M - 1, -1, -1):
        t = y[k]
        if k < M - 1:
            t = t - b[k] * y[k + 1]
        if k < M - 2:
            t = t - c[k] * y[k + 2]
        ak = np.where(np.abs(a[k]) < tol, np.where(a[k] >= 0, tol, -tol), a[k])
        y[k] = t / ak
    return y[:, 0] if vec else y


def stein(d, e, lam, tnorm, iters=2):
    M = len(d)
    eps = np.finfo(float).eps
    tol = max(eps * tnorm, np.finfo(float).tiny)  # T == 0: no division by zero
    f = lagtf(d, e, lam)
    X = np.stack([start_vector(k, M) for k in range(M)], axis=1)
    for _ in range(iters):
        X = lagts(*f, X, tol)
        X /= np.max(np.abs(X), axis=0)
    return X / np.linalg.norm(X, axis=0)


MGS_ITERS = 3   # inverse iterations of a replacement column (k_mgs_panel)
WEAK = 1e-2     # a column keeping <= this much of its squared norm inside its panel is "weak"
COLLAPSE = 1e-4  # ... and one keeping <= this much has collapsed


def mgs(Z, p, q, tri=None):
    """Columns [p, q) of Z (orthogonal to the columns < p up to rounding):
    classical Gram-Schmidt twice against the panel's earlier columns, normalise
    (k_mgs_panel).

    A WEAK column lost most of its norm to its cluster mates in the panel, and
    normalising it magnifies what rounding left in it of other eigenvectors (by
    1 / sqrt(fraction kept)); one that COLLAPSES (a numerically repeated
    eigenvalue: inverse iteration gave a vector in the span of the earlier
    ones) has nothing left to keep.

    In the bottom cluster (stein's random starts, the last columns) the
    complement of every earlier column IS the eigenspace: a weak column is
    projected out of EVERY earlier column before it is normalised, a collapsed
    one replaced by a fresh start vector treated the same way.

    Anywhere else such a vector lies in the span of ALL remaining eigenvectors
    (the defect of the first version: an orthonormal basis that is no
    eigenbasis, residual O(||A||)), so a weak or collapsed column is replaced
    as LAPACK's dstein does inside a cluster: a fresh start vector, projected
    out of every earlier column, put through inverse iteration on T - lam_j I
    and projected again, MGS_ITERS times -- an eigenvector of lam_j orthogonal
    to the earlier columns.

    tri = (d, e, lam_of_column, tnorm, nb0); without it the first version."""
    M = Z.shape[0]

    def project(x, lo, j):
        for _ in range(2):
            x = x - Z[:, lo:j] @ (Z[:, lo:j].T @ x)
        return x

    for j in range(p, q):
        bottom = tri is None or M - 1 - j < tri[4]
        for attempt in range(4):
            n0 = Z[:, j] @ Z[:, j]
            Z[:, j] = project(Z[:, j], p if attempt == 0 else 0, j)
            n1 = Z[:, j] @ Z[:, j]
            if n1 > (COLLAPSE if bottom else WEAK) * n0 and n1 > 0.0:
                if tri is not None and attempt == 0 and p > 0 and not n1 > WEAK * n0:
                    Z[:, j] = project(Z[:, j], 0, j)
                    n1 = Z[:, j] @ Z[:, j]
                Z[:, j] /= np.sqrt(n1)
                break
            x = start_vector(j + 7919 * (attempt + 1), M)
            if not bottom:
                d, e, lamc, tnorm = tri[:4]
                x = project(x, 0, j)
                f = tuple(u[:, 0] for u in lagtf(d, e, lamc[j]))
                for _ in range(MGS_ITERS):
                    x = lagts(*f, x, max(np.finfo(float).eps * tnorm, np.finfo(float).tiny))
                    x = x / np.max(np.abs(x))
                    x = project(x, 0, j)
            Z[:, j] = x


def cholqr2(Z, p, q, tri=None):
    """Z[:, p:q] <- Q of its QR, twice (k_orth_panel).  False when mgs has to
    take the panel: a pivot keeps <= COLLAPSE of its column's squared norm, or
    <= WEAK above the bottom cluster (the column is replaced); Z is then
    unchanged by the failing pass.  A weak column of the bottom cluster keeps
    the panel and is projected once more out of every earlier column
    afterwards (k_mgs_panel, flag 2).  tri = None: the first version."""
    M = Z.shape[0]
    weak = []
    for _ in range(2):
        G = Z[:, p:q].T @ Z[:, p:q]
        R = np.triu(G).copy()
        nb = q - p
        for j in range(nb):
            if not R[j, j] > COLLAPSE * G[j, j]:
                return False
            if tri is not None and not R[j, j] > WEAK * G[j, j]:
                if not M - 1 - (p + j) < tri[4]:
                    return False
                if p > 0 and p + j not in weak:
                    weak.append(p + j)
            R[j, j] = np.sqrt(R[j, j])
            R[j, j + 1:] /= R[j, j]
            R[j + 1:, j + 1:] -= np.triu(np.outer(R[j, j + 1:], R[j, j + 1:]))
        Z[:, p:q] = Z[:, p:q] @ np.linalg.inv(R)
    for j in sorted(weak):
        Z[:, j] -= Z[:, :j] @ (Z[:, :j].T @ Z[:, j])
        Z[:, j] /= np.sqrt(Z[:, j] @ Z[:, j])
    return True


def bcgs2(Z, nb=32, ob=128, tri=None):
    """Two-level BCGS2 (round 5, OI_ORTH_BLOCK = ob): each ob-column block
    projected out of every earlier block twice, then BCGS2 between its
    nb-column panels; ob = nb is plain panel-wise BCGS2."""
    M, K = Z.shape
    Z = Z.copy()

    def project(lo, p, q):
        for _ in range(2):
            H = Z[:, lo:p].T @ Z[:, p:q]
            Z[:, p:q] -= Z[:, lo:p] @ H

    for P in range(0, K, ob):
        Q = min(K, P + ob)
        if P > 0:
            project(0, P, Q)
        for p in range(P, Q, nb):
            q = min(K, p + nb)
            if p > P:
                project(P, p, q)
            if not cholqr2(Z, p, q, tri):
                mgs(Z, p, q, tri)
    return Z


def ormtr(panels, Z):
    U = Z.copy()
    for p, V, T in reversed(panels):
        U -= V @ (T @ (V.T @ U))
    return U


def eigh(A, fix=True):
    """fix=False: the replacement of a collapsed column as it was before the
    inverse-iteration step (wrong for clusters above the bottom of the spectrum)."""
    d, e, panels = sytrd(A)
    lam, tnorm = stebz(d, e)
    Z = stein(d, e, lam, tnorm)
    # the bottom cluster (consecutive gaps <= 1e3 eps ||T||): random starts, no
    # inverse iteration; orthogonalisation in descending eigenvalue order
    eps = np.finfo(float).eps
    nb0 = 1
    while nb0 < len(lam) and lam[nb0] - lam[nb0 - 1] <= 1e3 * eps * tnorm:
        nb0 += 1
    if nb0 >= 2:
        for k in range(nb0):
            x = start_vector(k, len(lam))
            Z[:, k] = x / np.linalg.norm(x)
    Z = bcgs2(Z[:, ::-1], tri=(d, e, lam[::-1], tnorm, nb0 if nb0 >= 2 else 0) if fix else None)[:, ::-1]
    return lam, ormtr(panels, Z)


if __name__ == '__main__':
    import sys
    sys.path.insert(0, '.')
    from scipy.spatial.distance import pdist, squareform
    rng = np.random.default_rng(0)
    for M, ell, dup in ((70, 3e4, False), (160, 6e4, False), (200, 2e5, True), (300, 9e4, False),
                        (240, 4e5, True), (260, 1e6, False)):
        g = np.arange(-12, 13) * 25e3
        sites = np.array([(a, b, t) for a in g for b in g for t in range(9)])
        x = sites[rng.choice(len(sites), M, replace=False)]
        if dup:
            x[M // 2:M // 2 + 10] = x[:10]
        Q = squareform(pdist(np.sqrt(3) * x / np.array([ell, ell, 3.0])))
        A = 6e-3 * (1 + Q) * np.exp(-Q)
        lam, U = eigh(A)
        s, u = np.linalg.eigh(A)
        nrm = np.abs(s).max()
        orth = np.abs(U.T @ U - np.eye(M)).max()
        res = np.abs(A @ U - U * lam).max() / nrm
        # invariant: the clamped pseudo-inverse NB1 uses
        def pinv(ss, uu):
            ss = ss.copy()
            ss[ss <= 0] = 1e-12
            return (uu / ss) @ uu.T
        good = s > 1e-8 * nrm
        print(f"M={M} dup={dup}: eigenvalue err {np.abs(lam - s).max() / nrm:.2e}, orth {orth:.2e}, "
              f"residual {res:.2e}, cond {nrm / s[good].min():.1e}")
