"""Helpers for the direct tests of the batched fp64 linear algebra
(csrc/oi_linalg.h through csrc/oi_linalg_abi.cpp): ctypes mirrors of the
descriptors, operand buffers with NaN padding and sentinels, matrix generators,
and references / checkers formed in np.longdouble on the host -- never with the
code under test.  A plain module (tests import it), not a conftest."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)      # 2^-52: twice the unit round-off
# pad rows and guard bands: a quiet NaN with a payload -- a read of it shows up
# as NaN in the result, a write over it changes its bits
SENT_BITS = np.uint64(0x7FF85EED0BADC0DE)
SENT = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]
GUARD = 2                                   # guard columns after an operand's last column


# ------------------------------------------------------------- descriptors --
c_dp = ctypes.c_void_p   # device pointers travel as integers


class Gemm(ctypes.Structure):
    _fields_ = [('A', c_dp), ('B', c_dp), ('C', c_dp), ('m', ctypes.c_int), ('n', ctypes.c_int),
                ('k', ctypes.c_int), ('lda', ctypes.c_int), ('ldb', ctypes.c_int), ('ldc', ctypes.c_int),
                ('alpha', ctypes.c_double), ('beta', ctypes.c_double), ('tri', ctypes.c_int)]


class Gemv(ctypes.Structure):
    _fields_ = [('A', c_dp), ('x', c_dp), ('y', c_dp), ('m', ctypes.c_int), ('n', ctypes.c_int),
                ('lda', ctypes.c_int), ('alpha', ctypes.c_double), ('beta', ctypes.c_double)]


class Chol(ctypes.Structure):
    _fields_ = [('A', c_dp), ('dinv', c_dp), ('info', c_dp), ('M', ctypes.c_int), ('lda', ctypes.c_int)]


class TrsmRLT(ctypes.Structure):
    _fields_ = [('X', c_dp), ('L', c_dp), ('dinv', c_dp), ('m', ctypes.c_int), ('M', ctypes.c_int),
                ('ldx', ctypes.c_int), ('ldl', ctypes.c_int)]


class Eigh(ctypes.Structure):
    _fields_ = [('A', c_dp), ('w', c_dp), ('work', c_dp), ('M', ctypes.c_int), ('lda', ctypes.c_int),
                ('info', c_dp)]


STRUCTS = (Gemm, Gemv, Chol, TrsmRLT, Eigh)   # oila_test_sizeof(which) in this order

_lib = None


def lib():
    """liboi.so with the oila_test_* entry points bound."""
    global _lib
    if _lib is None:
        from optimalinterpolation_amd import _lib as L
        h = L.load()
        for name, st in (('gemm', Gemm), ('gemv', Gemv), ('cholesky', Chol), ('trsm_right_lt', TrsmRLT),
                         ('eigh', Eigh)):
            f = getattr(h, 'oila_test_' + name)
            extra = {'gemm': [ctypes.c_int, ctypes.c_int], 'gemv': [ctypes.c_int]}.get(name, [])
            f.argtypes = [ctypes.POINTER(st), ctypes.c_int] + extra + [ctypes.c_void_p]
            f.restype = ctypes.c_int
        h.oila_test_sizeof.argtypes = [ctypes.c_int]
        h.oila_test_sizeof.restype = ctypes.c_int
        h.oila_test_eigh_workspace_doubles.argtypes = [ctypes.c_int]
        h.oila_test_eigh_workspace_doubles.restype = ctypes.c_longlong
        _lib = h
    return _lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


def _call(name, descs, *extra):
    h = lib()
    arr = (type(descs[0]) * len(descs))(*descs) if descs else None
    rc = getattr(h, 'oila_test_' + name)(arr, len(descs), *extra, _stream())
    if rc != 0:
        raise RuntimeError(f"oila_test_{name}: {rc}: {h.oi_last_error().decode(errors='replace')}")


def run_gemm(descs, ta, tb):
    _call('gemm', descs, int(ta), int(tb))


def run_gemv(descs, trans):
    _call('gemv', descs, int(trans))


def run_cholesky(descs):
    _call('cholesky', descs)


def run_trsm(descs):
    _call('trsm_right_lt', descs)


def run_eigh(descs):
    _call('eigh', descs)


# ----------------------------------------------------------------- buffers --
class DevMat:
    """A column-major rows x cols operand embedded in a larger device buffer:
    lda = rows + pad, GUARD further columns; pad rows and guard band hold SENT
    (a NaN).  ``host`` keeps what was uploaded."""

    def __init__(self, X, pad=0, fill=None):
        import torch
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        self.rows, self.cols = X.shape
        self.ld = max(self.rows + pad, 1)
        self.host = np.full((self.ld, self.cols + GUARD), SENT, order='F')
        self.host[:self.rows, :self.cols] = X if fill is None else fill
        self.dev = torch.from_numpy(np.ascontiguousarray(self.host.T)).cuda()

    def ptr(self, i=0, j=0):
        return self.dev.data_ptr() + 8 * (i + self.ld * j)

    def fetch(self):
        """(operand region, whole buffer) as on the device now."""
        import torch
        torch.cuda.synchronize()
        buf = self.dev.cpu().numpy().T
        return buf[:self.rows, :self.cols].copy(), buf

    def result(self):
        """The operand region after a run; asserts that pad rows and guard band
        kept their bits (no write outside the operand)."""
        reg, buf = self.fetch()
        bits = buf.view(np.uint64)
        assert (bits[self.rows:, :] == SENT_BITS).all(), "write into the pad rows"
        assert (bits[:, self.cols:] == SENT_BITS).all(), "write into the guard band"
        return reg


def dev_ints(values):
    import torch
    return torch.tensor(list(values), dtype=torch.int32).cuda()


# ------------------------------------------------------------ GEMM / GEMV --
def gemm_ref(opA, opB, C0, alpha, beta):
    """alpha op(A) op(B) + beta C0 and the elementwise bound
    (k + 4) 2^-52 (|alpha| |op A| |op B| + |beta| |C0|) in longdouble: the gamma
    bound of a length-k FMA sum in any order (2^-52 = twice the unit round-off)
    plus the roundings of alpha *, beta * and the final sum.  beta == 0 ignores
    C0 (BLAS semantics)."""
    a, b = np.asarray(opA, dtype=LD), np.asarray(opB, dtype=LD)
    k = a.shape[1]
    ref = LD(alpha) * (a @ b)
    mag = abs(LD(alpha)) * (np.abs(a) @ np.abs(b))
    if beta != 0.0:
        c0 = np.asarray(C0, dtype=LD)
        ref = ref + LD(beta) * c0
        mag = mag + abs(LD(beta)) * np.abs(c0)
    return ref, LD(k + 4) * LD(EPS) * mag


def bound_ratio(C, ref, bound):
    """max |C - ref| / bound (entries with a zero bound must be exact); asserts
    that C is finite."""
    C = np.asarray(C)
    assert np.isfinite(C).all(), "non-finite entries in the result"
    err = np.abs(np.asarray(C, dtype=LD) - ref)
    zero = bound == 0
    assert (err[zero] == 0).all(), "entries with a zero bound are not exact"
    if zero.all():
        return 0.0
    return float(np.max(err[~zero] / bound[~zero]))


def check_gemm(C, opA, opB, C0, alpha, beta):
    ref, bound = gemm_ref(opA, opB, C0, alpha, beta)
    return bound_ratio(C, ref, bound)


# ---------------------------------------------------------------- Cholesky --
def chol_ref(A):
    """Lower Cholesky factor of the lower triangle of A in longdouble (column
    by column, plain array operations)."""
    A = np.asarray(A, dtype=LD)
    M = A.shape[0]
    L = np.zeros((M, M), dtype=LD)
    for j in range(M):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < M:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def sym_from_lower(A):
    A = np.asarray(A)
    return np.tril(A) + np.tril(A, -1).T


def chol_ratio(A, L):
    """r = max |A - L L'| / (M eps max|A|) over the lower triangle, in longdouble."""
    A = sym_from_lower(np.asarray(A, dtype=LD))
    L = np.tril(np.asarray(L, dtype=LD))
    M = A.shape[0]
    assert np.isfinite(np.asarray(L, dtype=np.float64)).all(), "non-finite factor"
    return float(np.max(np.abs(np.tril(A - L @ L.T))) / (M * LD(EPS) * np.max(np.abs(A))))


def check_chol(A, L, limit):
    r = chol_ratio(A, L)
    assert r <= limit, f"Cholesky residual ratio {r:.3g} above {limit:.3g}"
    return r


def dinv_ratio(D, Ljj):
    """max |D Ljj - I| / (64 eps kappa_1(Ljj)), in longdouble."""
    D, Lj = np.asarray(D, dtype=LD), np.tril(np.asarray(Ljj, dtype=LD))
    nb = Lj.shape[0]
    k1 = float(np.linalg.norm(np.asarray(Lj, dtype=np.float64), 1)
               * np.linalg.norm(np.linalg.inv(np.asarray(Lj, dtype=np.float64)), 1))
    return float(np.max(np.abs(D @ Lj - np.eye(nb, dtype=LD))) / (64 * LD(EPS) * k1))


def trsm_ratio(Xout, L, Xin):
    """r = max |Xout L' - Xin| / (M eps max(|Xout| |L'|)), in longdouble."""
    Xo, Xi, Lt = np.asarray(Xout, dtype=LD), np.asarray(Xin, dtype=LD), np.tril(np.asarray(L, dtype=LD)).T
    M = Lt.shape[0]
    assert np.isfinite(np.asarray(Xout)).all(), "non-finite solve"
    return float(np.max(np.abs(Xo @ Lt - Xi)) / (M * LD(EPS) * np.max(np.abs(Xo) @ np.abs(Lt))))


def block_kappa(L):
    """max over the 64-blocks of kappa_2(L_jj) = sqrt(kappa_2) of the diagonal
    block the kernel factors and inverts at that step (L_jj L_jj')."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    return max(float(np.linalg.cond(L[j:j + 64, j:j + 64], 2)) for j in range(0, L.shape[0], 64))


def rand_orth(rng, M):
    Q, R = np.linalg.qr(rng.standard_normal((M, M)))
    return Q * np.sign(np.diag(R))


def spectral(Q, lam):
    """Q diag(lam) Q' formed in longdouble and rounded once, so that the spectrum
    is lam to within a rounding of the entries."""
    Ql = np.asarray(Q, dtype=LD)
    return np.asarray((Ql * np.asarray(lam, dtype=LD)) @ Ql.T, dtype=np.float64)


def matern(rng, M, dup=0, ell=1.0):
    """Matern-3/2 K on random sites (the shape of tools/eigh_probe.cpp); the
    last ``dup`` sites repeat the first ones (a rank-deficient K)."""
    x = np.column_stack([rng.uniform(-6, 6, M), rng.uniform(-6, 6, M), rng.uniform(0, 8, M)]) / ell
    if dup:
        x[M - dup:] = x[:dup]
    d = np.sqrt(np.maximum(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1), 0.0))
    Q = np.sqrt(3.0) * d
    return 6e-3 * (1 + Q) * np.exp(-Q)


CHOL_FAMILIES = ('well', 'matern', 'ill')


def chol_matrix(family, M, seed=0):
    rng = np.random.default_rng([CHOL_FAMILIES.index(family), M, seed, 77])
    if family == 'matern':
        A = matern(rng, M) + 1e-4 * np.eye(M)
    else:
        Q = rand_orth(rng, M)
        A = spectral(Q, np.logspace(0, -2 if family == 'well' else -10, M))
    return (A + A.T) / 2


# -------------------------------------------------------------------- eigh --
EIGH_FAMILIES = ('goe', 'goe_1e8', 'goe_1e-8', 'scaled_identity', 'zero', 'diagonal', 'identity_plus_rank1',
                 'minus_identity_plus_rank1', 'projector', 'triples', 'wilkinson', 'matern_dup', 'matern_pad')
CLUSTER_FAMILIES = ('minus_identity_plus_rank1', 'projector', 'triples')
EIGH_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 97, 130)
EIGH_T = 4.0


def eigh_matrix(family, M):
    rng = np.random.default_rng([EIGH_FAMILIES.index(family), M, 1000])
    if family.startswith('goe'):
        G = rng.standard_normal((M, M))
        A = (G + G.T) / np.sqrt(2.0)
        A = A * {'goe': 1.0, 'goe_1e8': 1e8, 'goe_1e-8': 1e-8}[family]
    elif family == 'scaled_identity':
        A = 2.5 * np.eye(M)
    elif family == 'zero':
        A = np.zeros((M, M))
    elif family == 'diagonal':
        A = np.diag(rng.permutation(M) * 0.37 - 0.11 * M)
    elif family in ('identity_plus_rank1', 'minus_identity_plus_rank1'):
        u = rng.standard_normal(M)
        A = np.eye(M) + np.outer(u, u)
        if family.startswith('minus'):
            A = -A
    elif family == 'projector':
        Q = rand_orth(rng, M)
        A = spectral(Q, (np.arange(M) >= M // 2).astype(float))
    elif family == 'triples':
        Q = rand_orth(rng, M)
        A = spectral(Q, 1.0 + np.arange(M) // 3)
    elif family == 'wilkinson':
        A = np.diag(np.abs(np.arange(M) - (M - 1) / 2.0)) + np.diag(np.ones(M - 1), 1) + np.diag(np.ones(M - 1), -1)
    elif family == 'matern_dup':
        A = matern(rng, M, dup=min(10, M // 2), ell=3.0)
    elif family == 'matern_pad':     # diag(K, 7 I): the Nystrom variant's padding of K_mm
        m1 = M - M // 4
        A = 7.0 * np.eye(M)
        A[:m1, :m1] = matern(rng, m1, ell=3.0)
    else:
        raise KeyError(family)
    return (A + A.T) / 2


def eigh_ratios(A, w, U):
    """(eigenvalues vs numpy, orthogonality, residual) of an eigendecomposition
    of the symmetric A, in units of M eps ||A||_2, M eps and M eps ||A||_2,
    formed in longdouble.  Asserts finite and ascending w.  For the zero matrix
    the first and third are |w| / 1e-300 (the limit there is |w| <= 1e-300)."""
    A = np.asarray(A, dtype=np.float64)
    w, U = np.asarray(w, dtype=np.float64), np.asarray(U, dtype=np.float64)
    M = A.shape[0]
    assert np.isfinite(w).all() and np.isfinite(U).all(), "non-finite eigenpairs"
    assert (np.diff(w) >= 0).all(), "eigenvalues not ascending"
    wn = np.linalg.eigvalsh(A)
    nrm = LD(np.max(np.abs(wn)))
    Ul, wl = U.astype(LD), w.astype(LD)
    orth = float(np.max(np.abs(Ul.T @ Ul - np.eye(M, dtype=LD))) / (M * LD(EPS)))
    if nrm == 0:
        z = float(np.max(np.abs(w)) / 1e-300)
        return z, orth, z
    ev = float(np.max(np.abs(wl - wn.astype(LD))) / (M * LD(EPS) * nrm))
    res = float(np.max(np.abs(A.astype(LD) @ Ul - Ul * wl)) / (M * LD(EPS) * nrm))
    return ev, orth, res


def check_eigh(A, w, U, T=EIGH_T, what=''):
    ev, orth, res = eigh_ratios(A, w, U)
    lim = 1.0 if not np.any(A) else T
    assert ev <= lim, f"{what}: eigenvalue error {ev:.3g} above {lim:g}"
    assert orth <= T, f"{what}: orthogonality {orth:.3g} above {T:g}"
    assert res <= lim, f"{what}: residual {res:.3g} above {lim:g}"
    return ev, orth, res
