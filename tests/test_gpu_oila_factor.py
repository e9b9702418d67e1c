"""oila::cholesky and oila::trsm_right_lt (csrc/oi_linalg.hip: k_potrf_tile,
the panel product with the explicit inverse of the diagonal block, the lower-
tile update) against longdouble checks on the host.

Accuracy is r = max|A - L L'| / (M eps max|A|), formed in longdouble.  The panel
step multiplies by an explicit inverse of the 64 x 64 diagonal block, so the
factorisation is not backward stable independently of conditioning and no
textbook bound applies: the limit is 8 x the worst r of np.linalg.cholesky on
the same matrices (computed in the test; the margin covers the different
blocking and summation order), for the ill-conditioned family times
kappa_2(L_jj) of the worst 64-block (= sqrt(kappa_2) of the diagonal block
that step inverts: the growth the explicit inverse allows).  The kernel's own
measurement never sets a limit.

Measured (reference: CPU; kernel: MI355X), worst over M in SIZES, pad {0, 3}:
    family   numpy r   limit            kernel r
    well     0.229     1.84             0.229
    matern   0.769     6.15             0.769
    ill      0.257     up to 2.05e5     0.257
(the worst cases are the smallest matrices, where both take the same roundings).
Inverse blocks, max|Dinv L_jj - I| / (64 eps kappa_1(L_jj)), np.linalg.inv /
kernel: well 0.0050 / 0.0074, matern 0.0116 / 0.0111, ill 0.0068 / 0.0069
(limit 8 x the first).  Solve r, scipy.linalg.solve_triangular / kernel: well
0.158 / 0.258, matern 0.474 / 0.474, ill 0.229 / 0.183.

The first run of these tests found that the lower-tile update wrote the whole
diagonal tiles, strict upper triangle included (test_structure); cholesky now
updates with Gemm::tri == 3."""
import numpy as np
import pytest
import scipy.linalg

import oila_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)
MARGIN = 8.0


class Fact:
    def __init__(self, A, pad):
        self.A0 = A
        self.M = A.shape[0]
        self.nblk = (self.M + 63) // 64
        self.A = R.DevMat(A, pad)
        self.dinv = R.DevMat(np.zeros((4096, self.nblk)), 0, fill=R.SENT)

    def desc(self, info_ptr):
        return R.Chol(self.A.ptr(), self.dinv.ptr(), info_ptr, self.M, self.A.ld)


def factor(mats, pads):
    """All matrices in one launch (mixed sizes share the jb loop)."""
    fs = [Fact(A, pad) for A, pad in zip(mats, pads)]
    info = R.dev_ints([0] * len(fs) + [-7])
    R.run_cholesky([f.desc(info.data_ptr() + 4 * i) for i, f in enumerate(fs)])
    info = info.cpu().numpy()
    assert info[-1] == -7
    for f, i in zip(fs, info):
        f.info = int(i)
        f.L = f.A.result()
        f.D = f.dinv.result().T.reshape(f.nblk, 64, 64).transpose(0, 2, 1)   # D[b] column-major 64 x 64
    return fs


@pytest.fixture(scope='module')
def families():
    """family -> (matrices, numpy factors, factored on the GPU), every size at
    pad 0 and 3 in ONE launch over all families."""
    mats, pads, fam = [], [], []
    for f in R.CHOL_FAMILIES:
        for M in SIZES:
            for pad in (0, 3):
                mats.append(R.chol_matrix(f, M, seed=pad))
                pads.append(pad)
                fam.append(f)
    fs = factor(mats, pads)
    out = {f: [] for f in R.CHOL_FAMILIES}
    for f, A, x in zip(fam, mats, fs):
        out[f].append((A, np.linalg.cholesky(A), x))
    return out


@pytest.mark.parametrize('family', R.CHOL_FAMILIES)
def test_structure(families, family):
    for A, Ln, f in families[family]:
        M = f.M
        assert f.info == 0
        up = np.triu_indices(M, 1)
        assert np.array_equal(f.L[up].view(np.uint64), A[up].view(np.uint64)), "strict upper triangle touched"
        assert np.isfinite(np.tril(f.L)).all()
        for b in range(f.nblk):
            nb = min(64, M - 64 * b)
            D = f.D[b]
            assert np.isfinite(D).all()
            assert (np.triu(D, 1) == 0).all(), "Dinv block not lower triangular"
            assert np.array_equal(D[nb:, :], np.eye(64)[nb:, :]), "Dinv block not the identity beyond nb"


@pytest.mark.parametrize('family', R.CHOL_FAMILIES)
def test_factorisation_accuracy(families, family):
    ref = max(R.chol_ratio(A, Ln) for A, Ln, f in families[family])
    worst, worst_lim = 0.0, 0.0
    for A, Ln, f in families[family]:
        limit = MARGIN * ref
        if family == 'ill':
            limit *= R.block_kappa(np.asarray(R.chol_ref(A), dtype=np.float64))
        r = R.chol_ratio(A, f.L)
        worst, worst_lim = max(worst, r), max(worst_lim, limit)
        assert r <= limit, (family, f.M, r, limit)
    print(f"CHOL {family}: numpy worst r {ref:.3g}, limit up to {worst_lim:.3g}, kernel worst r {worst:.3g}")


@pytest.mark.parametrize('family', R.CHOL_FAMILIES)
def test_inverse_blocks(families, family):
    """max|Dinv_jj L_jj - I| <= 64 eps kappa_1(L_jj) c, c = 8 x np.linalg.inv's
    worst ratio on the reference's blocks."""
    ref, ker = 0.0, []
    for A, Ln, f in families[family]:
        for b in range(f.nblk):
            nb = min(64, f.M - 64 * b)
            s = slice(64 * b, 64 * b + nb)
            ref = max(ref, R.dinv_ratio(np.linalg.inv(np.tril(Ln[s, s])), Ln[s, s]))
            ker.append((f.M, b, R.dinv_ratio(f.D[b][:nb, :nb], f.L[s, s])))
    print(f"DINV {family}: np.linalg.inv worst {ref:.3g}, kernel worst {max(k[2] for k in ker):.3g}")
    for M, b, r in ker:
        assert r <= MARGIN * ref, (family, M, b, r, MARGIN * ref)


def test_info_and_nan():
    rng = np.random.default_rng(21)
    # indefinite only in the second 64-block: A = L L' with L(100, 100) such that the pivot there is -1
    L = np.tril(rng.uniform(-1, 1, (130, 130)) / 16) + np.eye(130)
    A = L @ L.T
    A[100, 100] += -1.0 - L[100, 100] ** 2        # Schur complement's pivot at 100: L(100,100)^2 -> -1
    good = R.chol_matrix('well', 130, seed=5)
    zero = np.zeros((1, 1))
    nanm = R.chol_matrix('well', 65, seed=6)
    nanm[3, 1] = np.nan
    # the reference agrees on which are positive definite
    assert np.linalg.eigvalsh(A[:100, :100]).min() > 0 and np.linalg.eigvalsh(A[:101, :101]).min() < 0
    bad, ok, z, nn = factor([A, good, zero, nanm], [3, 0, 0, 3])
    assert bad.info == 1 and z.info == 1
    assert ok.info == 0
    assert R.chol_ratio(good, ok.L) <= MARGIN * R.chol_ratio(good, np.linalg.cholesky(good))
    # the first block of the indefinite matrix is still its factor
    assert R.chol_ratio(A[:64, :64], bad.L[:64, :64]) <= MARGIN * R.chol_ratio(A[:64, :64], np.linalg.cholesky(A[:64, :64]))
    assert nn.info == 0 and np.isnan(np.tril(nn.L)).any(), "a NaN entry propagates and is not flagged"


@pytest.mark.parametrize('family', R.CHOL_FAMILIES)
def test_trsm_right_lt(families, family):
    """X <- X L^-T with the kernel's own factor and inverse blocks; the limit
    is 8 x the worst r of scipy's solve_triangular (itself checked in
    longdouble by the same formula) on the same L and X, for the
    ill-conditioned family times kappa_2 of the worst diagonal block."""
    rng = np.random.default_rng(22)
    picks = [(A, f) for A, Ln, f in families[family]]   # M = 65, 129, 200: a partial last block (nbj < 64)
    descs, cases = [], []
    for i, (A, f) in enumerate(picks):
        m = (1, 64, 65, 130)[i % 4]
        X = rng.uniform(-1, 1, (m, f.M))
        x = R.DevMat(X, 3 * (i % 2))
        descs.append(R.TrsmRLT(x.ptr(), f.A.ptr(), f.dinv.ptr(), m, f.M, x.ld, f.A.ld))
        cases.append((x, X, f))
    R.run_trsm(descs)
    ref, ker = 0.0, []
    for x, X, f in cases:
        L = np.tril(f.L)
        Xs = scipy.linalg.solve_triangular(L, X.T, lower=True).T
        ref = max(ref, R.trsm_ratio(Xs, L, X))
        lim = R.block_kappa(L) if family == 'ill' else 1.0
        ker.append((f.M, X.shape[0], R.trsm_ratio(x.result(), L, X), lim))
    print(f"TRSM {family}: scipy worst r {ref:.3g}, kernel worst r {max(k[2] for k in ker):.3g}")
    for M, m, r, lim in ker:
        assert r <= MARGIN * ref * lim, (family, M, m, r, MARGIN * ref * lim)
