"""The checkers of tests/oila_ref.py and the eigensolver's CPU model
(tools/eigh_model.py), without a GPU: numpy's eigh must stay at or below 1 in
the checkers' units on every family, the model -- the kernels' algorithm step
for step -- at or below the GPU tests' T = 4; and each checker must be able to
fail (a float64 numpy result passes, one entry off by 1e-9 relative does not).

Measured (CPU), worst ratios (eigenvalues, orthogonality, residual) over all
families and sizes: numpy 0.83, 0.96, 0.92; the model, M <= 65, 1.30, 0.85,
1.73.  Without the weak / collapse rules of mgs (eigh_model.eigh(fix=False),
the first version of the kernels) the model's residual is 5e12 .. 7e13 on the
projector family (M = 32 .. 65) and on triples at M = 33, 64, 65."""
import os
import sys

import numpy as np
import pytest

import oila_ref as R

sys.path.insert(0, os.path.join(R.ROOT, 'tools'))
import eigh_model  # noqa: E402

@pytest.mark.parametrize('family', R.EIGH_FAMILIES)
def test_numpy_eigh_within_one(family):
    for M in R.EIGH_SIZES:
        A = R.eigh_matrix(family, M)
        assert (A == A.T).all()
        w, U = np.linalg.eigh(A)
        R.check_eigh(A, w, U, T=1.0, what=f"numpy {family} M={M}")


@pytest.mark.parametrize('family', R.EIGH_FAMILIES)
def test_model_within_T(family):
    for M in (m for m in R.EIGH_SIZES if m <= 65):
        A = R.eigh_matrix(family, M)
        w, U = eigh_model.eigh(A)
        R.check_eigh(A, w, U, T=R.EIGH_T, what=f"model {family} M={M}")


def test_model_without_the_cluster_rules_fails():
    """What the residual check is for: the first version's replacement of a
    collapsed column returns an orthonormal basis that is no eigenbasis."""
    A = R.eigh_matrix('projector', 64)
    w, U = eigh_model.eigh(A, fix=False)
    ev, orth, res = R.eigh_ratios(A, w, U)
    assert ev <= 1.0 and orth <= 1.0 and res > 1e9
    with pytest.raises(AssertionError, match='residual'):
        R.check_eigh(A, w, U)


def test_eigh_checker_can_fail():
    A = R.eigh_matrix('goe', 33)
    w, U = np.linalg.eigh(A)
    R.check_eigh(A, w, U, T=1.0)
    w2 = w.copy()
    w2[5] *= 1 + 1e-9
    with pytest.raises(AssertionError, match='eigenvalue'):
        R.check_eigh(A, w2, U)
    U2 = U.copy()
    U2[3, 7] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        R.check_eigh(A, w, U2)
    # an orthonormal basis that is not an eigenbasis (what the cluster defect returned)
    U3 = U.copy()
    c, s = np.cos(1e-6), np.sin(1e-6)
    U3[:, [0, 32]] = U[:, [0, 32]] @ np.array([[c, -s], [s, c]])
    with pytest.raises(AssertionError, match='residual'):
        R.check_eigh(A, w, U3)
    with pytest.raises(AssertionError, match='ascending'):
        R.check_eigh(A, w[::-1], U[:, ::-1])


def test_gemm_checker_can_fail():
    rng = np.random.default_rng(5)
    for scale in (False, True):
        A, B, C0 = rng.uniform(-1, 1, (65, 17)), rng.uniform(-1, 1, (17, 33)), rng.uniform(-1, 1, (65, 33))
        if scale:   # the bound is relative to |A||B|, not to |C|
            A = A * 10.0 ** rng.uniform(-8, 8, A.shape)
            B = B * 10.0 ** rng.uniform(-8, 8, B.shape)
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)):
            C = alpha * (A @ B) + (beta * C0 if beta else 0.0)
            assert R.check_gemm(C, A, B, C0, alpha, beta) <= 1.0
            i, j = np.unravel_index(np.argmax(np.abs(A) @ np.abs(B) / np.maximum(np.abs(C), 1e-300) < 50), C.shape)
            C[i, j] *= 1 + 1e-9
            assert R.check_gemm(C, A, B, C0, alpha, beta) > 1.0
    # beta == 0 ignores C0; a NaN in the result is refused
    C = A @ B
    assert R.check_gemm(C, A, B, np.full(C.shape, np.nan), 1.0, 0.0) <= 1.0
    C[0, 0] = np.nan
    with pytest.raises(AssertionError, match='finite'):
        R.check_gemm(C, A, B, C0, 1.0, 0.0)


def test_chol_checker_can_fail():
    for family in R.CHOL_FAMILIES:
        A = R.chol_matrix(family, 65)
        L = np.linalg.cholesky(A)
        r = R.chol_ratio(A, L)
        # the longdouble factor rounded to float64 is within a rounding of exact
        r0 = R.chol_ratio(A, np.asarray(R.chol_ref(A), dtype=np.float64))
        assert r0 <= 1.0 and r <= 1.0, (family, r, r0)
        R.check_chol(A, L, 8 * r)
        L2 = L.copy()
        L2[40, 0] *= 1 + 1e-9      # in the first column: A's largest scale
        L2[0, 0] *= 1 + 1e-9
        with pytest.raises(AssertionError, match='Cholesky'):
            R.check_chol(A, L2, 8 * r)


def test_descriptor_mirrors_match_the_library():
    import ctypes
    h = R.lib()
    for which, s in enumerate(R.STRUCTS):
        assert ctypes.sizeof(s) == h.oila_test_sizeof(which), s.__name__
    assert [ctypes.sizeof(s) for s in R.STRUCTS] == [72, 56, 32, 40, 40]
    assert h.oila_test_sizeof(len(R.STRUCTS)) == -1
    for M in (1, 33, 130):
        assert h.oila_test_eigh_workspace_doubles(M) >= 7 * M * M + 128 * M
