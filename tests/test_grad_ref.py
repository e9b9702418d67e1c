"""The numpy reference of ``oi_gpr_predict_grad`` (tests/grad_ref.py) against
the oracle, without a GPU: its value rows are ``gp_oracle.matern32``'s, its
derivative mean and variance agree with difference quotients of
``gp_oracle.predict`` and of its own value covariance, its joint prior is
positive semi-definite, and its value block is the ``Kxs - v'v`` of
tests/test_gpu_predict_multi.py.  Cells of predict64.npz cut to n observations,
7 targets each: a lattice of 5, one target ON an observation and one identical
to another target (both take the Q = 0 branch).

The step of the quotients is h_k = 1e-4 ell_k / sqrt(3), i.e. 1e-4 in Q.  The
mean's central difference has a defect of O(h^2) = 1e-8 of the prior sd and a
cancellation error of about eps |fs| / (1e-4 sqrt(sf2)) = 5e-12: bound 1e-6
(measured <= 6.9e-9; a sign, scale or index error is O(1)).  The variance of
the quotient (f(x + h) - f(x - h)) / 2 h falls short of the derivative's by
(4/3) h sqrt(3) / ell = 1.33e-4 relative (the |d|^3 term of the covariance):
bound 1e-3 (measured <= 1.8e-4)."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
import grad_ref as G

NS = (1, 5, 63, 64, 65, 130)
STEP = 1e-4


def _cell(n):
    d = load_golden('predict64.npz')
    c = NS.index(n)
    a = d['offs'][c]
    x, y, hyp = d['x'][a:a + n], d['y'][a:a + n], d['hyp'][c]
    xs = G.lattice(d['xs'][c], 5)
    xs = np.concatenate([xs, x[:1], xs[1:2]])    # on an observation; identical to target 1
    return x, y, xs, float(d['mean']), hyp


@pytest.fixture(scope='module', params=NS)
def case(request):
    x, y, xs, mean, hyp = _cell(request.param)
    m4, J = G.ref_cell(x, y, xs, mean, hyp)
    return x, y, xs, mean, hyp, m4, J


def test_value_rows_are_the_oracles(case):
    x, y, xs, mean, hyp, _, _ = case
    C = G.cross(x, xs, list(hyp[:3]), hyp[3])
    K = O.matern32(x, list(hyp[:3]), hyp[3], xs=xs)      # n x nt
    assert C.shape == (28, len(y))
    assert np.all(np.abs(C[0::4] - K.T) <= 1e-15 * np.abs(K.T))


def test_prior_is_psd_with_the_stated_diagonal(case):
    x, y, xs, mean, hyp, _, _ = case
    P = G.prior(xs, list(hyp[:3]), hyp[3])
    s = np.tile(G.scales(hyp), len(xs))
    assert np.array_equal(P, P.T)
    assert np.all(np.abs(P.diagonal() - s * s) <= 4e-16 * s * s)
    lo = np.linalg.eigvalsh(P / np.outer(s, s)).min()
    print("smallest eigenvalue of the prior correlation", lo)
    assert lo >= -1e-12


def _shifted(xs, k, h):
    e = np.zeros(3)
    e[k] = h
    return xs + e, xs - e


def test_derivative_mean_against_central_differences(case):
    x, y, xs, mean, hyp, m4, _ = case
    ell, sf2, sn2 = list(hyp[:3]), hyp[3], hyp[4]
    s = G.scales(hyp)
    for k in range(3):
        h = STEP * ell[k] / O.SQRT3
        p, m = _shifted(xs, k, h)
        fd = (O.predict(x, y, p, mean, ell, sf2, sn2)[0] - O.predict(x, y, m, mean, ell, sf2, sn2)[0]) / (2 * h)
        err = np.abs(m4[k + 1::4] - fd).max() / s[k + 1]
        print(f"n {len(y)} component {k}: |mean - central difference| / prior sd {err:.3e}")
        assert err <= 1e-6


def test_derivative_variance_against_the_quotients_variance(case):
    x, y, xs, mean, hyp, _, J = case
    ell = list(hyp[:3])
    nt = len(xs)
    for k in range(3):
        h = STEP * ell[k] / O.SQRT3
        p, m = _shifted(xs, k, h)
        _, Jq = G.ref_cell(x, y, np.concatenate([p, m]), mean, hyp)
        V = Jq[0::4, 0::4]                                   # the value covariance at the 2 nt shifted targets
        i = np.arange(nt)
        var = (V[i, i] + V[nt + i, nt + i] - 2 * V[i, nt + i]) / (4 * h * h)
        mine = J.diagonal()[k + 1::4]
        err = np.abs(mine - var).max(initial=0.0) / np.abs(mine).min()
        print(f"n {len(y)} component {k}: relative |variance - quotient's| {np.abs(mine / var - 1).max():.3e}")
        assert np.all(np.abs(mine - var) <= 1e-3 * np.abs(mine)), err


def test_value_block_is_predict_multis(case):
    """J's value block comes out of the solve and the product over all 4 nt
    columns, _ref_cell's out of those over the nt value columns alone; a BLAS may
    block the two differently, so they differ in the last bits.  Measured with
    OpenBLAS: 0, 9.7e-17, 1.8e-16, 1.8e-16, 4.7e-16 and 8.6e-16 of sf2 at n = 1, 5,
    63, 64, 65, 130 against the bound 1e-15 -- a thin margin at n = 130."""
    from test_gpu_predict_multi import _ref_cell
    x, y, xs, mean, hyp, m4, J = case
    fs, sd, _, cov = _ref_cell(x, y, xs, mean, hyp)
    err = np.abs(J[0::4, 0::4] - cov).max() / hyp[3]
    print(f"n {len(y)}: |J[4t, 4t'] - (Kxs - v'v)| / sf2 {err:.3e}")
    assert err <= 1e-15
    # V' (L^-1 r) against Kxsx' (L^-T L^-1 r): two orders of the same solves, T1's bound
    assert np.all(np.abs(m4[0::4] - fs) <= G.RTOL * np.maximum(1.0, np.abs(fs)))


def test_empty_cell_is_the_prior():
    x, y, xs, mean, hyp = _cell(5)
    m4, J = G.ref_cell(x[:0], y[:0], xs, mean, hyp)
    assert np.array_equal(m4, np.tile([mean, 0, 0, 0], 7))
    assert np.array_equal(J, G.prior(xs, list(hyp[:3]), hyp[3]))
    m0, J0 = G.ref_cell(x, y, xs[:0], mean, hyp)
    assert m0.shape == (0,) and J0.shape == (0, 0)
