"""``oi_svgp_predict`` and ``oi_svgp_elbo`` (include/oi.h) without a GPU: both
symbols are exported and bound, every misuse is rejected with OI_E_ARG (-1) and
a message naming the argument before any device work, an empty batch is a
no-op, and the Python wrappers reject inconsistent shapes -- as
tests/test_predict_multi_abi.py checks for ``oi_gpr_predict_multi``."""
import ctypes

import numpy as np
import pytest

from optimalinterpolation_amd import _lib, svgp

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32
M = 3
P = 6 + 4 * M + M * (M + 1) // 2


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _predict(lib, **over):
    """One cell with M = 3 and 2 targets; ``over`` replaces arguments."""
    a = dict(params=np.zeros((1, P)), M=M, ncell=1, xs=np.zeros((2, 3)),
             toffs=np.array([0, 2], dtype=np.int64), with_noise=0, mean=np.zeros(2),
             var=np.zeros(2), cov=None, status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_svgp_predict(_p(a['params'], D), a['M'], a['ncell'], _p(a['xs'], D),
                               _p(a['toffs'], I64), a['with_noise'], _p(a['mean'], D),
                               _p(a['var'], D), _p(a['cov'], D), _p(a['status'], I32), None)


def _elbo(lib, **over):
    """One cell with M = 3 and 4 observations; ``over`` replaces arguments."""
    a = dict(params=np.zeros((1, P)), M=M, xyt=np.zeros((4, 3)), y=np.zeros(4),
             offs=np.array([0, 4], dtype=np.int64), ncell=1, elbo=np.zeros(1),
             status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_svgp_elbo(_p(a['params'], D), a['M'], _p(a['xyt'], D), _p(a['y'], D),
                            _p(a['offs'], I64), a['ncell'], _p(a['elbo'], D),
                            _p(a['status'], I32), None)


def test_symbols_exported_and_bound():
    assert 'oi_svgp_predict' in _lib.EXPORTS and 'oi_svgp_elbo' in _lib.EXPORTS
    lib = _lib.load()
    assert lib.oi_svgp_predict.restype is ctypes.c_int and len(lib.oi_svgp_predict.argtypes) == 11
    assert lib.oi_svgp_elbo.restype is ctypes.c_int and len(lib.oi_svgp_elbo.argtypes) == 9
    assert callable(_lib.svgp_predict) and callable(_lib.svgp_elbo)
    assert callable(svgp.predict_f) and callable(svgp.predict_y) and callable(svgp.elbo)


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(M=0), b'M must be in [1, 64]'),
    (dict(M=65), b'M must be in [1, 64]'),
    (dict(params=None), b'params'),
    (dict(toffs=None), b'toffs'),
    (dict(status=None), b'status'),
    (dict(toffs=np.array([1, 2], dtype=np.int64)), b'toffs[0]'),
    (dict(ncell=2, params=np.zeros((2, P)), status=np.zeros(2, dtype=np.int32),
          toffs=np.array([0, 2, 1], dtype=np.int64)), b'toffs must be non-decreasing'),
    (dict(xs=None), b'xs'),
    (dict(mean=None), b'mean'),
    (dict(var=None), b'var'),
    (dict(with_noise=1, cov=np.zeros(4)), b'cov must be NULL with with_noise'),
    (dict(cov=np.zeros(4), toffs=np.array([0, 20000], dtype=np.int64)), b'toffs'),
])
def test_predict_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _predict(lib, **over) == -1
    assert word in lib.oi_last_error()


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(M=0), b'M must be in [1, 64]'),
    (dict(M=65), b'M must be in [1, 64]'),
    (dict(params=None), b'params'),
    (dict(xyt=None), b'xyt'),
    (dict(y=None), b'y'),
    (dict(offs=None), b'offs'),
    (dict(elbo=None), b'elbo'),
    (dict(status=None), b'status'),
    (dict(offs=np.array([1, 4], dtype=np.int64)), b'offs[0]'),
    (dict(ncell=2, params=np.zeros((2, P)), status=np.zeros(2, dtype=np.int32), elbo=np.zeros(2),
          offs=np.array([0, 4, 4], dtype=np.int64)), b'every cell needs n >= 1'),
])
def test_elbo_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _elbo(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    assert _predict(lib, ncell=0, params=None, xs=None, toffs=None, mean=None, var=None,
                    status=None) == 0
    assert _elbo(lib, ncell=0, params=None, xyt=None, y=None, offs=None, elbo=None,
                 status=None) == 0


def test_wrappers_reject_inconsistent_shapes():
    th = np.zeros((2, P))
    with pytest.raises(ValueError, match='belong to no M'):
        _lib.svgp_predict(np.zeros((1, P + 1)), np.zeros((2, 3)), [0, 2])
    with pytest.raises(ValueError, match='belong to no M'):
        _lib.svgp_elbo(np.zeros((1, 5)), np.zeros((2, 3)), np.zeros(2), [0, 2])
    with pytest.raises(ValueError):  # toffs too short for two cells
        _lib.svgp_predict(th, np.zeros((2, 3)), [0, 2])
    with pytest.raises(ValueError):  # toffs[-1] != len(xs)
        _lib.svgp_predict(th, np.zeros((2, 3)), [0, 1, 3])
    with pytest.raises(ValueError):  # decreasing toffs
        _lib.svgp_predict(th, np.zeros((2, 3)), [0, 3, 2])
    with pytest.raises(ValueError):  # len(y) != offs[-1]
        _lib.svgp_elbo(th, np.zeros((4, 3)), np.zeros(3), [0, 2, 4])
    with pytest.raises(ValueError):  # xyt rows != len(y)
        _lib.svgp_elbo(th, np.zeros((3, 3)), np.zeros(4), [0, 2, 4])
    with pytest.raises(_lib.OiError, match='cov must be NULL with with_noise'):
        _lib.svgp_predict(th, np.zeros((2, 3)), [0, 1, 2], with_noise=True, cov=True)


def test_unpack_keeps_the_flat_row():
    th = np.arange(P, dtype=np.float64)
    m = svgp.unpack(th, M)
    assert np.array_equal(m['theta'], th)
    assert set(m) >= {'lengthscales', 'kernel_variance', 'noise_variance', 'mean', 'Z', 'q_mu', 'q_sqrt'}
