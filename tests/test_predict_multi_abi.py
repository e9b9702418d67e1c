"""``oi_gpr_predict_multi`` (include/oi.h) without a GPU: the symbol is exported
and bound, and every misuse is rejected with OI_E_ARG (-1) and a message
before any device work -- as ``test_abi.test_argument_errors_without_gpu``
checks for the other entry points."""
import ctypes

import numpy as np
import pytest

from optimalinterpolation_amd import _lib, nystrom

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _call(lib, **over):
    """One cell with 3 observations and 2 targets; ``over`` replaces arguments."""
    a = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=np.array([0, 3], dtype=np.int64), ncell=1,
             xs=np.zeros((2, 3)), toffs=np.array([0, 2], dtype=np.int64), hyp=np.ones((1, 5)),
             fs=np.zeros(2), sd=np.zeros(2), lz=np.zeros(1), cov=np.zeros(4),
             status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_gpr_predict_multi(_p(a['xyt'], D), _p(a['z'], D), _p(a['offs'], I64), a['ncell'],
                                    _p(a['xs'], D), _p(a['toffs'], I64), 0.0, _p(a['hyp'], D),
                                    _p(a['fs'], D), _p(a['sd'], D), _p(a['lz'], D), _p(a['cov'], D),
                                    _p(a['status'], I32), None)


def test_symbol_exported_and_bound():
    assert 'oi_gpr_predict_multi' in _lib.EXPORTS
    lib = _lib.load()
    assert lib.oi_gpr_predict_multi.restype is ctypes.c_int
    assert len(lib.oi_gpr_predict_multi.argtypes) == 14
    assert callable(_lib.gpr_predict_multi) and callable(_lib.gpr_predict_multi_device)


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(offs=None), b'offs'),
    (dict(toffs=None), b'toffs'),
    (dict(offs=np.array([1, 3], dtype=np.int64)), b'offs[0]'),
    (dict(toffs=np.array([1, 2], dtype=np.int64)), b'toffs[0]'),
    (dict(offs=np.array([0, 3, 2], dtype=np.int64), ncell=2,
          toffs=np.array([0, 1, 2], dtype=np.int64)), b'offs must be non-decreasing'),
    (dict(offs=np.array([0, 1, 3], dtype=np.int64), ncell=2,
          toffs=np.array([0, 2, 1], dtype=np.int64)), b'toffs must be non-decreasing'),
    (dict(status=None), b'status'),
    (dict(hyp=None), b'hyp'),
    (dict(xyt=None), b'xyt'),
    (dict(z=None), b'z'),
    (dict(xs=None), b'xs'),
    (dict(fs=None), b'fs'),
    (dict(sd=None), b'sd'),
])
def test_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    z1 = np.zeros(1, dtype=np.int64)
    assert _call(lib, ncell=0, offs=z1, toffs=z1, xyt=None, z=None, xs=None, hyp=None, fs=None,
                 sd=None, lz=None, cov=None, status=None) == 0


def test_wrapper_rejects_inconsistent_batches():
    x, z = np.zeros((3, 3)), np.zeros(3)
    with pytest.raises(ValueError):
        _lib.gpr_predict_multi(x, z, [0, 3], np.zeros((2, 3)), [0, 3], 0.0, np.ones((1, 5)))
    with pytest.raises(ValueError):
        _lib.gpr_predict_multi(x, z, [0, 3], np.zeros((2, 3)), [0, 2], 0.0, np.ones((2, 5)))
    with pytest.raises(_lib.OiError, match='toffs must be non-decreasing'):
        _lib.gpr_predict_multi(x, z, [0, 1, 3], np.zeros((2, 3)), [0, 3, 2], 0.0, np.ones((2, 5)))


def test_nystrom_gpr_approx_many_targets_not_implemented():
    with pytest.raises(NotImplementedError, match='one target'):
        nystrom.GPR(np.zeros((4, 3)), np.zeros(4), np.zeros((2, 3)), [1.0, 1.0, 1.0], 1.0, 0.1, 0.0,
                    approx=True, M=2)
