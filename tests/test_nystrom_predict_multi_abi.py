"""``oi_nystrom_predict_multi`` without a GPU: the symbol is declared,
exported and bound, and every misuse is rejected with OI_E_ARG (-1) and a
message before any device work -- as tests/test_predict_multi_abi.py checks for
``oi_gpr_predict_multi``."""
import ctypes

import numpy as np
import pytest

import abi_ref
from optimalinterpolation_amd import _lib, nystrom

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _i(*v):
    return np.array(v, dtype=np.int64)


def _call(lib, **over):
    """One cell with 3 observations, 2 inducing rows and 2 targets; ``over``
    replaces arguments."""
    a = dict(xyt=np.zeros((3, 3)), y=np.zeros(3), offs=_i(0, 3), ncell=1, sel=_i(0, 1), soffs=_i(0, 2),
             hyp=np.ones((1, 5)), xs=np.zeros((2, 3)), toffs=_i(0, 2), fs=np.zeros(2), sd=np.zeros(2),
             cov=np.zeros(4), status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_nystrom_predict_multi(_p(a['xyt'], D), _p(a['y'], D), _p(a['offs'], I64), a['ncell'],
                                        _p(a['sel'], I64), _p(a['soffs'], I64), _p(a['hyp'], D),
                                        _p(a['xs'], D), _p(a['toffs'], I64), 0.0, _p(a['fs'], D),
                                        _p(a['sd'], D), _p(a['cov'], D), _p(a['status'], I32), None)


def test_symbol_exported_and_bound():
    """The entry point is declared in include/oi.h with 15 arguments, is in
    _lib.SIGNATURES (tests/test_abi.py compares the two type by type) and is
    exported by the library."""
    assert 'oi_nystrom_predict_multi' in _lib.SIGNATURES and abi_ref.nargs('oi_nystrom_predict_multi') == 15 == len(_lib.SIGNATURES['oi_nystrom_predict_multi'][1])
    assert 'oi_nystrom_predict_multi' in abi_ref.exported()
    assert callable(_lib.nystrom_predict_multi)
    for name in ('GPR_multi', 'GPR_multi_batch', 'fit_predict_multi_batch'):
        assert callable(getattr(nystrom, name))


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(xyt=None), b'null pointer'),
    (dict(y=None), b'null pointer'),
    (dict(sel=None), b'null pointer'),
    (dict(offs=None), b'null offs'),
    (dict(soffs=None), b'null soffs'),
    (dict(toffs=None), b'null toffs'),
    (dict(hyp=None), b'null hyp'),
    (dict(status=None), b'null status'),
    (dict(xs=None), b'xs'),
    (dict(fs=None), b'fs'),
    (dict(sd=None), b'sd'),
    (dict(offs=_i(1, 3)), b'offs[0]'),
    (dict(toffs=_i(1, 2)), b'toffs[0]'),
    (dict(offs=_i(0, 3, 2), ncell=2, soffs=_i(0, 1, 2), toffs=_i(0, 1, 2), hyp=np.ones((2, 5))),
     b'offs must be non-decreasing'),
    (dict(xyt=np.zeros((6, 3)), y=np.zeros(6), offs=_i(0, 3, 6), ncell=2, soffs=_i(0, 1, 2),
          toffs=_i(0, 2, 1), hyp=np.ones((2, 5))), b'toffs must be non-decreasing'),
    (dict(sel=_i(0, 1, 2, 0), soffs=_i(0, 4)), b'1 <= M <= n'),
    (dict(sel=np.zeros(0, dtype=np.int64), soffs=_i(0, 0)), b'1 <= M <= n'),
    (dict(sel=_i(0, 3)), b'inducing index out of range'),
    (dict(hyp=np.array([[1.0, 1.0, 1.0, 1.0, 0.0]])), b'hypers must be > 0'),
    (dict(hyp=np.array([[1.0, -2.0, 1.0, 1.0, 0.1]])), b'hypers must be > 0'),
    (dict(hyp=np.array([[np.nan, 1.0, 1.0, 1.0, 0.1]])), b'hypers must be > 0'),
])
def test_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_misuse_leaves_outputs_untouched():
    lib = _lib.load()
    fs, sd, cov = np.full(2, 7.0), np.full(2, 7.0), np.full(4, 7.0)
    assert _call(lib, toffs=_i(1, 2), fs=fs, sd=sd, cov=cov) == -1
    assert (fs == 7.0).all() and (sd == 7.0).all() and (cov == 7.0).all()


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    z1 = np.zeros(1, dtype=np.int64)
    assert _call(lib, ncell=0, offs=z1, soffs=z1, toffs=z1, xyt=None, y=None, sel=None, hyp=None, xs=None,
                 fs=None, sd=None, cov=None, status=None) == 0


def test_wrapper_rejects_inconsistent_batches():
    x, y, sel = np.zeros((3, 3)), np.zeros(3), [0, 1]
    ok = dict(xyt=x, y=y, offs=[0, 3], sel=sel, soffs=[0, 2], hyp=np.ones((1, 5)), xs=np.zeros((2, 3)),
              toffs=[0, 2])
    for over in (dict(toffs=[0, 3]),                 # toffs[-1] != rows(xs)
                 dict(toffs=[1, 2]),                 # toffs[0] != 0
                 dict(toffs=[0, 1, 2]),              # len(toffs) != ncell + 1
                 dict(hyp=np.ones((2, 5))),          # hyp rows != ncell
                 dict(soffs=[0, 3]),                 # soffs[-1] != len(sel)
                 dict(offs=[0, 2]),                  # offs[-1] != len(y)
                 dict(xyt=np.zeros((2, 3)))):        # rows(xyt) != len(y)
        with pytest.raises(ValueError):
            _lib.nystrom_predict_multi(**{**ok, **over})
    with pytest.raises(_lib.OiError, match='toffs must be non-decreasing'):
        _lib.nystrom_predict_multi(np.zeros((6, 3)), np.zeros(6), [0, 3, 6], [0, 0], [0, 1, 2], np.ones((2, 5)),
                                   np.zeros((2, 3)), [0, 3, 2])


def test_gpr_approx_many_targets_points_to_gpr_multi():
    with pytest.raises(NotImplementedError, match='one target.*GPR_multi'):
        nystrom.GPR(np.zeros((4, 3)), np.zeros(4), np.zeros((2, 3)), [1.0, 1.0, 1.0], 1.0, 0.1, 0.0,
                    approx=True, M=2)
