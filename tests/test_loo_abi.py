"""``oi_gpr_loo`` without a GPU: the symbol is declared, exported and bound
(tests/test_abi.py compares its types with include/oi.h), and every misuse is
rejected with OI_E_ARG (-1) and a message before any device work -- as
tests/test_nystrom_predict_multi_abi.py checks for its entry point."""
import ctypes

import numpy as np
import pytest

import abi_ref
from optimalinterpolation_amd import _lib, gpr, nystrom

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _i(*v):
    return np.array(v, dtype=np.int64)


def _call(lib, **over):
    """One cell with 3 observations; ``over`` replaces arguments."""
    a = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=_i(0, 3), ncell=1, hyp=np.ones((1, 5)), mu=np.zeros(3),
             sd=np.zeros(3), lpl=np.zeros(1), status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_gpr_loo(_p(a['xyt'], D), _p(a['z'], D), _p(a['offs'], I64), a['ncell'], 0.0, _p(a['hyp'], D),
                          _p(a['mu'], D), _p(a['sd'], D), _p(a['lpl'], D), _p(a['status'], I32), None)


def test_symbol_exported_and_bound():
    assert 'oi_gpr_loo' in _lib.SIGNATURES and abi_ref.nargs('oi_gpr_loo') == 11 == len(_lib.SIGNATURES['oi_gpr_loo'][1])
    assert 'oi_gpr_loo' in abi_ref.exported()
    assert callable(_lib.gpr_loo) and callable(_lib.gpr_loo_device)
    assert callable(gpr.loo_cells) and callable(nystrom.GPR_loo)


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(offs=None), b'null offs'),
    (dict(offs=_i(1, 3)), b'offs[0]'),
    (dict(offs=_i(0, 3, 2), ncell=2, hyp=np.ones((2, 5))), b'offs must be non-decreasing'),
    (dict(xyt=None), b'null xyt / z'),
    (dict(z=None), b'null xyt / z'),
    (dict(hyp=None), b'null hyp'),
    (dict(mu=None), b'null mu / sd'),
    (dict(sd=None), b'null mu / sd'),
    (dict(status=None), b'null status'),
    # Np^2 doubles reach 2 GiB from n = 16 321 (Np = 16 384); no array of that size is touched
    (dict(offs=_i(0, 16321)), b'cell too large'),
])
def test_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_misuse_leaves_outputs_untouched():
    lib = _lib.load()
    mu, sd, lpl = np.full(3, 7.0), np.full(3, 7.0), np.full(1, 7.0)
    assert _call(lib, offs=_i(1, 3), mu=mu, sd=sd, lpl=lpl) == -1
    assert (mu == 7.0).all() and (sd == 7.0).all() and (lpl == 7.0).all()


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    assert _call(lib, ncell=0, offs=np.zeros(1, dtype=np.int64), xyt=None, z=None, hyp=None, mu=None, sd=None,
                 lpl=None, status=None) == 0


def test_wrapper_rejects_inconsistent_batches():
    ok = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=[0, 3], mean=0.0, hyp=np.ones((1, 5)))
    for over in (dict(hyp=np.ones((2, 5))),          # hyp rows != ncell
                 dict(offs=[0, 2]),                  # offs[-1] != len(z)
                 dict(offs=[1, 3]),                  # offs[0] != 0
                 dict(xyt=np.zeros((2, 3)))):        # rows(xyt) != len(z)
        with pytest.raises(ValueError):
            _lib.gpr_loo(**{**ok, **over})
