"""``oi_gpr_loo`` (include/oi_loo.h) without a GPU: the symbol is exported and
bound type by type, include/oi.h keeps its 32 prototypes, and every misuse is
rejected with OI_E_ARG (-1) and a message before any device work -- as
tests/test_nystrom_predict_multi_abi.py checks for its entry point."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from optimalinterpolation_amd import _lib, gpr, nystrom

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32


def _ctype(decl):
    """The ctypes type of a C type as the header spells it."""
    t = re.sub(r'\s+', ' ', re.sub(r'\bconst\b', '', decl)).strip().replace(' *', '*')
    scalar = {'double': ctypes.c_double, 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'int': ctypes.c_int}
    if t in scalar:
        return scalar[t]
    if t.endswith('*') and t[:-1] in scalar:
        return ctypes.POINTER(scalar[t[:-1]])
    assert t == 'oi_options*', f"unmapped C type {decl!r}"
    return ctypes.POINTER(_lib.OiOptions)


def _protos(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    return re.findall(r'([A-Za-z_][\w\s\*]*?)\b(oi_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)


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
    protos = _protos('oi_loo.h')
    assert [n for _, n, _ in protos] == ['oi_gpr_loo'] == list(_lib.SIGNATURES_LOO)
    assert not set(_lib.SIGNATURES_LOO) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_NYSTROM_MULTI))
    lib = _lib.load()
    for ret, name, args in protos:
        want = [_ctype(re.match(r'(.*?)\w+$', a.strip()).group(1)) for a in args.split(',')]
        restype, argtypes = _lib.SIGNATURES_LOO[name]
        ret = ret.strip().splitlines()[-1]    # the pattern's first group starts at the preceding #endif
        assert (restype, list(argtypes)) == (_ctype(ret), want)
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, list(argtypes)) and len(argtypes) == 11
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\b[TW] oi_gpr_loo\b', out)
    assert callable(_lib.gpr_loo) and callable(_lib.gpr_loo_device)
    assert callable(gpr.loo_cells) and callable(nystrom.GPR_loo)


def test_oi_h_keeps_its_32_prototypes():
    names = [n for _, n, _ in _protos('oi.h')]
    assert len(names) == 32 and 'oi_gpr_loo' not in names


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
