"""``oi_gpr_predict_grad`` without a GPU: include/oi_ext.h, the header of the
entries after oi.h's, agrees with ``_lib.EXT_SIGNATURES`` type by type; the
symbol and its test hook are exported; every misuse is rejected with OI_E_ARG
(-1) and a message before any device work; the ``_lib`` wrapper refuses
inconsistent batches; and the workspace the chunk planner counts for a cell
equals the layout restated here."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_ref
from abi_ref import _ctype
from conftest import ROOT
from optimalinterpolation_amd import _lib, gpr, nystrom

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32
EXT_HEADER = os.path.join(ROOT, 'include', 'oi_ext.h')


def _ext_protos():
    """(return type, name, [argument types]) of every prototype of include/oi_ext.h."""
    src = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', open(EXT_HEADER).read(), flags=re.S))
    src = re.sub(r'^\s*#[^\n]*$', '', src, flags=re.M)        # preprocessor lines
    out = []
    for ret, name, args in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(oi_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')] if args.strip() not in ('', 'void') else []
        out.append((ret.strip(), name, [re.match(r'(.*?)\w+$', a).group(1) for a in args]))
    return out


def test_ext_header_matches_ext_signatures():
    protos = _ext_protos()
    assert sorted(n for _, n, _ in protos) == sorted(_lib.EXT_SIGNATURES) and 'oi_gpr_predict_grad' in _lib.EXT_SIGNATURES
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert re.search(r'#include\s+"oi\.h"', open(EXT_HEADER).read())
    lib = _lib.load()
    for ret, name, args in protos:
        want = [_ctype(a) for a in args]
        restype, argtypes = _lib.EXT_SIGNATURES[name]
        assert (restype, list(argtypes)) == (_ctype(ret), want), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, list(argtypes)), name
    assert len(_lib.EXT_SIGNATURES['oi_gpr_predict_grad'][1]) == 16


def test_symbol_and_hook_exported():
    assert {'oi_gpr_predict_grad', 'oi_test_grad_cell_doubles'} <= abi_ref.exported()
    assert callable(_lib.gpr_predict_grad) and callable(_lib.gpr_predict_grad_device) and callable(_lib.split_jcov)
    assert callable(gpr.grad_cells) and callable(nystrom.GPR_grad)


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _i(*v):
    return np.array(v, dtype=np.int64)


def _call(lib, **over):
    """One cell with 3 observations and 2 targets; ``over`` replaces arguments."""
    a = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=_i(0, 3), ncell=1, xs=np.zeros((2, 3)), toffs=_i(0, 2),
             hyp=np.ones((1, 5)), grad=np.zeros((2, 3)), gsd=np.zeros((2, 3)), fs=np.zeros(2), sd=np.zeros(2),
             blk=None, cov=None, status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_gpr_predict_grad(_p(a['xyt'], D), _p(a['z'], D), _p(a['offs'], I64), a['ncell'], _p(a['xs'], D),
                                   _p(a['toffs'], I64), 0.0, _p(a['hyp'], D), _p(a['grad'], D), _p(a['gsd'], D),
                                   _p(a['fs'], D), _p(a['sd'], D), _p(a['blk'], D), _p(a['cov'], D),
                                   _p(a['status'], I32), None)


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(offs=None), b'null offs'),
    (dict(offs=_i(1, 3)), b'offs[0]'),
    (dict(offs=_i(0, 3, 2), ncell=2, toffs=_i(0, 1, 2), hyp=np.ones((2, 5))), b'offs must be non-decreasing'),
    (dict(toffs=None), b'null toffs'),
    (dict(toffs=_i(1, 2)), b'toffs[0]'),
    (dict(offs=_i(0, 1, 3), ncell=2, toffs=_i(0, 2, 1), hyp=np.ones((2, 5))), b'toffs must be non-decreasing'),
    (dict(status=None), b'null status'),
    (dict(hyp=None), b'null hyp'),
    (dict(xyt=None), b'null xyt / z'),
    (dict(z=None), b'null xyt / z'),
    (dict(xs=None), b'null xs / grad / gsd'),
    (dict(grad=None), b'null xs / grad / gsd'),
    (dict(gsd=None), b'null xs / grad / gsd'),
    # K: Np^2 doubles reach 2 GiB from n = 16 321 (Np = 16 384); no array of that size is touched
    (dict(offs=_i(0, 16321)), b'cell too large'),
    # X: (4 nt + 1) n doubles with n = 16 320 (K fits), nt = 4 112; without cov, whose 16 nt^2 would reach it too
    (dict(offs=_i(0, 16320), toffs=_i(0, 4112)), b'cell too large'),
    # X's row count alone, 4 nt + 1, in a cell WITHOUT observations (X is empty, cov not asked for): it must stay
    # an int in the kernels, so the same limit holds for it
    (dict(xyt=None, z=None, offs=_i(0, 0), toffs=_i(0, 1 << 29)), b'cell too large'),
    (dict(xyt=None, z=None, offs=_i(0, 0), toffs=_i(0, 1 << 26)), b'cell too large'),
    # cov: 16 nt^2 = 2^28 doubles at nt = 4 096, X (16 385 x 3) small
    (dict(toffs=_i(0, 4096), cov=np.zeros(1)), b'cell too large'),
])
def test_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_the_limit_cases_sit_on_the_gradients_own_limits():
    """The X and cov cases above reach the limit through the 4 rows per target
    and are the smallest that do; oi_gpr_predict_multi's X, (nt + 1) n, is far
    from it at that shape."""
    LIM = 0x7FFFFFF0 // 8
    assert (4 * 4112 + 1) * 16320 >= LIM > (4 * 4111 + 1) * 16320 and 16 * 4096 ** 2 >= LIM > 16 * 4095 ** 2
    assert (4112 + 1) * 16320 < LIM and 16320 ** 2 < LIM <= 16384 ** 2


def test_misuse_leaves_outputs_untouched():
    lib = _lib.load()
    grad, gsd, fs, sd = np.full((2, 3), 7.0), np.full((2, 3), 7.0), np.full(2, 7.0), np.full(2, 7.0)
    for over in (dict(offs=_i(1, 3)), dict(hyp=None), dict(xs=None), dict(status=None)):
        assert _call(lib, grad=grad, gsd=gsd, fs=fs, sd=sd, **over) == -1
    assert (grad == 7.0).all() and (gsd == 7.0).all() and (fs == 7.0).all() and (sd == 7.0).all()


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    z1 = np.zeros(1, dtype=np.int64)
    assert _call(lib, ncell=0, offs=z1, toffs=z1, xyt=None, z=None, xs=None, hyp=None, grad=None, gsd=None, fs=None,
                 sd=None, status=None) == 0


def test_wrapper_rejects_inconsistent_batches():
    ok = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=[0, 3], xs=np.zeros((2, 3)), toffs=[0, 2], mean=0.0,
              hyp=np.ones((1, 5)))
    for over in (dict(hyp=np.ones((2, 5))),              # hyp rows != ncell
                 dict(offs=[0, 2]),                      # offs[-1] != len(z)
                 dict(offs=[1, 3]),                      # offs[0] != 0
                 dict(toffs=[0, 1]),                     # toffs[-1] != rows(xs)
                 dict(toffs=[0, 1, 2])):                 # len(toffs) != ncell + 1
        with pytest.raises(ValueError):
            _lib.gpr_predict_grad(**{**ok, **over})


def test_wrapper_rejects_a_cpu_tensor_as_device_input():
    import torch
    x, z = torch.zeros((3, 3), dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError, match='must live on cuda'):
        _lib.gpr_predict_grad_device(x, z, [0, 3], np.zeros((2, 3)), [0, 2], 0.0, np.ones((1, 5)))
    with pytest.raises(ValueError):
        _lib.gpr_predict_grad_device(np.zeros((3, 3)), np.zeros(3), [0, 3], np.zeros((2, 3)), [0, 2], 0.0,
                                     np.ones((1, 5)))


def test_split_jcov_returns_views():
    toffs = [0, 2, 2, 5]
    flat = np.arange(16 * (4 + 0 + 9), dtype=np.float64)
    parts = _lib.split_jcov(flat, toffs)
    assert [p.shape for p in parts] == [(8, 8), (0, 0), (12, 12)]
    assert parts[0][0, 0] == 0 and parts[2][0, 0] == 64 and parts[2][11, 11] == flat[-1]
    assert all(p.base is not None and np.shares_memory(p, flat) for p in parts if p.size)


def _up(v, q):
    return (v + q - 1) // q * q


def _grad_form(n, nt, cov, host):
    """oi_gpr_predict_multi's cell (tests/workspace_ref.py's predict_form) with
    (4 nt + 1) n for X and 16 nt^2 for cov, plus its unrounded share of the
    chunk-wide outputs as they are carved: grad 3 nt, gsd 3 nt and blk 16 nt
    (always: gsd is taken from it)."""
    Np = _up(n, 64)
    own = _up(3 * n, 32) + _up(3 * nt, 32) + Np * Np + Np * 64 + _up((4 * nt + 1) * n, 32)
    share = (16 * nt * nt if cov else 0) + 2 * nt + 3 * nt + (4 * n if host else 0) + 2
    return own + share + 2 * 3 * nt + 16 * nt


def test_workspace_hook_equals_the_restated_layout():
    import workspace_ref as W
    fn = _lib.load().oi_test_grad_cell_doubles
    fn.restype, fn.argtypes = I64, [I64, I64, I32]
    for n in (0, 1, 64, 65):
        for nt in (0, 1, 16):
            for cov in (False, True):
                for host in (False, True):
                    got = fn(n, nt, W.COV * cov + W.HOST * host)
                    assert got == _grad_form(n, nt, cov, host), (n, nt, cov, host)
                    # on top of the prediction's cell, which stays as it is
                    base = W.cell_doubles(W.PREDICT, n, nt=nt, cov=cov, host=host)
                    assert base == W.predict_form(n, nt, cov, host)
                    assert got - base == (_up((4 * nt + 1) * n, 32) - _up((nt + 1) * n, 32)
                                          + (15 * nt * nt if cov else 0) + 22 * nt)
