"""``oi_gpr_sample`` without a GPU: the symbol is declared, exported and bound
(tests/test_abi.py compares its types with include/oi.h), every misuse is
rejected with OI_E_ARG (-1) and a message before any device work, and the
workspace the chunk planner counts for a cell equals the layout restated here
-- as tests/test_loo_abi.py checks for its entry point."""
import ctypes

import numpy as np
import pytest

import abi_ref
from optimalinterpolation_amd import _lib, gpr, nystrom

D, I64, I32, U64 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _i(*v):
    return np.array(v, dtype=np.int64)


def _call(lib, **over):
    """One cell with 3 observations, 2 targets and 4 draws; ``over`` replaces arguments."""
    a = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=_i(0, 3), ncell=1, xs=np.zeros((2, 3)), toffs=_i(0, 2),
             hyp=np.ones((1, 5)), nsamp=4, noise=0, jitter=0.0, seed=0, streams=None, xi=None,
             samples=np.zeros((2, 4)), fs=np.zeros(2), sd=np.zeros(2), status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_gpr_sample(_p(a['xyt'], D), _p(a['z'], D), _p(a['offs'], I64), a['ncell'], _p(a['xs'], D),
                             _p(a['toffs'], I64), 0.0, _p(a['hyp'], D), a['nsamp'], a['noise'], a['jitter'],
                             a['seed'], _p(a['streams'], U64), _p(a['xi'], D), _p(a['samples'], D), _p(a['fs'], D),
                             _p(a['sd'], D), _p(a['status'], I32), None)


def test_symbol_exported_and_bound():
    assert 'oi_gpr_sample' in _lib.SIGNATURES and abi_ref.nargs('oi_gpr_sample') == 19 == len(_lib.SIGNATURES['oi_gpr_sample'][1])
    assert {'oi_gpr_sample', 'oi_test_sample_normals', 'oi_test_sample_cell_doubles'} <= abi_ref.exported()
    assert callable(_lib.gpr_sample) and callable(_lib.gpr_sample_device)
    assert callable(gpr.sample_cells) and callable(nystrom.GPR_sample)


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(offs=None), b'null offs'),
    (dict(offs=_i(1, 3)), b'offs[0]'),
    (dict(offs=_i(0, 3, 2), ncell=2, toffs=_i(0, 1, 2), hyp=np.ones((2, 5))), b'offs must be non-decreasing'),
    (dict(toffs=None), b'null toffs'),
    (dict(toffs=_i(1, 2)), b'toffs[0]'),
    (dict(offs=_i(0, 1, 3), ncell=2, toffs=_i(0, 2, 1), hyp=np.ones((2, 5))), b'toffs must be non-decreasing'),
    (dict(xyt=None), b'null xyt / z'),
    (dict(z=None), b'null xyt / z'),
    (dict(xs=None), b'null xs'),
    (dict(hyp=None), b'null hyp'),
    (dict(samples=None), b'null samples'),
    (dict(status=None), b'null status'),
    (dict(nsamp=-1), b'nsamp'),
    (dict(noise=2), b'noise'),
    (dict(noise=-1), b'noise'),
    (dict(jitter=-1e-300), b'jitter'),
    (dict(jitter=float('nan')), b'jitter'),
    (dict(jitter=float('inf')), b'jitter'),
    # Np^2 doubles reach 2 GiB from n = 16 321 (Np = 16 384); no array of that size is touched
    (dict(offs=_i(0, 16321)), b'cell too large'),
    # X: (nt + 1) n doubles with n = 16 000, nt = 16 777
    (dict(offs=_i(0, 16000), toffs=_i(0, 16777)), b'cell too large'),
    # the padded C: Ntp = 16 384 from nt = 16 321 (X alone, 3 x 16 322 doubles, is small)
    (dict(toffs=_i(0, 16321)), b'cell too large'),
    # nt nsamp doubles: 2 x 2^27
    (dict(nsamp=1 << 27), b'cell too large'),
])
def test_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_misuse_leaves_outputs_untouched():
    lib = _lib.load()
    samples, fs, sd = np.full((2, 4), 7.0), np.full(2, 7.0), np.full(2, 7.0)
    for over in (dict(offs=_i(1, 3)), dict(nsamp=-1), dict(noise=3), dict(jitter=-1.0)):
        assert _call(lib, samples=samples, fs=fs, sd=sd, **over) == -1
    assert (samples == 7.0).all() and (fs == 7.0).all() and (sd == 7.0).all()


def test_empty_batch_is_a_noop():
    lib = _lib.load()
    z1 = np.zeros(1, dtype=np.int64)
    assert _call(lib, ncell=0, offs=z1, toffs=z1, xyt=None, z=None, xs=None, hyp=None, samples=None, fs=None,
                 sd=None, status=None) == 0
    # the scalars are checked all the same
    assert _call(lib, ncell=0, offs=z1, toffs=z1, nsamp=-1) == -1


def test_wrapper_rejects_inconsistent_batches():
    ok = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=[0, 3], xs=np.zeros((2, 3)), toffs=[0, 2], mean=0.0,
              hyp=np.ones((1, 5)), nsamp=4)
    for over in (dict(hyp=np.ones((2, 5))),              # hyp rows != ncell
                 dict(offs=[0, 2]),                      # offs[-1] != len(z)
                 dict(toffs=[0, 1]),                     # toffs[-1] != rows(xs)
                 dict(toffs=[0, 1, 2]),                  # len(toffs) != ncell + 1
                 dict(nsamp=-1),
                 dict(streams=[1, 2]),                   # streams != [ncell]
                 dict(xi=np.zeros((2, 3)))):             # xi != [T x nsamp]
        with pytest.raises(ValueError):
            _lib.gpr_sample(**{**ok, **over})


def _up(v, q):
    return (v + q - 1) // q * q


def _sample_form(n, nt, nsamp, host):
    """oi_gpr_predict_multi's cell without cov (tests/workspace_ref.py's
    predict_form) plus the draw's: the padded C and its factor's diagonal-block
    inverses of the cell's own, and its unrounded share of the chunk-wide Xi,
    samples and second info."""
    Np, Ntp = _up(n, 64), _up(nt, 64)
    own = _up(3 * n, 32) + _up(3 * nt, 32) + Np * Np + Np * 64 + _up((nt + 1) * n, 32) + Ntp * Ntp + Ntp * 64
    share = 2 * nt + 3 * nt + (4 * n if host else 0) + 2 + 2 * nt * nsamp + 1
    return own + share


def test_workspace_hook_equals_the_restated_layout():
    import workspace_ref as W
    fn = _lib.load().oi_test_sample_cell_doubles
    fn.restype, fn.argtypes = I64, [I64, I64, I64, I32]
    for n in (0, 1, 63, 64, 65, 333, 4600):
        for nt in (0, 1, 63, 64, 65, 121, 200):
            for nsamp in (0, 1, 64, 100, 257):
                for host in (False, True):
                    got = fn(n, nt, nsamp, W.HOST * host)
                    assert got == _sample_form(n, nt, nsamp, host), (n, nt, nsamp, host)
                    # the draw's own arrays on top of the prediction's cell, which stays as it is
                    base = W.cell_doubles(W.PREDICT, n, nt=nt, cov=False, host=host)
                    Ntp = _up(nt, 64)
                    assert got - base == Ntp * Ntp + Ntp * 64 + 2 * nt * nsamp + 1
