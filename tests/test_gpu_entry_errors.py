"""Every entry family refuses a device ordinal that does not exist in the same
way: code OI_E_ARG (-1), "bad device ordinal", before any HIP work -- and the
library goes on working afterwards.  Pins the device check that all entry
points share (csrc/oi_host.h, oi_select_device)."""
import numpy as np
import pytest

from optimalinterpolation_amd import _lib, nystrom, synthetic

pytestmark = pytest.mark.gpu

BAD = 99


def _one_cell():
    c = synthetic.make_cells([60], seed=4)
    hyp = np.array([synthetic.FIXED_HYPERS])
    sel, soffs = nystrom._ragged_sel(c.offs, np.array([12]))
    return c, hyp, sel, soffs


def _calls():
    c, hyp, sel, soffs = _one_cell()
    y = c.z - c.mean
    x0 = nystrom.default_x0()
    pts = c.xyt[:, :2]
    return c, hyp, {
        'gpr_batch': lambda **k: _lib.gpr_batch(c.xyt, c.z, c.offs, c.xs, c.mean, opt=False, hyp=hyp, **k),
        'nlml_grad_batch': lambda **k: _lib.nlml_grad_batch(c.xyt, c.z, np.full(60, c.mean), c.offs,
                                                            np.zeros((1, 6)), **k),
        'nystrom_batch': lambda **k: _lib.nystrom_batch(c.xyt, y, c.offs, sel, soffs, hyp, xs=c.xs,
                                                        mean=c.mean, **k),
        'nystrom_fit_batch': lambda **k: _lib.nystrom_fit_batch(c.xyt, y, c.offs, sel, soffs, x0, c.xs,
                                                                c.mean, **k),
        'svgp_batch': lambda **k: _lib.svgp_batch(c.xyt, c.z, c.offs, c.xyt[None, :8],
                                                  [[25e3, 25e3, 1.0, 1.0, 0.1, 0.3]], c.xs, batch=16,
                                                  iterations=1, **k),
        'gpr_predict_multi': lambda **k: _lib.gpr_predict_multi(c.xyt, c.z, c.offs, c.xs, [0, 1], c.mean,
                                                                hyp, cov=True, **k),
        'smooth_fields': lambda **k: _lib.smooth_fields(np.ones((1, 8, 8)), 1.0, np.ones((8, 8)),
                                                        np.full((3, 3), 1 / 9), **k),
        'ball_query': lambda **k: _lib.ball_query(pts, pts[:3], 1e5, **k),
        'Session': lambda **k: _lib.Session(**k),
        'NystromSession': lambda **k: _lib.NystromSession(**k),
    }


def test_bad_device_ordinal_everywhere_then_a_good_call():
    c, hyp, calls = _calls()
    for name, call in calls.items():
        with pytest.raises(_lib.OiError) as e:
            call(device=BAD)
        print(name, '->', e.value)
        assert 'bad device ordinal' in str(e.value), name
        if 'Session' not in name:  # the create calls return a null handle, not a code
            assert str(e.value).startswith('liboi error -1:'), name
    out, st, _ = calls['gpr_batch'](device=0)
    assert st[0] == 0 and np.all(np.isfinite(out))
