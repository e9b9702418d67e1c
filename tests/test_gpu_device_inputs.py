"""Device-tensor inputs (``device_inputs=True``) of the entries no other test
covers: they give the host-array result bit for bit, and a tensor liboi could
not read safely -- wrong dtype, strided, wrong size, or living on another GPU
than ``device=`` -- is a ValueError raised by the binding, before any library
call (gpr_batch_device, gpr_predict_multi_device, svgp_predict and svgp_elbo
have their equality tests next to their other tests)."""
import numpy as np
import pytest
import torch

from optimalinterpolation_amd import _lib, nystrom, synthetic

pytestmark = pytest.mark.gpu

M_SVGP = 8
P_SVGP = 6 + 4 * M_SVGP + M_SVGP * (M_SVGP + 1) // 2


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=p.dtype.kind == 'f') for p, q in zip(a, b))


class Data:
    def __init__(self):
        c = synthetic.make_cells([40, 70], seed=21)
        self.c = c
        self.y = c.z - c.mean
        self.sel, self.soffs = nystrom._ragged_sel(c.offs, np.array([8, 33]))
        self.x0 = nystrom.default_x0()
        self.xd = torch.from_numpy(c.xyt).cuda()
        self.yd = torch.from_numpy(self.y).cuda()
        self.Z0 = np.stack([c.xyt[c.offs[k]:c.offs[k] + M_SVGP] for k in range(2)])
        self.init = np.tile([25e3, 25e3, 1.0, 1.0, 0.1, 0.3], (2, 1))

    def nystrom_fit(self, x, y, **kw):
        return _lib.nystrom_fit_batch(x, y, self.c.offs, self.sel, self.soffs, self.x0, self.c.xs,
                                      self.c.mean, maxiter=3, **kw)

    def nystrom_submit(self, s, x, y):
        return s.submit(x, y, self.c.offs, self.sel, self.soffs, self.x0, self.c.xs, self.c.mean)

    def svgp(self, x, y, **kw):
        return _lib.svgp_batch(x, y, self.c.offs, self.Z0, self.init, self.c.xs, batch=16, iterations=5,
                               log_every=2, seed=3, want_params=True, **kw)


@pytest.fixture(scope='module')
def d():
    return Data()


@pytest.fixture(scope='module')
def nystrom_host(d):
    return d.nystrom_fit(d.c.xyt, d.y)


def test_nystrom_fit_batch(d, nystrom_host):
    assert _same(d.nystrom_fit(d.xd, d.yd, device_inputs=True), nystrom_host)


def test_nystrom_session(d, nystrom_host):
    with _lib.NystromSession(device_inputs=True, maxiter=3) as s:
        got = s.wait(d.nystrom_submit(s, d.xd, d.yd))
    assert _same(got, nystrom_host)


def test_svgp_batch(d):
    host = d.svgp(d.c.xyt, d.y)
    assert host[2].shape == (2, P_SVGP) and host[3].shape == (2, 3)
    assert _same(d.svgp(d.xd, d.yd, device_inputs=True), host)


def test_smooth_fields_device():
    rng = np.random.default_rng(22)
    f = rng.normal(0.3, 0.1, (2, 12, 12))
    f[rng.random(f.shape) < 0.3] = np.nan
    mask = (rng.random((12, 12)) < 0.8).astype(float)
    g = np.arange(-1, 2)
    kern = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / 2.0)
    kern /= kern.sum()
    host = _lib.smooth_fields(f, 1.0, mask, kern)
    out = torch.empty(2, 12, 12, dtype=torch.float64, device='cuda')
    got = _lib.smooth_fields_device(torch.from_numpy(f).cuda(), 1.0, torch.from_numpy(mask).cuda(), kern, out)
    assert got is out and np.isnan(f).any()
    assert np.array_equal(out.cpu().numpy(), host, equal_nan=True)


def _in_session(cls, submit):
    def call(x, y, device):
        with cls(device_inputs=True) as s:   # on cuda:0; ``device`` is what a session on that GPU holds
            s.device = device
            submit(s, x, y)
    return call


def _entries(d):
    c = d.c
    th = np.zeros((2, P_SVGP))
    return {
        'nystrom_fit_batch': lambda x, y, dev: d.nystrom_fit(x, y, device_inputs=True, device=dev),
        'svgp_batch': lambda x, y, dev: d.svgp(x, y, device_inputs=True, device=dev),
        # its targets play xyt's part: [N x 3] cut by offs
        'svgp_predict': lambda x, y, dev: _lib.svgp_predict(th, x, c.offs, device_inputs=True, device=dev),
        'svgp_elbo': lambda x, y, dev: _lib.svgp_elbo(th, x, y, c.offs, device_inputs=True, device=dev),
        'Session': _in_session(_lib.Session, lambda s, x, y: s.submit(
            x, y, c.offs, c.xs, c.mean, opt=False, hyp=np.tile(synthetic.FIXED_HYPERS, (2, 1)))),
        'NystromSession': _in_session(_lib.NystromSession, d.nystrom_submit),
    }


ENTRIES = ['nystrom_fit_batch', 'svgp_batch', 'svgp_predict', 'svgp_elbo', 'Session', 'NystromSession']


@pytest.mark.parametrize('name', ENTRIES)
@pytest.mark.parametrize('kind', ['float32', 'strided', 'count', 'ordinal'])
def test_refused_before_any_library_call(d, name, kind):
    """On a one-GPU machine a library call with device=1 would be an OiError
    ("bad device ordinal"); on a larger one it would launch on cuda:1 kernels
    that read cuda:0's memory.  Neither happens: the binding raises first."""
    x, y, dev = d.xd, d.yd, 0
    if kind == 'float32':
        x = x.float()
    elif kind == 'strided':
        x = x.t().contiguous().t()
        assert x.shape == d.xd.shape and not x.is_contiguous()
    elif kind == 'count':
        x = x[:-1]
    else:
        dev = 1
    with pytest.raises(ValueError, match={'float32': 'float64', 'strided': 'contiguous', 'count': 'elements',
                                          'ordinal': 'cuda:1'}[kind]):
        _entries(d)[name](x, y, dev)
