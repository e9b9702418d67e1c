"""GPU parity of ``oi_gpr_predict_multi``: prediction at many targets per cell
with the full posterior covariance (GP_example.ipynb code cell 1, ``GPR`` with
``xs`` ns x 3; GPR_CS2S3.py GPR:173-182 with ns columns).

Reference: ``oracle.gp_oracle.matern32`` plus numpy, the formulas of
``gp_oracle.predict`` keeping the whole ``Kxs - v'v`` (``_ref_cell`` below).
Bounds, fixed before any GPU run:
  fs, sd, lz   |gpu - ref| <= 1e-10 * max(1, |ref|)     (T1, test_gpu_nystrom's RTOL)
  cov          |gpu - ref| <= 1e-10 * max(sf2, |ref|)   entrywise
The reference's own spread under re-ordered observations on these inputs is
<= 2.3e-17 absolute in cov (about 2e-12 sf2 at the smallest sf2), 3e-15 in fs
and 2e-15 in sd, well inside the bounds.  Batch mates, chunking and device
inputs must not change a bit of a cell's results.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, gpr, nystrom, synthetic
import workspace_ref as W

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _ref_cell(x, y, xs, mean, hyp):
    """(fs [nt], sd [nt], lZ, cov [nt x nt]) of one cell; LinAlgError propagates."""
    ell, sf2, sn2 = list(hyp[:3]), hyp[3], hyp[4]
    n, nt = len(y), len(xs)
    Kxs = O.matern32(xs, ell, sf2) if nt else np.zeros((0, 0))
    if n == 0:  # GPR3D on an empty neighbourhood: the prior
        return np.full(nt, mean), np.sqrt(Kxs.diagonal()), -0.0, Kxs
    Kx = O.matern32(x, ell, sf2)
    L = np.linalg.cholesky(Kx + np.eye(n) * sn2)
    resid = y - np.ones(n) * mean
    A = np.linalg.solve(L.T, np.linalg.solve(L, resid))
    lZ = - np.dot(resid.T, A) / 2 - np.log(L.diagonal()).sum() - n * np.log(2 * np.pi) / 2
    if nt == 0:
        return np.zeros(0), np.zeros(0), lZ, Kxs
    Kxsx = O.matern32(x, ell, sf2, xs=xs)
    v = np.linalg.solve(L, Kxsx)
    cov = Kxs - np.dot(v.T, v)
    return mean + np.dot(Kxsx.T, A), np.sqrt(cov.diagonal()), lZ, cov


def _lattice(centre, nt, spacing=25e3):
    """nt targets on a square lattice (25 km) centred on ``centre``, at its t."""
    side = int(np.ceil(np.sqrt(max(nt, 1))))
    g = (np.arange(side) - (side - 1) / 2) * spacing
    gx, gy = np.meshgrid(g, g, indexing='ij')
    p = np.stack([centre[0] + gx.ravel(), centre[1] + gy.ravel(), np.full(side * side, centre[2])], axis=1)
    return p[:nt]


class Batch:
    """A ragged batch with a list of targets per cell, and its reference."""

    def __init__(self, cells, mean):
        # cells: list of (x [n x 3], y [n], xs [nt x 3], hyp [5])
        self.cells = cells
        self.mean = float(mean)
        self.xyt = np.ascontiguousarray(np.concatenate([c[0].reshape(-1, 3) for c in cells]))
        self.z = np.concatenate([c[1] for c in cells])
        self.xs = np.ascontiguousarray(np.concatenate([c[2].reshape(-1, 3) for c in cells]))
        self.offs = np.concatenate([[0], np.cumsum([len(c[1]) for c in cells])]).astype(np.int64)
        self.toffs = np.concatenate([[0], np.cumsum([len(c[2]) for c in cells])]).astype(np.int64)
        self.hyp = np.stack([c[3] for c in cells])
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = [_ref_cell(c[0], c[1], c[2], self.mean, c[3]) for c in self.cells]
        return self._ref

    def run(self, **kw):
        fs, sd, lz, cov, st = _lib.gpr_predict_multi(self.xyt, self.z, self.offs, self.xs, self.toffs,
                                                     self.mean, self.hyp, cov=True, lz=True, **kw)
        return fs, sd, lz, cov, st

    def subset(self, idx):
        return Batch([self.cells[i] for i in idx], self.mean)


def _same(a, b):
    """Bit for bit (NaN equal to NaN)."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def _check_against_ref(b, res):
    fs, sd, lz, cov, st = res
    covs = _lib.split_cov(cov, b.toffs)
    assert not st.any()
    for c, (rfs, rsd, rlz, rcov) in enumerate(b.ref()):
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        sf2 = b.hyp[c, 3]
        efs = np.abs(fs[t0:t1] - rfs).max(initial=0.0)
        esd = np.abs(sd[t0:t1] - rsd).max(initial=0.0)
        ecov = np.abs(covs[c] - rcov).max(initial=0.0)
        print(f"cell {c}: n {len(b.cells[c][1])} nt {t1 - t0} |dfs| {efs:.3e} |dsd| {esd:.3e} "
              f"|dlz| {abs(lz[c] - rlz):.3e} |dcov|/sf2 {ecov / sf2:.3e}")
        assert np.all(np.abs(fs[t0:t1] - rfs) <= RTOL * np.maximum(1.0, np.abs(rfs))), c
        assert np.all(np.abs(sd[t0:t1] - rsd) <= RTOL * np.maximum(1.0, np.abs(rsd))), c
        assert abs(lz[c] - rlz) <= RTOL * max(1.0, abs(rlz)), c
        assert np.all(np.abs(covs[c] - rcov) <= RTOL * np.maximum(sf2, np.abs(rcov))), c


@pytest.fixture(scope='module')
def fixture_batch():
    """Every cell of gpr3d.npz (n = 0 .. 300) at hyp2 with a 5 x 5 lattice of targets."""
    d = load_golden('gpr3d.npz')
    cells = []
    for c in range(len(d['offs']) - 1):
        a, e = d['offs'][c], d['offs'][c + 1]
        cells.append((d['x'][a:e], d['y'][a:e], _lattice(d['xs'][c], 25), d['hyp2'][c]))
    return Batch(cells, float(d['mean']))


N_EDGE = (1, 2, 63, 64, 65, 127, 128, 129, 200)
NT_EDGE = (1, 15, 16, 17, 63, 64, 65, 130, 0)


@pytest.fixture(scope='module')
def edge_batch():
    """Cells of predict64.npz truncated to the tile edges, one ragged batch."""
    d = load_golden('predict64.npz')
    cells = []
    for c, (n, nt) in enumerate(zip(N_EDGE, NT_EDGE)):
        a = d['offs'][c]
        cells.append((d['x'][a:a + n], d['y'][a:a + n], _lattice(d['xs'][c], nt), d['hyp'][c]))
    return Batch(cells, float(d['mean']))


@pytest.fixture(scope='module')
def edge_result(edge_batch):
    return edge_batch.run()


def test_fixture_cells(fixture_batch):
    b = fixture_batch
    assert 0 in np.diff(b.offs)
    for (_, _, _, rcov) in b.ref():
        assert np.linalg.eigvalsh(rcov).min() > 0
    _check_against_ref(b, b.run())


def test_tile_edges_ragged_batch(edge_batch, edge_result):
    _check_against_ref(edge_batch, edge_result)


def test_batch_equals_single(edge_batch, edge_result):
    fs, sd, lz, cov, st = edge_result
    covs = _lib.split_cov(cov, edge_batch.toffs)
    for c in range(len(edge_batch.cells)):
        t0, t1 = edge_batch.toffs[c], edge_batch.toffs[c + 1]
        one = edge_batch.subset([c]).run()
        assert _same(one, (fs[t0:t1], sd[t0:t1], lz[c:c + 1], covs[c].ravel(), st[c:c + 1])), c


def test_chunking_is_bitwise_neutral(edge_batch, edge_result):
    _lib.profile_reset()
    res = edge_batch.run(pool_bytes=768 * 1024, profile=True)
    chunks = _lib.profile_json()['kernels']['pm_reduce']['launches']
    _lib.profile_reset()
    assert chunks >= 3, chunks
    assert _same(res, edge_result)


def test_cell_larger_than_the_pool_is_nomem(edge_batch):
    with pytest.raises(_lib.OiError, match=r'error -3.*pool_bytes'):
        # the n = 200 cell alone (workspace_ref.cell_doubles(W.PREDICT, 200, 0, cov=True) doubles) needs ~0.65 MiB
        edge_batch.run(pool_bytes=256 * 1024)


def test_pool_that_fits_the_largest_cell_exactly():
    """A pool of exactly the planner's count for the larger cell (plus the
    chunk's slack) holds the call, one cell per chunk; one double less does not."""
    d = load_golden('predict64.npz')
    cells = []
    for c, n in enumerate((65, 1)):
        a = d['offs'][c]
        cells.append((d['x'][a:a + n], d['y'][a:a + n], _lattice(d['xs'][c], n), d['hyp'][c]))
    b = Batch(cells, float(d['mean']))
    free = b.run()
    fit = 8 * (W.SLACK[W.PREDICT] + W.cell_doubles(W.PREDICT, 65, 65, cov=True))
    assert not free[4].any()
    assert _same(b.run(pool_bytes=fit), free)
    with pytest.raises(_lib.OiError, match=r"error -3: a cell's prediction workspace does not fit pool_bytes"):
        b.run(pool_bytes=fit - 8)


def test_failed_cell_is_nan_and_mates_unchanged(edge_batch, edge_result):
    d = load_golden('predict64.npz')
    a = d['offs'][20]
    hyp = d['hyp'][20].copy()
    hyp[4] = -2.0 * hyp[3]  # first pivot sf2 + sn2 <= 0
    bad = (d['x'][a:a + 100], d['y'][a:a + 100], _lattice(d['xs'][20], 70), hyp)
    with pytest.raises(np.linalg.LinAlgError):
        _ref_cell(bad[0], bad[1], bad[2], edge_batch.mean, hyp)
    k = 4
    cells = edge_batch.cells[:k] + [bad] + edge_batch.cells[k:]
    b = Batch(cells, edge_batch.mean)
    fs, sd, lz, cov, st = b.run()
    covs = _lib.split_cov(cov, b.toffs)
    t0, t1 = b.toffs[k], b.toffs[k + 1]
    assert st[k] == 1 and st.sum() == 1
    assert np.isnan(fs[t0:t1]).all() and np.isnan(sd[t0:t1]).all() and np.isnan(lz[k])
    assert covs[k].shape == (70, 70) and np.isnan(covs[k]).all()
    keep = [c for c in range(len(cells)) if c != k]
    mates = (np.concatenate([fs[:t0], fs[t1:]]), np.concatenate([sd[:t0], sd[t1:]]), lz[keep],
             np.concatenate([covs[c].ravel() for c in keep]), st[keep])
    assert _same(mates, edge_result)


def test_covariance_symmetric_and_diagonal(fixture_batch, edge_batch, edge_result):
    for b, res in ((edge_batch, edge_result), (fixture_batch, fixture_batch.run())):
        fs, sd, lz, cov, st = res
        for c, C in enumerate(_lib.split_cov(cov, b.toffs)):
            t0, t1 = b.toffs[c], b.toffs[c + 1]
            assert np.array_equal(C, C.T), c
            s = np.sqrt(C.diagonal())
            assert np.all(np.abs(s - sd[t0:t1]) <= RTOL * np.maximum(1.0, np.abs(sd[t0:t1]))), c


def test_agrees_with_single_target_path():
    d = load_golden('gpr3d.npz')
    ncell = len(d['offs']) - 1
    out, st1, _ = _lib.gpr_batch(d['x'], d['y'], d['offs'], d['xs'], float(d['mean']), opt=False,
                                 hyp=d['hyp2'])
    fs, sd, lz, _, st = _lib.gpr_predict_multi(d['x'], d['y'], d['offs'], d['xs'], np.arange(ncell + 1),
                                               float(d['mean']), d['hyp2'])
    assert not st.any() and not st1.any()
    for k, v in enumerate((fs, sd, lz)):
        print(k, np.abs(v - out[:, k]).max())
        assert np.all(np.abs(v - out[:, k]) <= RTOL * np.maximum(1.0, np.abs(out[:, k]))), k


def test_device_inputs_equal_host_inputs(edge_batch, edge_result):
    import torch
    b = edge_batch
    x = torch.from_numpy(b.xyt).to('cuda:0')
    z = torch.from_numpy(b.z).to('cuda:0')
    res = _lib.gpr_predict_multi_device(x, z, b.offs, b.xs, b.toffs, b.mean, b.hyp, cov=True, lz=True,
                                        device=0)
    assert _same(res, edge_result)


def test_nystrom_gpr_exact_many_targets():
    d = load_golden('nystrom.npz')
    a, e = d['offs'][2], d['offs'][3]
    x, y, h, mean = d['x'][a:e], d['y'][a:e], np.exp(d['h'][2]), float(d['mean'])
    xs7 = _lattice(np.array([0.0, 0.0, 4.0]), 7)
    fs, sd, sp = nystrom.GPR(x, y, xs7, list(h[:3]), h[3], h[4], mean, returnprior=True)
    rfs, rsd, _, _ = _ref_cell(x, y, xs7, 0.0, h)
    assert fs.shape == (7,) and sd.shape == (7,) and sp == np.sqrt(h[3])
    assert np.all(np.abs(fs - (mean + rfs)) <= RTOL * np.maximum(1.0, np.abs(mean + rfs)))
    assert np.all(np.abs(sd - rsd) <= RTOL * np.maximum(1.0, np.abs(rsd)))
    # one target keeps going through the existing path: the same bits as a
    # direct oi_gpr_batch(opt=0) call on the residual outputs
    f1, s1 = nystrom.GPR(x, y, d['xs'], list(h[:3]), h[3], h[4], mean)
    out, _, _ = _lib.gpr_batch(x, y, [0, len(y)], d['xs'], 0.0, opt=False, hyp=h.reshape(1, 5))
    assert f1.shape == (1,) and f1[0] == mean + out[0, 0] and s1[0] == out[0, 1]
    # and the approximate branch still reproduces the recorded notebook value
    fa, _ = nystrom.GPR(x, y, d['xs'], list(h[:3]), h[3], h[4], mean, approx=True, M=int(d['M'][2]))
    assert abs(fa.item() - d['fs'][2]) <= RTOL * max(1.0, abs(d['fs'][2]))


def test_gpr_cells_multi_fit_then_predict():
    d = load_golden('gpr3d.npz')
    cells = synthetic.RaggedCells(d['x'], d['y'], d['offs'], d['xs'], float(d['mean'])).subset([5, 6, 7])
    xs = np.concatenate([_lattice(cells.xs[c], 9) for c in range(3)])  # centre = the cell's own target
    toffs = np.array([0, 9, 18, 27])
    ref8, rst, _ = gpr.gpr_cells(cells, opt=True, x0=O.X0_PRODUCTION)
    fs, sd, covs, out8, st = gpr.gpr_cells_multi(cells, xs, toffs, opt=True, x0=O.X0_PRODUCTION, cov=True)
    assert np.array_equal(out8, ref8) and not st.any() and not rst.any()
    assert len(covs) == 3 and covs[0].shape == (9, 9)
    own = fs[4::9]  # the lattice's centre point
    assert np.array_equal(xs[4::9], cells.xs)
    assert np.all(np.abs(own - out8[:, 0]) <= RTOL * np.maximum(1.0, np.abs(out8[:, 0])))
