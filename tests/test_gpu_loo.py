"""GPU parity of ``oi_gpr_loo``: leave-one-out cross-validation per cell from
one factorisation (Rasmussen & Williams, GPML 5.4.2).

Reference: tests/loo_ref.py -- ``loo_closed`` (the closed form in numpy) and
``loo_brute`` (n fits of n - 1 observations).  Bounds, the project's T1, fixed
before any GPU run:
  mu    |gpu - ref| <= 1e-10 * max(1, |ref|)
  sd    |gpu - ref| <= 1e-10 * ref           (purely relative: sd is 0.03 .. 0.06 here)
  lpl   |gpu - ref| <= 1e-10 * max(1, |ref|)
For scale, numpy's own spread under re-ordered observations on these inputs
(n = 63 .. 1100, condition numbers <= 1.9e3) is <= 4.9e-15 in mu, <= 3.7e-16
in sd and <= 7.3e-16 in lpl.  Batch mates, chunking, device inputs and
``lpl=False`` must not change a bit of a cell's results.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, gpr, nystrom, synthetic
import loo_ref as R
import workspace_ref as W

pytestmark = pytest.mark.gpu

RTOL = 1e-10
HYP = np.array([2e5, 2e5, 6.0, 5e-3, 1e-3])   # the hypers of scripts/loo_timing.py
EDGE_N = [1, 2, 63, 64, 65, 127, 128, 129, 130, 333, 700, 1100]


def _same(a, b):
    """Bit for bit (NaN equal to NaN)."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def _check(tag, n, got, ref):
    """One cell's (mu, sd, lpl) against a reference's, to the bounds above."""
    (mu, sd, lpl), (rmu, rsd, rlpl) = got, ref
    emu = np.max(np.abs(mu - rmu) / np.maximum(1.0, np.abs(rmu)), initial=0.0)
    esd = np.max(np.abs(sd - rsd) / rsd, initial=0.0)
    elp = abs(lpl - rlpl) / max(1.0, abs(rlpl))
    print(f"{tag}: n {n} |dmu| {emu:.3e} |dsd|/sd {esd:.3e} |dlpl| {elp:.3e}")
    assert np.all(np.abs(mu - rmu) <= RTOL * np.maximum(1.0, np.abs(rmu))), tag
    assert np.all(np.abs(sd - rsd) <= RTOL * rsd), tag
    assert abs(lpl - rlpl) <= RTOL * max(1.0, abs(rlpl)), tag


def _cut(res, offs, c):
    """Cell c's (mu, sd, lpl [1], status [1]) out of a batch result."""
    mu, sd, lpl, st = res
    a, e = offs[c], offs[c + 1]
    return mu[a:e], sd[a:e], lpl[c:c + 1], st[c:c + 1]


@pytest.fixture(scope='module')
def edge():
    """Cells at the 64-tile's edges and with 5, 10 and 17 sweep steps."""
    return synthetic.make_cells(EDGE_N, seed=11)


@pytest.fixture(scope='module')
def edge_hyp():
    return np.tile(HYP, (len(EDGE_N), 1))


@pytest.fixture(scope='module')
def edge_result(edge, edge_hyp):
    return _lib.gpr_loo(edge.xyt, edge.z, edge.offs, edge.mean, edge_hyp)


def test_fixture_cells():
    d = load_golden('gpr3d.npz')
    mean, offs = float(d['mean']), d['offs']
    sizes = np.diff(offs)
    assert sizes.min() == 0 and sizes.max() == 300
    res = _lib.gpr_loo(d['x'], d['y'], offs, mean, d['hyp2'])
    assert not res[3].any()
    for c, n in enumerate(sizes):
        x, z = d['x'][offs[c]:offs[c + 1]], d['y'][offs[c]:offs[c + 1]]
        mu, sd, lpl, _ = _cut(res, offs, c)
        _check(f"cell {c} closed", n, (mu, sd, lpl[0]), R.loo_closed(x, z, mean, d['hyp2'][c]))
        if n <= 200:
            _check(f"cell {c} brute", n, (mu, sd, lpl[0]), R.loo_brute(x, z, mean, d['hyp2'][c]))


def test_tile_edges_ragged_batch(edge, edge_hyp, edge_result):
    assert not edge_result[3].any()
    dup = [n - len(np.unique(edge.cell(c)[0], axis=0)) for c, n in enumerate(EDGE_N)]
    assert dup[-3:] == [11, 56, 135], dup   # repeated sites (rows of K equal): only sn2 I keeps these factorable
    for c, n in enumerate(EDGE_N):
        x, z, _ = edge.cell(c)
        mu, sd, lpl, _ = _cut(edge_result, edge.offs, c)
        _check(f"cell {c}", n, (mu, sd, lpl[0]), R.loo_closed(x, z, edge.mean, HYP))


def test_agrees_with_the_brute_force_batch(edge, edge_result):
    """The parent's only route: n cells of n - 1 observations with one target
    each through oi_gpr_predict_multi."""
    c = EDGE_N.index(65)
    x, z, _ = edge.cell(c)
    n = len(z)
    keep = [np.arange(n) != i for i in range(n)]
    fs, sd, _, _, st = _lib.gpr_predict_multi(np.concatenate([x[k] for k in keep]), np.concatenate([z[k] for k in keep]),
                                              np.arange(n + 1) * (n - 1), x, np.arange(n + 1), edge.mean,
                                              np.tile(HYP, (n, 1)), lz=False)
    assert not st.any()
    mu, s, _, _ = _cut(edge_result, edge.offs, c)
    emu = np.max(np.abs(mu - fs) / np.maximum(1.0, np.abs(fs)))
    evar = np.max(np.abs(s * s - (sd * sd + HYP[4])) / (sd * sd + HYP[4]))
    print(f"|dmu| {emu:.3e} |dvar|/var {evar:.3e}")
    assert np.all(np.abs(mu - fs) <= RTOL * np.maximum(1.0, np.abs(fs)))
    assert np.all(np.abs(s - np.sqrt(sd * sd + HYP[4])) <= RTOL * np.sqrt(sd * sd + HYP[4]))


def test_batch_equals_single(edge, edge_hyp, edge_result):
    for c in range(len(EDGE_N)):
        x, z, _ = edge.cell(c)
        one = _lib.gpr_loo(x, z, [0, len(z)], edge.mean, edge_hyp[c:c + 1])
        assert _same(one, _cut(edge_result, edge.offs, c)), c


def test_chunking_is_bitwise_neutral(edge, edge_hyp, edge_result):
    # the first ten cells (n <= 333), sized by the library's own count
    # (workspace_ref.cell_doubles; tests/test_workspace_layout.py pins the
    # largest): 1.6 MiB (209 715 doubles) cuts after n = 128 and n = 130
    k = 10
    e = edge.offs[k]
    _lib.profile_reset()
    res = _lib.gpr_loo(edge.xyt[:e], edge.z[:e], edge.offs[:k + 1], edge.mean, edge_hyp[:k],
                       pool_bytes=1677721, profile=True)
    chunks = _lib.profile_json()['kernels']['loo_sweep']['launches']
    _lib.profile_reset()
    assert chunks >= 3, chunks
    mu, sd, lpl, st = edge_result
    assert _same(res, (mu[:e], sd[:e], lpl[:k], st[:k]))


def test_device_inputs_equal_host_inputs(edge, edge_hyp, edge_result):
    import torch
    x = torch.from_numpy(edge.xyt).to('cuda:0')
    z = torch.from_numpy(edge.z).to('cuda:0')
    assert _same(_lib.gpr_loo_device(x, z, edge.offs, edge.mean, edge_hyp, device=0), edge_result)


def test_without_lpl_nothing_else_changes(edge, edge_hyp, edge_result):
    mu, sd, lpl, st = _lib.gpr_loo(edge.xyt, edge.z, edge.offs, edge.mean, edge_hyp, lpl=False)
    assert lpl is None
    assert _same((mu, sd, st), (edge_result[0], edge_result[1], edge_result[3]))


def test_failed_cell_is_nan_and_mates_unchanged(edge, edge_hyp, edge_result):
    k = 9   # the n = 333 cell again, non-PD, in front of itself
    x, z, _ = edge.cell(k)
    bad = HYP.copy()
    bad[4] = -2.0 * bad[3]  # first pivot sf2 + sn2 <= 0
    with pytest.raises(np.linalg.LinAlgError):
        R.loo_closed(x, z, edge.mean, bad)
    a = edge.offs[k]
    xyt = np.concatenate([edge.xyt[:a], x, edge.xyt[a:]])
    zz = np.concatenate([edge.z[:a], z, edge.z[a:]])
    offs = np.concatenate([edge.offs[:k + 1], edge.offs[k:] + len(z)])
    hyp = np.concatenate([edge_hyp[:k], bad[None], edge_hyp[k:]])
    mu, sd, lpl, st = _lib.gpr_loo(xyt, zz, offs, edge.mean, hyp)
    e = a + len(z)
    assert st[k] == 1 and st.sum() == 1
    assert np.isnan(mu[a:e]).all() and np.isnan(sd[a:e]).all() and np.isnan(lpl[k])
    keep = [c for c in range(len(hyp)) if c != k]
    mates = (np.concatenate([mu[:a], mu[e:]]), np.concatenate([sd[:a], sd[e:]]), lpl[keep], st[keep])
    assert _same(mates, edge_result)


def test_cell_larger_than_the_pool_is_nomem(edge, edge_hyp):
    with pytest.raises(_lib.OiError, match=r'error -3.*pool_bytes'):
        # the n = 1100 cell alone (workspace_ref.cell_doubles(W.LOO, 1100) doubles) needs ~11.9 MB
        _lib.gpr_loo(edge.xyt, edge.z, edge.offs, edge.mean, edge_hyp, pool_bytes=4 << 20)


def test_pool_that_fits_the_largest_cell_exactly():
    """A pool of exactly the planner's count for the larger cell (plus the
    chunk's slack) holds the call, one cell per chunk; one double less does not."""
    cells = synthetic.make_cells([65, 1], seed=12)
    hyp = np.tile(HYP, (2, 1))
    free = _lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, hyp)
    fit = 8 * (W.SLACK[W.LOO] + W.cell_doubles(W.LOO, 65))
    assert not free[3].any()
    assert _same(_lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, hyp, pool_bytes=fit), free)
    with pytest.raises(_lib.OiError, match=r"error -3: a cell's leave-one-out workspace does not fit pool_bytes"):
        _lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, hyp, pool_bytes=fit - 8)


def test_empty_cell_and_single_observation(edge, edge_hyp, edge_result):
    x, z, _ = edge.cell(0)
    mu, sd, lpl, st = _cut(edge_result, edge.offs, 0)
    assert st[0] == 0 and len(z) == 1
    assert abs(mu[0] - edge.mean) <= RTOL and abs(sd[0] - np.sqrt(HYP[3] + HYP[4])) <= RTOL * sd[0]
    # no observation: no row, lpl = 0, and the cells around it as they are alone
    offs = np.concatenate([edge.offs[:4], edge.offs[3:]])
    hyp = np.concatenate([edge_hyp[:3], HYP[None], edge_hyp[3:]])
    res = _lib.gpr_loo(edge.xyt, edge.z, offs, edge.mean, hyp)
    assert res[2][3] == 0.0 and res[3][3] == 0
    keep = [c for c in range(len(hyp)) if c != 3]
    assert _same((res[0], res[1], res[2][keep], res[3][keep]), edge_result)
    only = _lib.gpr_loo(np.zeros((0, 3)), np.zeros(0), [0, 0], edge.mean, HYP[None])
    assert only[0].shape == (0,) and only[1].shape == (0,) and only[2][0] == 0.0 and only[3][0] == 0


def test_loo_cells_fit_then_cross_validate():
    d = load_golden('gpr3d.npz')
    cells = synthetic.RaggedCells(d['x'], d['y'], d['offs'], d['xs'], float(d['mean'])).subset([5, 6, 7])
    ref8, rst, _ = gpr.gpr_cells(cells, opt=True, x0=O.X0_PRODUCTION)
    mu, sd, lpl, out8, st = gpr.loo_cells(cells, opt=True, x0=O.X0_PRODUCTION)
    assert np.array_equal(out8, ref8) and not st.any() and not rst.any()
    direct = _lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, out8[:, 3:8])
    assert _same((mu, sd, lpl), direct[:3])
    assert np.isfinite(mu).all() and (sd > 0).all()
    # the notebook-style single cell: residual outputs in, the mean added back
    x, z, _ = cells.cell(1)
    h = out8[1, 3:8]
    m1, s1, l1 = nystrom.GPR_loo(x, z - cells.mean, list(h[:3]), h[3], h[4], cells.mean)
    one = _lib.gpr_loo(x, z - cells.mean, [0, len(z)], 0.0, h[None])
    assert _same((m1, s1, l1), (cells.mean + one[0], one[1], one[2][0]))
    _check("GPR_loo", len(z), (m1, s1, l1), R.loo_closed(x, z, cells.mean, h))
    bad = h.copy()
    bad[4] = -2.0 * bad[3]
    with pytest.raises(np.linalg.LinAlgError):
        nystrom.GPR_loo(x, z - cells.mean, list(bad[:3]), bad[3], bad[4], cells.mean)
