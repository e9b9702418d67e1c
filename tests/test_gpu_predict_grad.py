"""GPU parity of ``oi_gpr_predict_grad`` (include/oi_ext.h): the posterior of
u = (f, df/dx, df/dy, df/dt) at many targets per cell.

Reference: tests/grad_ref.py (numpy on ``oracle.gp_oracle.matern32``; pinned
against the oracle by tests/test_grad_ref.py).  Bounds, fixed before any GPU
run, T1's 1e-10 (tests/test_gpu_predict_multi.py) on scaled quantities: with
s = (sqrt(sf2), sqrt(3 sf2) / ell_x, sqrt(3 sf2) / ell_y, sqrt(3 sf2) / ell_t),
  mean components, sd   |gpu - ref| <= 1e-10 max(s_k, |ref|)
  blk / cov entries     |gpu - ref| <= 1e-10 max(s_a s_b, |ref|)
The reference's own spread under re-ordered observations on the gpr3d.npz cells
at hyp2 with the 5 x 5 lattice is <= 4.2e-14 for the mean and <= 3.5e-15 for
the covariance in these units, and the smallest posterior / prior variance
ratio there is 3.1e-3; every input here keeps that ratio >= 1e-4 (checked on
the reference), so that every sd is well conditioned.  Batch mates, chunking,
max_pool and device inputs must not change a bit of a cell's results, and fs /
sd are ``oi_gpr_predict_multi``'s bit for bit.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, gpr, nystrom, synthetic
import grad_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fixture_batch():
    """Every non-empty cell of gpr3d.npz (n = 1 .. 300) at hyp2 with a 5 x 5 lattice of targets."""
    d = load_golden('gpr3d.npz')
    cells = []
    for c in range(len(d['offs']) - 1):
        a, e = d['offs'][c], d['offs'][c + 1]
        if e > a:
            cells.append((d['x'][a:e], d['y'][a:e], G.lattice(d['xs'][c], 25), d['hyp2'][c]))
    return G.Batch(cells, float(d['mean']))


N_EDGE = (0, 1, 2, 63, 64, 65, 129, 200)
NT_EDGE = (0, 1, 15, 16, 17, 32, 33)


def _edge_targets(d, c, x, nt, q):
    """nt targets for cell c: a lattice, with (where there is room) target 1 ON
    an observation and the last target identical to target 0."""
    xs = G.lattice(d['xs'][c], nt)
    if nt >= 3 and len(x) and q % 2 == 0:
        xs[1] = x[len(x) // 2]
    if nt >= 3 and q % 3 != 1:
        xs[-1] = xs[0]
    return xs


@pytest.fixture(scope='module')
def edge_batch():
    """Cells of predict64.npz cut to the tile edges: every n of N_EDGE with
    every nt of NT_EDGE, one ragged call of 56 cells (4 nt + 1 crosses 64 at
    nt = 16 and 128 at nt = 32; 4 nt reaches 64 at nt = 16 and crosses it at 17)."""
    d = load_golden('predict64.npz')
    cells = []
    for q, (n, nt) in enumerate((n, nt) for n in N_EDGE for nt in NT_EDGE):
        c = q % 64
        a = d['offs'][c]
        x = d['x'][a:a + n]
        cells.append((x, d['y'][a:a + n], _edge_targets(d, c, x, nt, q), d['hyp'][c]))
    return G.Batch(cells, float(d['mean']))


@pytest.fixture(scope='module')
def edge_result(edge_batch):
    return edge_batch.run()


def test_parity_on_golden_cells(fixture_batch):
    b = fixture_batch
    ratio = G.well_conditioned(b)
    print("smallest posterior / prior variance ratio", ratio)
    assert ratio >= G.MIN_RATIO
    G.check_against_ref(b, b.run())


def test_tile_edges_ragged_batch(edge_batch, edge_result):
    b = edge_batch
    assert sorted(set(zip(np.diff(b.offs), np.diff(b.toffs)))) == sorted((n, nt) for n in N_EDGE for nt in NT_EDGE)
    on_obs = dup = 0
    for x, _, xs, _ in b.cells:
        on_obs += sum((x == t).all(axis=1).any() for t in xs) if len(x) else 0
        dup += len(xs) - len(np.unique(xs, axis=0))
    assert on_obs > 0 and dup > 0
    ratio = G.well_conditioned(b)
    print("smallest posterior / prior variance ratio", ratio)
    assert ratio >= G.MIN_RATIO
    G.check_against_ref(b, edge_result)


def test_empty_cell_is_the_prior(edge_batch, edge_result):
    b = edge_batch
    grad, gsd, fs, sd, blk, cov, st = edge_result
    covs = _lib.split_jcov(cov, b.toffs)
    seen = 0
    for c in np.flatnonzero(np.diff(b.offs) == 0):
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        if t1 == t0:
            continue
        seen += 1
        s = G.scales(b.hyp[c])
        assert (grad[t0:t1] == 0).all() and (fs[t0:t1] == b.mean).all()
        assert np.all(np.abs(sd[t0:t1] - s[0]) <= 4e-16 * s[0])
        assert np.all(np.abs(gsd[t0:t1] - s[1:]) <= 4e-16 * s[1:])
        P = b.ref()[c][1]
        assert np.all(np.abs(covs[c] - P) <= G.RTOL * np.maximum(np.outer(np.tile(s, t1 - t0), np.tile(s, t1 - t0)),
                                                                 np.abs(P)))
        for t in range(t1 - t0):
            assert np.array_equal(blk[t0 + t], np.diag(blk[t0 + t].diagonal()))   # P_t is diagonal
            assert np.array_equal(blk[t0 + t], covs[c][4 * t:4 * t + 4, 4 * t:4 * t + 4])
    assert seen == len(NT_EDGE) - 1


def test_fs_sd_bitwise_equal_predict_multi(edge_batch, edge_result):
    b = edge_batch
    fs, sd, _, _, st = _lib.gpr_predict_multi(b.xyt, b.z, b.offs, b.xs, b.toffs, b.mean, b.hyp, cov=False, lz=False)
    assert not st.any() and not edge_result[6].any()
    assert np.array_equal(edge_result[2], fs) and np.array_equal(edge_result[3], sd)


def test_structure(edge_batch, edge_result, fixture_batch):
    for b, res in ((edge_batch, edge_result), (fixture_batch, fixture_batch.run())):
        grad, gsd, fs, sd, blk, cov, st = res
        d = np.stack([blk[:, k, k] for k in range(4)], axis=1) if len(blk) else np.zeros((0, 4))
        assert np.array_equal(gsd, np.sqrt(d[:, 1:])) and np.array_equal(sd, np.sqrt(d[:, 0]))
        assert np.array_equal(blk, blk.transpose(0, 2, 1))
        for c, C in enumerate(_lib.split_jcov(cov, b.toffs)):
            assert C.shape == (4 * (b.toffs[c + 1] - b.toffs[c]),) * 2
            assert np.array_equal(C, C.T), c
        # blk and the diagonal blocks of cov within the bound of the reference: check_against_ref
        G.check_against_ref(b, res)
        bare = b.run(blk=False, cov=False)
        assert bare[4] is None and bare[5] is None
        assert G.same(bare[:4] + bare[6:], res[:4] + res[6:])


def test_batch_equals_single(edge_batch, edge_result):
    for c in range(len(edge_batch.cells)):
        one = edge_batch.subset([c]).run()
        assert G.same((one[0], one[1], one[2], one[3], one[4], one[5], one[6]),
                      G.cell_slices(edge_batch, edge_result, c)), c


def test_chunking_is_bitwise_neutral(edge_batch, edge_result):
    _lib.profile_reset()
    res = edge_batch.run(pool_bytes=2 * 1024 * 1024, profile=True)
    prof = _lib.profile_json()['kernels']
    _lib.profile_reset()
    assert {'pg_generate', 'pg_cholesky', 'pg_solve', 'pg_reduce', 'pg_cov'} <= set(prof)
    assert prof['pg_reduce']['launches'] >= 3, prof['pg_reduce']
    assert G.same(res, edge_result)


def test_max_pool_one_is_bitwise_neutral(edge_batch, edge_result):
    assert G.same(edge_batch.run(max_pool=1), edge_result)


def test_cell_larger_than_the_pool_is_nomem(edge_batch):
    with pytest.raises(_lib.OiError, match=r"error -3: a cell's gradient workspace does not fit pool_bytes"):
        edge_batch.run(pool_bytes=256 * 1024)


def test_device_inputs_equal_host_inputs(edge_batch, edge_result):
    import torch
    b = edge_batch
    x = torch.from_numpy(b.xyt).to('cuda:0')
    z = torch.from_numpy(b.z).to('cuda:0')
    res = _lib.gpr_predict_grad_device(x, z, b.offs, b.xs, b.toffs, b.mean, b.hyp, blk=True, cov=True, device=0)
    assert G.same(res, edge_result)


def test_failed_cell_is_nan_and_mates_unchanged(edge_batch, edge_result):
    d = load_golden('predict64.npz')
    a = d['offs'][20]
    hyp = d['hyp'][20].copy()
    hyp[4] = -2.0 * hyp[3]  # first pivot sf2 + sn2 <= 0
    bad = (d['x'][a:a + 100], d['y'][a:a + 100], G.lattice(d['xs'][20], 18), hyp)
    with pytest.raises(np.linalg.LinAlgError):
        G.ref_cell(bad[0], bad[1], bad[2], edge_batch.mean, hyp)
    k = 30
    cells = edge_batch.cells[:k] + [bad] + edge_batch.cells[k:]
    b = G.Batch(cells, edge_batch.mean)
    res = b.run()
    st = res[6]
    assert st[k] == 1 and st.sum() == 1
    mine = G.cell_slices(b, res, k)
    assert mine[5].shape == (72 * 72,)
    for v in mine[:6]:
        assert np.isnan(v).all()
    keep = [c for c in range(len(cells)) if c != k]
    for q, c in enumerate(keep):
        assert G.same(G.cell_slices(b, res, c), G.cell_slices(edge_batch, edge_result, q)), c


def test_gradient_against_differences_of_predict_multi(edge_batch, edge_result):
    """End to end without the reference: central differences of
    oi_gpr_predict_multi's fs at targets shifted by +-h_k, h_k = 1e-4 ell_k /
    sqrt(3); bound 1e-6 s_k (the defect is O(h^2) = 1e-8, the cancellation about
    eps |fs| / (1e-4 sqrt(sf2)) = 5e-12)."""
    b = edge_batch
    grad = edge_result[0]
    nt = np.diff(b.toffs)
    for k in range(3):
        h = 1e-4 * np.repeat(b.hyp[:, k], nt) / O.SQRT3
        e = np.zeros((len(h), 3))
        e[:, k] = h
        xs2 = np.concatenate([b.xs + e, b.xs - e])
        # every cell's targets doubled: cell c owns rows of both halves, so build it cell by cell
        rows = np.concatenate([np.concatenate([np.arange(b.toffs[c], b.toffs[c + 1]),
                                               len(h) + np.arange(b.toffs[c], b.toffs[c + 1])])
                               for c in range(len(nt))]).astype(np.int64)
        fs, _, _, _, st = _lib.gpr_predict_multi(b.xyt, b.z, b.offs, xs2[rows], 2 * b.toffs, b.mean, b.hyp,
                                                 cov=False, lz=False)
        assert not st.any()
        back = np.empty(len(rows))
        back[rows] = fs
        fd = (back[:len(h)] - back[len(h):]) / (2 * h)
        s = np.repeat(np.sqrt(3 * b.hyp[:, 3]) / b.hyp[:, k], nt)
        err = np.abs(grad[:, k] - fd) / s
        print(f"component {k}: worst |grad - central difference| / s_k {err.max():.3e}")
        assert np.all(err <= 1e-6), k


def test_grad_cells_fit_then_gradient():
    d = load_golden('gpr3d.npz')
    cells = synthetic.RaggedCells(d['x'], d['y'], d['offs'], d['xs'], float(d['mean'])).subset([5, 6, 7])
    xs = np.concatenate([G.lattice(cells.xs[c], 9) for c in range(3)])
    toffs = np.array([0, 9, 18, 27])
    ref8, rst, _ = gpr.gpr_cells(cells, opt=True, x0=O.X0_PRODUCTION)
    grad, gsd, fs, sd, blk, covs, out8, st = gpr.grad_cells(cells, xs, toffs, opt=True, x0=O.X0_PRODUCTION, blk=True,
                                                            cov=True)
    assert np.array_equal(out8, ref8) and not st.any() and not rst.any()
    direct = _lib.gpr_predict_grad(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, out8[:, 3:8], blk=True,
                                   cov=True)
    assert G.same((grad, gsd, fs, sd, blk, np.concatenate([c.ravel() for c in covs])), direct[:6])
    assert len(covs) == 3 and covs[0].shape == (36, 36) and grad.shape == (27, 3) and blk.shape == (27, 4, 4)
    bare = gpr.grad_cells(cells, xs, toffs, opt=False, hyp=out8[:, 3:8])
    assert bare[4] is None and bare[5] is None and G.same(bare[:4], direct[:4])


def test_nystrom_gpr_grad_equals_the_one_cell_call():
    d = load_golden('nystrom.npz')
    a, e = d['offs'][2], d['offs'][3]
    x, y, h, mean = d['x'][a:e], d['y'][a:e], np.exp(d['h'][2]), float(d['mean'])
    xs7 = G.lattice(np.array([0.0, 0.0, 4.0]), 7)
    grad, gsd, fs, sd, blk = nystrom.GPR_grad(x, y, xs7, list(h[:3]), h[3], h[4], mean)
    one = _lib.gpr_predict_grad(x, y, [0, len(y)], xs7, [0, 7], 0.0, h.reshape(1, 5), blk=True)
    assert not one[6].any()
    assert G.same((grad, gsd, fs, sd, blk), (one[0], one[1], mean + one[2], one[3], one[4]))
    f1, s1 = nystrom.GPR(x, y, xs7, list(h[:3]), h[3], h[4], mean)
    assert np.array_equal(fs, f1) and np.array_equal(sd, s1)
    with pytest.raises(np.linalg.LinAlgError):
        nystrom.GPR_grad(x, y, xs7, list(h[:3]), h[3], -2.0 * h[3], mean)
