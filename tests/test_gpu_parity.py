"""GPU parity of the HIP path (through the C ABI) against the oracle and the
reference-generated golden fixtures.

Tolerances (tier T1 -- fixed hyper-parameters):
  nlZ, fs, sd, lZ     |gpu - ref| <= 1e-10 * max(1, |ref|)
  gradient            |gpu - ref| <= 1e-10 * (|ref| + S_j),  S_j = 1/2 sum|Q o dK_j|
                      (the magnitude of the terms the reference sums)
Optimised fits (tier T3) are checked in tests/test_gpu_fit.py.
"""
import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform

from conftest import load_golden, ragged_cell
from dense_ref import exact_cell, exact_cells, site_counts
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def grad_scale(h, x, y, mX):
    """S_j = 1/2 sum |Q o dK_j| (and sn2*sum|diag Q| for j=4) at h (oracle-side)."""
    n = len(y)
    if n == 0:
        return np.zeros(6)
    ell = np.exp(h[:3])
    sf2, sn2 = np.exp(h[3]), np.exp(h[4])
    K, dK = O.matern32(x, ell, sf2, grad=True)
    Kinv = np.linalg.inv(K + np.eye(n) * sn2)
    a = Kinv @ (y - mX)
    Q = Kinv - np.outer(a, a)
    s = np.zeros(6)
    for j in range(3):
        s[j] = np.abs(Q * dK[j]).sum() / 2
    s[3] = np.abs(Q * 2 * K).sum() / 2
    s[4] = sn2 * np.abs(np.diag(Q)).sum()
    return s


def close(a, b, scale=None, rtol=RTOL):
    a = np.asarray(a, float)
    b = np.asarray(b, float)
    if scale is None:
        scale = np.maximum(1.0, np.abs(b))
    both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    both_nan = np.isnan(a) & np.isnan(b)
    ok = both_inf | both_nan | (np.abs(a - b) <= rtol * scale)
    return bool(np.all(ok)), np.max(np.where(both_inf | both_nan, 0, np.abs(a - b) / scale))


def test_smlii_golden():
    d = load_golden('smlii.npz')
    nc = len(d['nlZ'])
    mX = np.full(len(d['y']), float(d['mean']))
    nlz, grad, status = _lib.nlml_grad_batch(d['x'], d['y'], mX, d['offs'], d['h'])
    for k in range(nc):
        ok, err = close(nlz[k], d['nlZ'][k])
        assert ok, (k, nlz[k], d['nlZ'][k], err)
        x, y = ragged_cell(d, k)
        if np.isfinite(d['nlZ'][k]):
            sc = np.abs(d['g'][k]) + grad_scale(d['h'][k], x, y, np.ones(len(y)) * float(d['mean']))
            ok, err = close(grad[k], d['g'][k], scale=np.maximum(sc, 1e-300))
            assert ok, (k, grad[k], d['g'][k], err)


@pytest.mark.parametrize('n', [63, 64, 65, 130, 333, 700, 1100])
def test_smlii_vs_oracle_sizes(n):
    """Tile-boundary sizes and multi-tile cells, 3 hyper points each.  n is the
    number of distinct SITES, which is what the kernels tile (two cells
    without repeats, one with n sites under n + max(3, n / 10) observations:
    the site form's (n - m) and SSW terms on the same edge)."""
    rng = np.random.default_rng(n)
    cells = exact_cells([n, n, (n, n + max(3, n // 10))], seed=n)
    assert [q[1] for q in site_counts(cells)] == [n] * 3
    hs = np.array([O.X0_PRODUCTION,
                   [np.log(3e5), np.log(2e5), np.log(8.), np.log(4e-3), np.log(5e-4), 0.0],
                   [np.log(9e4), np.log(1.5e5), np.log(3.), np.log(1e-2), np.log(2e-3), -2.0]])
    mX = np.full(len(cells.z), cells.mean)
    nlz, grad, status = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, hs)
    for c in range(3):
        x, y, _ = cells.cell(c)
        mx = np.ones(len(y)) * cells.mean
        f, g = O.neg_log_ml(hs[c], x, y, mx)
        f = float(np.asarray(f).item())
        ok, err = close(nlz[c], f)
        assert ok, (n, c, nlz[c], f, err)
        sc = np.abs(g) + grad_scale(hs[c], x, y, mx)
        ok, err = close(grad[c], g, scale=np.maximum(sc, 1e-300))
        assert ok, (n, c, grad[c], g, err)
    del rng


def test_not_pd_reports_inf():
    """Exactly duplicated sites with sn2 = 0 give a zero pivot: the reference's
    LinAlgError branch (GPR:139-140) -> (inf, inf*ones)."""
    x = np.array([[1e5, 2e5, 3.0], [1e5, 2e5, 3.0]])
    y = np.array([0.3, 0.31])
    h = np.array([[np.log(25000), np.log(25000), 0.0, 0.0, -np.inf, 0.0]])
    f_ref, g_ref = O.neg_log_ml(h[0], x, y, np.ones(2) * 0.28)
    assert np.isinf(f_ref)
    nlz, grad, status = _lib.nlml_grad_batch(x, y, np.ones(2) * 0.28, np.array([0, 2]), h)
    assert np.isinf(nlz[0]) and np.all(np.isinf(grad[0])) and status[0] == 1


def test_predict_golden_gpr3d_pass2():
    d = load_golden('gpr3d.npz')
    out, status, _ = _lib.gpr_batch(d['x'], d['y'], d['offs'], d['xs'], float(d['mean']),
                                    opt=False, hyp=d['hyp2'])
    for c in range(len(d['offs']) - 1):
        ok, err = close(out[c, :2], d['out2'][c])
        assert ok, (c, out[c, :2], d['out2'][c], err)


def test_predict_golden_64cells():
    d = load_golden('predict64.npz')
    out, status, _ = _lib.gpr_batch(d['x'], d['y'], d['offs'], d['xs'], float(d['mean']),
                                    opt=False, hyp=d['hyp'])
    ok, err = close(out[:, :2], d['out2'])
    assert ok, err
    assert np.all(status == 0)


def test_predict_lZ_vs_oracle():
    cells = synthetic.make_cells([0, 1, 5, 64, 200, 513], seed=5)
    hyp = np.tile(synthetic.FIXED_HYPERS, (cells.ncell, 1))
    out, status, _ = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean,
                                    opt=False, hyp=hyp)
    for c in range(cells.ncell):
        x, y, xs = cells.cell(c)
        fs, sd, lZ = O.predict(x, y, xs, cells.mean, hyp[c, :3], hyp[c, 3], hyp[c, 4])
        ok, err = close(out[c, :3], [fs[0], sd[0], lZ])
        assert ok, (c, out[c, :3], (fs[0], sd[0], lZ), err)
    # n = 0: (mean, sqrt(sf2), -0.0) exactly like GPR:178-182 on empty arrays
    assert out[0, 0] == cells.mean and out[0, 1] == np.sqrt(hyp[0, 3])
    assert out[0, 2] == 0.0 and np.signbit(out[0, 2])


def test_batch_composition_independence():
    """A cell's results are bitwise identical alone or inside any batch."""
    cells = synthetic.make_cells([150, 700, 40, 300], seed=9)
    hs = np.tile(np.array([np.log(2e5), np.log(2e5), np.log(5.), np.log(5e-3), np.log(1e-3), 0.]),
                 (4, 1))
    mX = np.full(len(cells.z), cells.mean)
    nlz, grad, _ = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, hs)
    for c in range(4):
        sub = cells.subset([c])
        n1, g1, _ = _lib.nlml_grad_batch(sub.xyt, sub.z, np.full(len(sub.z), cells.mean), sub.offs,
                                         hs[c:c + 1])
        assert n1[0] == nlz[c] and np.array_equal(g1[0], grad[c])


def test_gpr3d_n0_edge():
    """GPR3D on an empty neighbourhood: CG stops at x0 and the
    cell returns (mean, 1.0, -0.0, 25000, 25000, 1, 1, 1)."""
    cells = synthetic.make_cells([0], seed=1)
    out, status, info = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean,
                                       x0=np.array(O.X0_PRODUCTION), opt=True, info=True)
    ref = O.gp_cell(np.zeros((0, 3)), np.zeros(0), cells.xs[0], cells.mean, opt=True)
    assert np.array_equal(out[0], np.array(ref, float))
    assert np.signbit(out[0, 2])
    assert info[0, 1] == 0 and info[0, 3] == 1


def _check_tile_boundary_sizes():
    """SMLII and the predict block meet the T1 tolerance on tile-boundary sizes:
    site counts m = 63 .. 700 (T = 1, 1, 2, 3, 4, 5, 11 block rows, the last
    with 63, 64, 1, 1, 8, 1, 60 rows) and one cell of 129 sites under 150
    observations (the deduplicated path)."""
    sizes = [63, 64, 65, 129, 200, 257, 700, (129, 150)]
    cells = exact_cells(sizes, seed=11)
    assert [q[1] for q in site_counts(cells)] == [63, 64, 65, 129, 200, 257, 700, 129]
    h = np.tile(np.array([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(1e-3), 0.]),
                (len(sizes), 1))
    mX = np.full(len(cells.z), cells.mean)
    nlz, grad, st = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, h)
    for c in range(len(sizes)):
        x, y, _ = cells.cell(c)
        f, g = O.neg_log_ml(h[c], x, y, np.full(len(y), cells.mean))
        f = float(np.asarray(f).item())
        assert abs(nlz[c] - f) <= RTOL * max(1.0, abs(f)), sizes[c]
        S = grad_scale(h[c], x, y, np.full(len(y), cells.mean))
        assert np.all(np.abs(grad[c] - g) <= RTOL * (np.abs(g) + S)), sizes[c]
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    out, st2, _ = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
    for c in range(len(sizes)):
        x, y, xs = cells.cell(c)
        fs, sd, lZ = O.predict(x, y, xs, cells.mean, hyp[c, :3], hyp[c, 3], hyp[c, 4])
        assert abs(out[c, 0] - fs[0]) <= RTOL * max(1, abs(fs[0]))
        assert abs(out[c, 1] - sd[0]) <= RTOL * max(1, abs(sd[0]))


def test_panels_tile_boundary_sizes():
    """The Cholesky panels as the engine picks them by default (paired columns
    sharing one stream: an even-column kernel, then k_chol_panel for the odd
    column) on sizes around the 64-tile."""
    _check_tile_boundary_sizes()


@pytest.mark.parametrize('knob,value', [('OI_PANEL4', '0'), ('OI_PANEL4_MINT', '0')])
def test_alternate_kernels_agree(knob, value, monkeypatch):
    """The even-column panel core the engine selects per round -- k_panel_even
    everywhere (OI_PANEL4=0) or k_panel4 in every round (OI_PANEL4_MINT=0 with
    OI_PANEL4_MINWG=0; by default only in rounds whose largest cell has >= 12
    block columns and in launches of >= 512 workgroups, which these few cells
    of at most 11 block rows never reach) --
    meets the T1 tolerance on tile-boundary sizes, fit and predict.  (Round 4
    retired the other A/B alternates -- round 1's 32-blocked and round 2's
    single-wave diagonal factors, the P-form panels with k_scale, the 128x128
    K^-1 kernel and the folded pair step)"""
    monkeypatch.setenv(knob, value)
    if knob == 'OI_PANEL4_MINT':
        monkeypatch.setenv('OI_PANEL4_MINWG', '0')
    _check_tile_boundary_sizes()


def test_config5_size_n5000():
    """BASELINE config 5 allows n up to 5000 per cell: SMLII and the predict
    block at 5000 distinct sites (T = 79 block rows, the last with 8; off the
    25 km lattice, which holds only ~4070 sites per cell), T1 tolerance, one
    cell each."""
    n = 5000
    cells = exact_cell(n, n, seed=5000, lattice=False)
    assert site_counts(cells) == [(5000, 5000, 79, 8)]
    h = np.array([[np.log(2.2e5), np.log(1.8e5), np.log(6.), np.log(5e-3), np.log(1e-3), 0.0]])
    mX = np.full(n, cells.mean)
    nlz, grad, status = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, h)
    x, y, xs = cells.cell(0)
    f, g = O.neg_log_ml(h[0], x, y, mX)
    f = float(np.asarray(f).item())
    assert status[0] == 0
    ok, err = close(nlz[0], f)
    assert ok, (nlz[0], f, err)
    sc = np.abs(g) + grad_scale(h[0], x, y, mX)
    ok, err = close(grad[0], g, scale=np.maximum(sc, 1e-300))
    assert ok, (grad[0], g, err)
    hyp = np.exp(h[:, :5])
    out, st, _ = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
    fs, sd, lZ = O.predict(x, y, xs, cells.mean, hyp[0, :3], hyp[0, 3], hyp[0, 4])
    for got, ref in ((out[0, 0], fs[0]), (out[0, 1], sd[0])):
        ok, err = close(got, ref)
        assert ok, (got, ref, err)


def test_duplicate_sites_reduction():
    """The site form (oi_device.h "Duplicate sites"): observations with equal
    (x, y, t) are folded into one site of weight sqrt(count) and the (n - m),
    SSW terms added back -- exact algebra, so nlZ / gradient / predict agree
    with the oracle's n x n computation (GPR:107-141, 173-182) at T1, with
    deduplication on (default) and off (OI_DEDUP=0), including a cell beyond
    k_dedup's LDS staging size (4500 observations on 2820 sites: T = 45 block
    rows deduplicated, 71 with OI_DEDUP=0) and one made only of copies of a
    single site."""
    import os
    rng = np.random.default_rng(8)
    sizes = [3, 200, 700, 4500]
    cells = synthetic.make_cells(sizes, seed=31)
    xyt, z = cells.xyt.copy(), cells.z.copy()
    a = int(cells.offs[0])
    xyt[a + 1] = xyt[a]
    xyt[a + 2] = xyt[a]                      # cell 0: three copies of one site
    b = int(cells.offs[1])
    xyt[b:b + 50] = xyt[b + 50:b + 100]      # cell 1: 50 extra duplicates
    h = np.tile([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(8e-4), 0.0], (4, 1))
    mX = np.full(len(z), cells.mean)
    res = {}
    for mode in ('1', '0'):
        os.environ['OI_DEDUP'] = mode
        try:
            res[mode] = _lib.nlml_grad_batch(xyt, z, mX, cells.offs, h)
            hyp = np.tile(np.exp(h[0, :5]), (4, 1))
            res[mode + 'p'] = _lib.gpr_batch(xyt, z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
        finally:
            os.environ.pop('OI_DEDUP', None)
    for c in range(4):
        lo, hi = int(cells.offs[c]), int(cells.offs[c + 1])
        x, y = xyt[lo:hi], z[lo:hi]
        f, g = O.neg_log_ml(h[c], x, y, np.ones(len(y)) * cells.mean)
        f = float(np.asarray(f).item())
        S = grad_scale(h[c], x, y, np.ones(len(y)) * cells.mean) if len(y) <= 1000 else np.abs(g) + 1e-6 * np.abs(f)
        fs, sd, lZ = O.predict(x, y, cells.xs[c:c + 1], cells.mean, np.exp(h[c, :3]), np.exp(h[c, 3]),
                               np.exp(h[c, 4]))
        for mode in ('1', '0'):
            nlz, grad, st = res[mode]
            out = res[mode + 'p'][0]
            assert st[c] == 0
            assert close(nlz[c], f)[0], (mode, c, nlz[c], f)
            assert np.all(np.abs(grad[c, :5] - g[:5]) <= RTOL * (np.abs(g[:5]) + S[:5])), (mode, c, grad[c], g)
            assert close(out[c, 0], fs[0])[0] and close(out[c, 1], sd[0])[0] and close(out[c, 2], lZ)[0], \
                (mode, c, out[c, :3], fs, sd, lZ)


def test_duplicate_nonpd_band():
    """Duplicate sites at tiny sn2 / sf2 (oi_device.h OI_DUP_NONPD_TAU): the
    reference's n x n Cholesky (GPR:126) fails on a repeated row's pivot below
    a band ~max(1e-18 n_obs, 1e-16) that its own rounding decides (permuting the
    observations moves it); outside [tau / 5, 5 tau] the GPU's status and the
    oracle's inf / finite SMLII (GPR:139-140) must agree exactly, inside it
    either outcome is the reference's own noise.  Cells of the synthetic
    generator (natural lattice duplicates) and two-copy cells, n = 50 .. 1000."""
    rng = np.random.default_rng(17)
    sf2 = 4e-3
    ratios = [1e-17, 1e-16, 3e-16, 1e-15, 3e-15, 1e-14, 1e-13, 1e-12]
    cases = []
    for n in (50, 500, 1000):
        nat = synthetic.make_cells([n], seed=900 + n)
        x, z, _ = nat.cell(0)
        cases.append((x, z))
        idx = rng.permutation(np.repeat(np.arange(n // 2), 2))
        cases.append((x[:n // 2][idx], z[:n // 2][idx] + rng.normal(0, 0.01, len(idx))))
    xs, zs, offs, hs, meta = [], [], [0], [], []
    for x, z in cases:
        for r in ratios:
            xs.append(x)
            zs.append(z)
            offs.append(offs[-1] + len(z))
            hs.append([np.log(3e5), np.log(2.5e5), np.log(8.), np.log(sf2), np.log(sf2 * r), 0.0])
            meta.append((len(z), r))
    xyt, zz, offs, h = np.concatenate(xs), np.concatenate(zs), np.array(offs), np.array(hs)
    nlz, grad, st = _lib.nlml_grad_batch(xyt, zz, np.full(len(zz), 0.28), offs, h)
    disagree_outside, inband = [], []
    for c, (n, r) in enumerate(meta):
        x, y = xyt[offs[c]:offs[c + 1]], zz[offs[c]:offs[c + 1]]
        f, _ = O.neg_log_ml(h[c], x, y, np.ones(n) * 0.28)
        ref_fail = not np.isfinite(np.ravel(f)[0])
        gpu_fail = st[c] == 1
        assert gpu_fail == (not np.isfinite(nlz[c]))
        tau = max(1e-18 * n, 1e-16)   # small n: the sf2 + sn2 == sf2 rounding rule
        if gpu_fail != ref_fail:
            (inband if tau / 5 <= r <= 5 * tau else disagree_outside).append((n, r, ref_fail, gpu_fail))
    assert not disagree_outside, (disagree_outside, inband)


def test_panel4_equals_panel_even(monkeypatch):
    """k_panel4 (two block rows per workgroup on the 128 x 128 core) does the
    even-column panel's arithmetic in the same order as k_panel_even (same
    MFMA chunk sequence, S = A - acc, the same triangular product, and since
    round 5 the same look-ahead, (A - acc) - L L^T): objective, gradient and
    predictions are BITWISE equal, so the engine's per-round choice between
    them never changes a result; poisoned workspaces (OI_POISON=1) included --
    nothing is read before it is written."""
    sizes = [1, 40, 63, 64, 65, 128, 129, 191, 192, 193, 257, 700, 1100, 2000, (193, 230)]   # site counts
    cells = exact_cells(sizes, seed=23)
    assert [q[1] for q in site_counts(cells)] == [s if np.ndim(s) == 0 else s[0] for s in sizes]
    h = np.tile(np.array([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(1e-3), 0.]), (len(sizes), 1))
    mX = np.full(len(cells.z), cells.mean)
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    res = {}
    monkeypatch.setenv('OI_PANEL4_MINT', '0')   # k_panel4 in every round (default: rounds with T >= 12
    monkeypatch.setenv('OI_PANEL4_MINWG', '0')  # and >= 512 workgroups)
    for p4 in ('0', '1'):
        for poison in ('0', '1'):
            monkeypatch.setenv('OI_PANEL4', p4)
            monkeypatch.setenv('OI_POISON', poison)
            ev = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, h)
            pr = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
            res[(p4, poison)] = (ev[0], ev[1], pr[0][:, :3])
    for p4 in ('0', '1'):
        for a, b in zip(res[(p4, '1')], res[(p4, '0')]):
            assert np.array_equal(a, b), p4
    for a, b in zip(res[('1', '0')], res[('0', '0')]):
        assert np.array_equal(a, b), np.max(np.abs(a - b) / np.maximum(1, np.abs(b)))


def test_fused_diag_factor_equals_separate_launches(monkeypatch):
    """The look-ahead workgroup of column j's panel launch factors diagonal
    tile j+1 (default, OI_FUSE_DIAG_MIN=1); with OI_FUSE_DIAG_MIN above the
    round size every column's diagonal tile is factored by its own
    k_diag_factor4w launch instead.  Same arithmetic on the same
    LDS layout: objective, gradient, predictions and a full fit bitwise equal,
    for both even-column kernels."""
    sizes = [1, 63, 64, 65, 129, 192, 257, 700, 1100, 2000, (257, 300)]   # site counts
    cells = exact_cells(sizes, seed=29)
    assert [q[1] for q in site_counts(cells)] == [s if np.ndim(s) == 0 else s[0] for s in sizes]
    h = np.tile(np.array([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(1e-3), 0.]), (len(sizes), 1))
    mX = np.full(len(cells.z), cells.mean)
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    fit = synthetic.make_cells([300, 700], seed=31)
    monkeypatch.setenv('OI_PANEL4_MINT', '0')
    monkeypatch.setenv('OI_PANEL4_MINWG', '0')
    res = {}
    for p4 in ('0', '1'):
        for fuse in ('1', '100000'):
            monkeypatch.setenv('OI_PANEL4', p4)
            monkeypatch.setenv('OI_FUSE_DIAG_MIN', fuse)
            ev = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, h)
            pr = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
            ft = _lib.gpr_batch(fit.xyt, fit.z, fit.offs, fit.xs, fit.mean, opt=True, info=True,
                                x0=np.array([np.log(25e3), np.log(25e3), 0., 0., 0., np.log(.1)]))
            res[(p4, fuse)] = (ev[0], ev[1], pr[0][:, :3], ft[0], ft[2][:, 3])
    for p4 in ('0', '1'):
        for a, b in zip(res[(p4, '1')], res[(p4, '100000')]):
            assert np.array_equal(a, b, equal_nan=True), (p4, a, b)


def test_cell_result_independent_of_round_mates(monkeypatch):
    """A cell's results never depend on the other cells of its rounds: small
    cells (T < 12, k_panel_even when alone) fitted and evaluated alone, and
    together with large cells (rounds of T >= 12 where the engine may pick
    k_panel4), are bitwise equal -- objective, gradient, a full opt=True fit
    and predictions."""
    monkeypatch.setenv('OI_PANEL4_MINWG', '0')  # the mixed rounds do take k_panel4
    small = synthetic.make_cells([90, 333, 700], seed=51)
    big = synthetic.make_cells([1500, 2200], seed=52)
    both = synthetic.RaggedCells(np.concatenate([small.xyt, big.xyt]), np.concatenate([small.z, big.z]),
                                 np.concatenate([small.offs, small.offs[-1] + big.offs[1:]]),
                                 np.concatenate([small.xs, big.xs]), small.mean)
    h = np.tile(np.array([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(1e-3), 0.]), (5, 1))
    n1, g1, _ = _lib.nlml_grad_batch(small.xyt, small.z, np.full(len(small.z), small.mean), small.offs, h[:3])
    n2, g2, _ = _lib.nlml_grad_batch(both.xyt, both.z, np.full(len(both.z), both.mean), both.offs, h)
    assert np.array_equal(n1, n2[:3]) and np.array_equal(g1, g2[:3])
    x0 = np.array(O.X0_PRODUCTION)
    o1, s1, i1 = _lib.gpr_batch(small.xyt, small.z, small.offs, small.xs, small.mean, x0=x0, opt=True, info=True)
    o2, s2, i2 = _lib.gpr_batch(both.xyt, both.z, both.offs, both.xs, both.mean, x0=x0, opt=True, info=True)
    assert np.array_equal(o1, o2[:3], equal_nan=True) and np.array_equal(i1, i2[:3])


def test_profile_by_j_matches_kernel_totals():
    """The per-(kernel, block column) launch table of the profile (bench.py
    --dump) accounts for every profiled launch: per kernel its
    launches, HIP-event milliseconds and executed flops sum to the kernel
    totals, and the factor-panel rows cover the block columns the cells have."""
    sizes = [300, 700, 1300]
    cells = synthetic.make_cells(sizes, seed=41)
    h = np.tile(np.array([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(1e-3), 0.]), (len(sizes), 1))
    mX = np.full(len(cells.z), cells.mean)
    _lib.profile_reset()
    _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, h, profile=True)
    pj = _lib.profile_json()
    byj = pj['by_j']
    assert byj
    for k, v in pj['kernels'].items():
        rows = [r for r in byj if r[0] == k]
        if not v['launches']:
            assert not rows
            continue
        assert sum(r[2] for r in rows) == v['launches'], k
        assert abs(sum(r[4] for r in rows) - v['total_ms']) <= 1e-3 * max(1.0, v['total_ms']), k
        if v['flops'] > 0 and k != 'k_lauum_grad':
            assert abs(sum(r[5] for r in rows) - v['flops']) <= 1e-6 * v['flops'], k  # printed to 7 digits
    # k_diag_factor4w runs for block column 0 only: the look-ahead workgroup of
    # column j's panel launch factors diagonal tile j+1 (round 5)
    js = sorted(r[1] for r in byj if r[0] == 'k_diag_factor')
    assert js == [0]
    jp = sorted({r[1] for r in byj if r[0] in ('k_panel4', 'k_panel_even', 'k_chol_panel')})
    assert jp == list(range(len(jp))) and len(jp) >= 2



# Hyper-parameter points the chaotic CG does reach (line searches
# overshoot into overflow -- cell 37 of the day fixture made 111 inf
# evaluations, DESIGN §2b history): length-scales and variances far outside
# the data's range, exp() over- and underflowing (GPR:120-122).  The class of
# the result must be the reference's exactly -- NaN where numpy's cholesky
# propagates NaN (GPR:126 raises only for a non-positive finite pivot), inf
# where it raises LinAlgError (GPR:139-140) -- because scipy's line search
# branches on it; finite values at the T1 tolerance.  (Round 6: this test
# found two class mismatches, both fixed -- sn2 = exp(-800) = 0 gave NaN
# through the duplicate-site terms' 0/0 where the reference is finite, and an
# infinite sf2 tripped the duplicate not-PD rule where numpy's cholesky
# propagates NaN.)  Not covered, by design: one-observation cells (the
# reference's 1 x 1 K keeps squareform's zero "distance" even for non-finite
# coordinates, and numpy raises on a 1 x 1 inf matrix) and
# near-singular points (sf2 / sn2 beyond 1e16), where finite vs not-PD is
# the reference's own rounding noise (test_duplicate_nonpd_band).
EXTREME_H = {
    'huge_ell': [30, 30, 30, 0, 0, 0],
    'tiny_ell': [-30, -30, -30, 0, -5, 0],
    'tiny_sn2': [12, 12, 1, 0, -50, 0],
    'ell_overflow': [800, 12, 1, 0, 0, 0],
    'sf2_overflow': [12, 12, 1, 800, 0, 0],
    'sn2_overflow': [12, 12, 1, 0, 800, 0],
    'sn2_underflow': [12, 12, 1, 0, -800, 0],
    'ell_underflow': [-800, 12, 1, 0, 0, 0],
    'nan_h': [np.nan, 12, 1, 0, 0, 0],
    'sf2_underflow': [12, 12, 1, -800, 0, 0],
    'lt_overflow': [12, 12, 800, 0, 0, 0],
    'all_overflow': [800, 800, 800, 800, 800, 0],
    'neg_inf_h': [-np.inf, 12, 1, 0, 0, 0],
    'pos_inf_sn2': [12, 12, 1, 0, np.inf, 0],
}


@pytest.mark.parametrize('dedup', ['1', '0'])
def test_extreme_hypers_match_reference_class(dedup, monkeypatch):
    monkeypatch.setenv('OI_DEDUP', dedup)
    cells = synthetic.make_cells([50, 300, 700], seed=77)
    names = list(EXTREME_H)
    h = np.array([EXTREME_H[k] for k in names for _ in range(cells.ncell)], float)
    big = synthetic.RaggedCells(np.concatenate([cells.xyt] * len(names)), np.concatenate([cells.z] * len(names)),
                                np.concatenate([[0]] + [cells.offs[1:] + k * cells.offs[-1] for k in range(len(names))]),
                                np.concatenate([cells.xs] * len(names)), cells.mean)
    mX = np.full(len(big.z), cells.mean)
    nlz, grad, st = _lib.nlml_grad_batch(big.xyt, big.z, mX, big.offs, h)
    bad = []
    with np.errstate(all='ignore'):
        for q in range(big.ncell):
            x, y, _ = big.cell(q)
            f, g = O.neg_log_ml(h[q], x, y, np.full(len(y), cells.mean))
            f = float(np.asarray(f).ravel()[0])
            name, n = names[q // cells.ncell], len(y)
            cls = lambda v: 'nan' if np.isnan(v) else ('+inf' if v == np.inf else '-inf' if v == -np.inf else 'fin')
            if cls(nlz[q]) != cls(f) or [cls(v) for v in grad[q, :5]] != [cls(v) for v in np.asarray(g)[:5]]:
                bad.append((name, n, 'class', nlz[q], f, grad[q, :5].tolist(), np.asarray(g)[:5].tolist()))
                continue
            if np.isfinite(f):
                ok, err = close(nlz[q], f)
                sc = np.abs(g) + grad_scale(h[q], x, y, np.full(len(y), cells.mean))
                okg, errg = close(grad[q], g, scale=np.maximum(sc, 1e-300))
                if not (ok and okg):
                    bad.append((name, n, 'value', err, errg))
    assert not bad, bad


# Pass 2 / predict-only (GPR:169-182) at the same kind of hypers, given as
# values (ell_x, ell_y, ell_t, sf2, sn2); cells of 0 and >= 50 observations
# (one-observation cells: see above).
EXTREME_HYP = {
    'ell_inf': [np.inf, 1e5, 3, 5e-3, 1e-3],
    'ell_zero': [0.0, 1e5, 3, 5e-3, 1e-3],
    'sf2_inf': [1e5, 1e5, 3, np.inf, 1e-3],
    'sf2_zero': [1e5, 1e5, 3, 0.0, 1e-3],
    'sn2_zero': [1e5, 1e5, 3, 5e-3, 0.0],
    'sn2_inf': [1e5, 1e5, 3, 5e-3, np.inf],
    'nan': [np.nan, 1e5, 3, 5e-3, 1e-3],
    'tiny_ell': [1e-3, 1e-3, 1e-5, 5e-3, 1e-3],
}


@pytest.mark.parametrize('dedup', ['1', '0'])
def test_extreme_predict_match_reference_class(dedup, monkeypatch):
    monkeypatch.setenv('OI_DEDUP', dedup)
    cells = synthetic.make_cells([0, 50, 300, 700], seed=78)
    names = list(EXTREME_HYP)
    hyp = np.array([EXTREME_HYP[k] for k in names for _ in range(cells.ncell)], float)
    big = synthetic.RaggedCells(np.concatenate([cells.xyt] * len(names)), np.concatenate([cells.z] * len(names)),
                                np.concatenate([[0]] + [cells.offs[1:] + k * cells.offs[-1] for k in range(len(names))]),
                                np.concatenate([cells.xs] * len(names)), cells.mean)
    out, status, _ = _lib.gpr_batch(big.xyt, big.z, big.offs, big.xs, big.mean, opt=False, hyp=hyp)
    bad = []
    cls = lambda v: 'nan' if np.isnan(v) else ('+inf' if v == np.inf else '-inf' if v == -np.inf else 'fin')
    with np.errstate(all='ignore'):
        for q in range(big.ncell):
            x, y, xs = big.cell(q)
            name, n = names[q // cells.ncell], len(y)
            try:  # GPR3D(opt=False): NaN 2-tuple on LinAlgError (GPR:187-191)
                fs, sd, lz = O.predict(x, y, xs, big.mean, hyp[q, :3], hyp[q, 3], hyp[q, 4])
                ref = np.array([float(np.ravel(fs)[0]), float(np.ravel(sd)[0]), float(lz)])
            except np.linalg.LinAlgError:
                ref = np.full(3, np.nan)
            got = out[q, :3]
            if [cls(v) for v in got] != [cls(v) for v in ref]:
                bad.append((name, n, 'class', got.tolist(), ref.tolist()))
                continue
            fin = np.isfinite(ref)
            if fin.any():
                ok, err = close(got[fin], ref[fin])
                if not ok:
                    bad.append((name, n, 'value', err, got.tolist(), ref.tolist()))
    assert not bad, bad


@pytest.mark.parametrize('dedup', ['1', '0'])
def test_repeated_site_nonfinite_coordinates(dedup, monkeypatch):
    """A cell whose observations all sit on ONE site (m = 1 < n): at a
    length-scale of 0 or NaN the reference's K has NaN between the identical
    observations (pdist of non-finite coordinates, GPR:93) and its nlZ is NaN;
    the site form must not hide that behind its one finite diagonal entry.
    Finite hypers: T1 as everywhere."""
    monkeypatch.setenv('OI_DEDUP', dedup)
    p = np.array([[3.1e6, 2.2e6, 4.0]])
    xyt = np.concatenate([np.repeat(p, 3, 0), [[3.0e6, 2.0e6, 1.0], [3.05e6, 2.1e6, 2.0]]])
    z = np.array([0.31, 0.29, 0.30, 0.27, 0.33])
    offs = np.array([0, 3, 5])
    hs = {'finite': [np.log(2e5), np.log(2e5), np.log(5.), np.log(5e-3), np.log(1e-3), 0.],
          'ell_underflow': [-800, np.log(2e5), np.log(5.), np.log(5e-3), np.log(1e-3), 0.],
          'ell_nan': [np.nan, np.log(2e5), np.log(5.), np.log(5e-3), np.log(1e-3), 0.]}
    for name, h in hs.items():
        H = np.tile(np.array(h, float), (2, 1))
        nlz, grad, st = _lib.nlml_grad_batch(xyt, z, np.full(5, 0.28), offs, H)
        for c in range(2):
            x, y = xyt[offs[c]:offs[c + 1]], z[offs[c]:offs[c + 1]]
            with np.errstate(all='ignore'):
                f, g = O.neg_log_ml(H[c], x, y, np.full(len(y), 0.28))
            f = float(np.asarray(f).ravel()[0])
            if np.isfinite(f):
                ok, err = close(nlz[c], f)
                assert ok, (name, c, nlz[c], f)
            else:
                assert np.isnan(f) == np.isnan(nlz[c]) and (np.isnan(f) or nlz[c] == f), (name, c, nlz[c], f)
