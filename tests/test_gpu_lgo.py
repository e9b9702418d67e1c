"""GPU parity of ``oi_gpr_lgo``: leave-group-out cross-validation per cell from
one factorisation (GPML 5.4.2 in block form).

References: tests/lgo_ref.py -- ``lgo_closed`` (the block formulas in numpy) and
``lgo_brute`` (one fit per group, the joint density from the full predictive
covariance); tests/test_lgo_ref.py holds them within 1e-11 of each other on
these inputs.  Bounds, the project's T1, fixed before any GPU run, against both:
  mu    |gpu - ref| <= 1e-10 * max(1, |ref|)
  sd    |gpu - ref| <= 1e-10 * ref
  lpd   |gpu - ref| <= 1e-10 * max(1, |ref|)
  d2    |gpu - ref| <= 1e-10 * max(1, ref)
  lpl   |gpu - ref| <= 1e-10 * max(1, |ref|)
The inputs (lgo_ref.SPECS): n in {1, 2, 63, 64, 65, 130, 333, 700} with
repeated sites, groups of 1, 2, 63, 64, 65, 128, 129 and 130 that start, after
the sort, at 0, 1 and 63 past a block boundary (130 at 63 spans three), a whole
cell as one group, all singletons, the groups of gpr.site_groups, labels
interleaved, negative and near 2^62.  Batch mates, chunking, device inputs,
dropped outputs and the label values must not change a bit of a cell's results.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, gpr, nystrom, synthetic
import lgo_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
NAMES = [s[0] for s in R.SPECS]


def _same(a, b):
    """Bit for bit (NaN equal to NaN)."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def _check(tag, got, ref):
    """One cell's (mu, sd, lpd, d2, lpl) against a reference's, to the bounds above."""
    print(f"{tag}: n {len(ref[0])} dmu dsd/sd dlpd dd2 dlpl", ' '.join(f'{v:.3e}' for v in R.errors(got, ref)))
    one = lambda a: np.maximum(1.0, np.abs(a))
    assert np.all(np.abs(got[0] - ref[0]) <= RTOL * one(ref[0])), tag
    assert np.all(np.abs(got[1] - ref[1]) <= RTOL * ref[1]), tag
    assert np.all(np.abs(got[2] - ref[2]) <= RTOL * one(ref[2])), tag
    assert np.all(np.abs(got[3] - ref[3]) <= RTOL * one(ref[3])), tag
    assert abs(got[4] - ref[4]) <= RTOL * max(1.0, abs(ref[4])), tag


def _cut(res, offs, c):
    """Cell c's (mu, sd, lpd, d2, lpl [1], status [1]) out of a batch result."""
    a, e = offs[c], offs[c + 1]
    return tuple(v[a:e] for v in res[:4]) + (res[4][c:c + 1], res[5][c:c + 1])


def _cell(res, offs, c):
    """The same with lpl a scalar, as the references return it."""
    v = _cut(res, offs, c)
    return v[:4] + (v[4][0],)


@pytest.fixture(scope='module')
def base():
    return R.batch()


@pytest.fixture(scope='module')
def result(base):
    xyt, z, offs, lab, mean, hyp = base
    return _lib.gpr_lgo(xyt, z, offs, lab, mean, hyp)


@pytest.mark.parametrize('name', NAMES)
def test_against_both_references(name, base, result):
    c = NAMES.index(name)
    assert result[5][c] == 0
    closed, brute = R.refs(name)
    _check(f"{name} closed", _cell(result, base[2], c), closed)
    _check(f"{name} brute", _cell(result, base[2], c), brute)


def test_fixture_cells_at_their_fitted_hypers():
    d = load_golden('gpr3d.npz')
    mean, offs = float(d['mean']), d['offs']
    sizes = np.diff(offs)
    assert sizes.min() == 0 and sizes.max() == 300
    lab = (np.arange(offs[-1]) * 7) % 5 - 2           # five groups per cell, interleaved
    res = _lib.gpr_lgo(d['x'], d['y'], offs, lab, mean, d['hyp2'])
    assert not res[5].any()
    for c, n in enumerate(sizes):
        x, z, g = d['x'][offs[c]:offs[c + 1]], d['y'][offs[c]:offs[c + 1]], lab[offs[c]:offs[c + 1]]
        _check(f"cell {c} closed", _cell(res, offs, c), R.lgo_closed(x, z, g, mean, d['hyp2'][c]))
        if n <= 200:
            _check(f"cell {c} brute", _cell(res, offs, c), R.lgo_brute(x, z, g, mean, d['hyp2'][c]))
    assert res[4][sizes == 0].tolist() == [0.0] * int((sizes == 0).sum())


@pytest.mark.parametrize('name', ['two', 'n63-singletons', 'n130-singletons'])
def test_singletons_are_leave_one_out(name, base, result):
    xyt, z, offs, lab, mean, hyp = base
    c = NAMES.index(name)
    a, e = offs[c], offs[c + 1]
    lmu, lsd, llpl, lst = _lib.gpr_loo(xyt[a:e], z[a:e], [0, e - a], mean, hyp[c:c + 1])
    mu, sd, lpd, d2, lpl = _cell(result, offs, c)
    assert lst[0] == 0
    assert np.all(np.abs(mu - lmu) <= RTOL * np.maximum(1.0, np.abs(lmu)))
    assert np.all(np.abs(sd - lsd) <= RTOL * lsd)
    assert abs(lpl - llpl[0]) <= RTOL * max(1.0, abs(llpl[0]))
    want = ((z[a:e] - lmu) / lsd) ** 2
    assert np.all(np.abs(d2 - want) <= RTOL * np.maximum(1.0, want))


@pytest.mark.parametrize('name', ['one', 'n64-whole'])
def test_the_whole_cell_as_one_group_is_the_prior(name, base, result):
    c = NAMES.index(name)
    mu, sd, lpd, d2, lpl = _cell(result, base[2], c)
    prior = np.sqrt(R.HYP[3] + R.HYP[4])
    assert np.all(np.abs(mu - base[4]) <= RTOL * max(1.0, abs(base[4])))
    assert np.all(np.abs(sd - prior) <= RTOL * prior)
    assert np.all(lpd == lpd[0]) and np.all(d2 == d2[0]) and lpl == lpd[0]


def test_agrees_with_the_brute_force_batch(base, result):
    """The parent's only route: one cell per group through oi_gpr_predict_multi
    with the covariance, that group removed and its members as targets; the
    noise and the joint density added on the host."""
    xyt, z, offs, lab, mean, hyp = base
    c = NAMES.index('n65-five')
    x, zz, g = xyt[offs[c]:offs[c + 1]], z[offs[c]:offs[c + 1]], lab[offs[c]:offs[c + 1]]
    members = R.groups_of(g)
    assert [len(m) for m in members] == R.SIZES_65
    rest = [np.setdiff1d(np.arange(65), m) for m in members]
    fs, _, _, cov, st = _lib.gpr_predict_multi(
        np.concatenate([x[r] for r in rest]), np.concatenate([zz[r] for r in rest]),
        np.concatenate([[0], np.cumsum([len(r) for r in rest])]), np.concatenate([x[m] for m in members]),
        np.concatenate([[0], np.cumsum([len(m) for m in members])]), mean, np.tile(R.HYP, (5, 1)), cov=True, lz=False)
    assert not st.any()
    toffs = np.concatenate([[0], np.cumsum([len(m) for m in members])])
    mu, sd, lpd, d2, lpl = (np.empty(65) for _ in range(5))
    for q, (m, S) in enumerate(zip(members, _lib.split_cov(cov, toffs))):
        S = S + np.eye(len(m)) * R.HYP[4]
        Ls = np.linalg.cholesky(S)
        u = np.linalg.solve(Ls, zz[m] - fs[toffs[q]:toffs[q + 1]])
        mu[m], sd[m], d2[m] = fs[toffs[q]:toffs[q + 1]], np.sqrt(np.diag(S)), u @ u
        lpd[m] = -0.5 * (u @ u) - np.log(np.diag(Ls)).sum() - 0.5 * len(m) * R.LOG2PI
    _check("n65-five predict_multi", _cell(result, offs, c), (mu, sd, lpd, d2, sum(lpd[m[0]] for m in members)))


def test_batch_equals_single(base, result):
    xyt, z, offs, lab, mean, hyp = base
    for c in range(len(NAMES)):
        a, e = offs[c], offs[c + 1]
        one = _lib.gpr_lgo(xyt[a:e], z[a:e], [0, e - a], lab[a:e], mean, hyp[c:c + 1])
        assert _same(one, _cut(result, offs, c)), NAMES[c]


def test_chunking_is_bitwise_neutral(base, result):
    xyt, z, offs, lab, mean, hyp = base
    cs, _ = R.cases()
    pool = 8 * (16 * 32 + max(R.cell_form(len(c[2]), c[4], True) for c in cs))   # the largest cell and the slack
    _lib.profile_reset()
    res = _lib.gpr_lgo(xyt, z, offs, lab, mean, hyp, pool_bytes=pool, profile=True)
    prof = _lib.profile_json()['kernels']
    _lib.profile_reset()
    assert prof['lgo_gram']['launches'] >= 3, prof
    assert {'lgo_generate', 'lgo_cholesky', 'lgo_solve', 'lgo_sweep', 'lgo_gram', 'lgo_groups'} <= set(prof)
    assert _same(res, result)
    with pytest.raises(_lib.OiError, match=r"error -3: a cell's leave-group-out workspace does not fit pool_bytes"):
        _lib.gpr_lgo(xyt, z, offs, lab, mean, hyp, pool_bytes=pool - 8)


def test_device_inputs_equal_host_inputs(base, result):
    import torch
    xyt, z, offs, lab, mean, hyp = base
    x = torch.from_numpy(xyt).to('cuda:0')
    zz = torch.from_numpy(z).to('cuda:0')
    assert _same(_lib.gpr_lgo_device(x, zz, offs, lab, mean, hyp, device=0), result)
    assert torch.equal(x.cpu(), torch.from_numpy(xyt)) and torch.equal(zz.cpu(), torch.from_numpy(z))


def test_without_lpd_d2_lpl_nothing_else_changes(base, result):
    xyt, z, offs, lab, mean, hyp = base
    mu, sd, lpd, d2, lpl, st = _lib.gpr_lgo(xyt, z, offs, lab, mean, hyp, lpd=False, d2=False, lpl=False)
    assert lpd is None and d2 is None and lpl is None
    assert _same((mu, sd, st), (result[0], result[1], result[5]))


def test_results_depend_on_the_partition_not_on_the_labels(base, result):
    xyt, z, offs, lab, mean, hyp = base
    rng = np.random.default_rng(9)
    # injective relabellings of the whole batch (3 is odd: the wrapped product stays injective)
    with np.errstate(over='ignore'):
        assert _same(_lib.gpr_lgo(xyt, z, offs, lab * 3 - 1, mean, hyp), result)
    assert _same(_lib.gpr_lgo(xyt, z, offs, lab ^ 0x2AAAAAAAAAAAAAAA, mean, hyp), result)
    # per cell: the label values permuted among the groups, and replaced by 0, 1, 2 ... in first-appearance order
    shuffled, ordered = lab.copy(), lab.copy()
    for c in range(len(NAMES)):
        g = lab[offs[c]:offs[c + 1]]
        vals, inv = np.unique(g, return_inverse=True)
        shuffled[offs[c]:offs[c + 1]] = rng.permutation(vals)[inv]
        first = {}
        ordered[offs[c]:offs[c + 1]] = [first.setdefault(v, len(first)) for v in g.tolist()]
    assert not np.array_equal(shuffled, lab)
    assert _same(_lib.gpr_lgo(xyt, z, offs, shuffled, mean, hyp), result)
    assert _same(_lib.gpr_lgo(xyt, z, offs, ordered, mean, hyp), result)


def test_failed_cell_is_nan_and_mates_unchanged(base, result):
    xyt, z, offs, lab, mean, hyp = base
    k = NAMES.index('n333')   # the n = 333 cell again, non-PD, in front of itself
    a, e = offs[k], offs[k + 1]
    bad = R.HYP.copy()
    bad[4] = -2.0 * bad[3]    # first pivot sf2 + sn2 <= 0
    with pytest.raises(np.linalg.LinAlgError):
        R.lgo_closed(xyt[a:e], z[a:e], lab[a:e], mean, bad)
    ins = lambda v: np.concatenate([v[:a], v[a:e], v[a:]])
    offs2 = np.concatenate([offs[:k + 1], offs[k:] + (e - a)])
    hyp2 = np.concatenate([hyp[:k], bad[None], hyp[k:]])
    res = _lib.gpr_lgo(ins(xyt), ins(z), offs2, ins(lab), mean, hyp2)
    assert res[5][k] == 1 and res[5].sum() == 1
    assert all(np.isnan(v[a:e]).all() for v in res[:4]) and np.isnan(res[4][k])
    keep = [c for c in range(len(hyp2)) if c != k]
    mates = tuple(np.concatenate([v[:a], v[e:]]) for v in res[:4]) + (res[4][keep], res[5][keep])
    assert _same(mates, result)


def test_empty_cells(base, result):
    xyt, z, offs, lab, mean, hyp = base
    offs2 = np.concatenate([offs[:4], offs[3:]])
    hyp2 = np.concatenate([hyp[:3], R.HYP[None], hyp[3:]])
    res = _lib.gpr_lgo(xyt, z, offs2, lab, mean, hyp2)
    assert res[4][3] == 0.0 and res[5][3] == 0
    keep = [c for c in range(len(hyp2)) if c != 3]
    assert _same(res[:4] + (res[4][keep], res[5][keep]), result)
    only = _lib.gpr_lgo(np.zeros((0, 3)), np.zeros(0), [0, 0], np.zeros(0, dtype=np.int64), mean, R.HYP[None])
    assert all(v.shape == (0,) for v in only[:4]) and only[4][0] == 0.0 and only[5][0] == 0


def test_lgo_cells_fit_then_cross_validate_by_site():
    d = load_golden('gpr3d.npz')
    cells = synthetic.RaggedCells(d['x'], d['y'], d['offs'], d['xs'], float(d['mean'])).subset([5, 6, 7])
    lab = gpr.site_groups(cells.xyt, cells.offs)
    ref8, rst, _ = gpr.gpr_cells(cells, opt=True, x0=O.X0_PRODUCTION)
    mu, sd, lpd, d2, lpl, out8, st = gpr.lgo_cells(cells, lab, opt=True, x0=O.X0_PRODUCTION)
    assert np.array_equal(out8, ref8) and not st.any() and not rst.any()
    direct = _lib.gpr_lgo(cells.xyt, cells.z, cells.offs, lab, cells.mean, out8[:, 3:8])
    assert _same((mu, sd, lpd, d2, lpl), direct[:5])
    assert np.isfinite(mu).all() and (sd > 0).all() and (d2 >= 0).all()
    # the notebook-style single cell: residual outputs in, the mean added back
    x, z, _ = cells.cell(1)
    g = lab[cells.offs[1]:cells.offs[2]]
    h = out8[1, 3:8]
    got = nystrom.GPR_lgo(x, z - cells.mean, g, list(h[:3]), h[3], h[4], cells.mean)
    one = _lib.gpr_lgo(x, z - cells.mean, [0, len(z)], g, 0.0, h[None])
    assert _same(got, (cells.mean + one[0], one[1], one[2], one[3], one[4][0]))
    _check("GPR_lgo", got, R.lgo_closed(x, z, g, cells.mean, h))
    bad = h.copy()
    bad[4] = -2.0 * bad[3]
    with pytest.raises(np.linalg.LinAlgError):
        nystrom.GPR_lgo(x, z - cells.mean, g, list(bad[:3]), bad[3], bad[4], cells.mean)
