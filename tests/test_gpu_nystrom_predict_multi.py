"""GPU tests of ``oi_nystrom_predict_multi``: NB1 GPR(approx=True) at many
targets per cell with the posterior covariance (include/oi.h).

Reference: the oracle's own functions (nystrom_multi_cases.reference):
  Ki, A = nystroem(...);  k = matern32(x, xs=xs)
  cov_ref = matern32(xs) - k' Ki k;  fs_ref = MEAN + k' A
Bars:
  fs   |fs - ref| <= 1e-10 max(1, |ref|)        (BARS['fs'] of nystrom_cases)
  cov  |cov - ref| <= 1e-9 max(sf2, |ref|)      entrywise: the project's sd bar
       on the covariance's own scale
  sd   NaN exactly where diag(cov_ref) < 0 (every |diag(cov_ref)| >= 1e-6 sf2 is
       asserted first), otherwise sqrt(diag(cov)) bit for bit
  cov  exactly symmetric
tests/test_nystrom_predict_multi_wform.py shows on the CPU that the algebra
itself sits three orders inside these bars.  Everything else here is bitwise:
a ragged batch against its single-cell calls, cov = None against cov, a subset
of targets against the full list, device inputs against host inputs.
"""
import numpy as np
import pytest

import nystrom_cases as NC
import nystrom_multi_cases as MC
from optimalinterpolation_amd import _lib, nystrom

pytestmark = pytest.mark.gpu

IDS = [f"n{n}M{M}" for n, M in MC.SHAPES]


def same(a, b):
    """Bitwise equality of two float arrays up to the payload of NaNs."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def call(n, M, hname, xs, cov=True, x=None, **kw):
    """One single-cell call: (fs, sd, cov [nt x nt] | None, status)."""
    cx, cy = MC.case_cell(n, M)
    x = cx if x is None else x
    ell, sf2, sn2 = MC.linear(hname)
    fs, sd, c, st = _lib.nystrom_predict_multi(x, cy, [0, n], NC.N.inducing_indices(n, M), [0, M],
                                               [ell + [sf2, sn2]], xs, [0, len(xs)], mean=MC.MEAN, cov=cov,
                                               **kw)
    return fs, sd, (c.reshape(len(xs), len(xs)) if cov else None), st


_SINGLE = {}


def single(n, M, hname, nt):
    """The single-cell call of a case with cov, made once (read-only)."""
    key = (n, M, hname, nt)
    if key not in _SINGLE:
        r = call(n, M, hname, MC.targets(n, nt))
        for a in r[:3]:
            a.setflags(write=False)
        _SINGLE[key] = r
    return _SINGLE[key]


@pytest.mark.parametrize('hname', MC.HNAMES)
@pytest.mark.parametrize('shape', MC.SHAPES, ids=IDS)
def test_parity_with_the_oracle(shape, hname):
    n, M = shape
    sf2 = MC.linear(hname)[1]
    for nt in MC.NTS:
        fs_ref, cov_ref = MC.reference(n, M, hname, nt)
        fs, sd, cov, st = single(n, M, hname, nt)
        assert st[0] == 0 and fs.shape == (nt,) and sd.shape == (nt,) and cov.shape == (nt, nt)
        efs = np.max(np.abs(fs - fs_ref) / np.maximum(1.0, np.abs(fs_ref)))
        ecov = np.max(np.abs(cov - cov_ref) / np.maximum(sf2, np.abs(cov_ref)))
        dref = np.diag(cov_ref)
        print(f"n={n} M={M} {hname} nt={nt}: fs {efs:.3g} / 1e-10, cov {ecov:.3g} / 1e-9, "
              f"{int((dref < 0).sum())} negative diagonals")
        assert np.isfinite(fs).all() and np.isfinite(cov).all()
        assert efs <= 1e-10, (nt, efs)
        assert ecov <= 1e-9, (nt, ecov)
        assert np.all(np.abs(dref) >= 1e-6 * sf2), nt      # the NaN class is decidable
        assert np.array_equal(np.isnan(sd), dref < 0), nt
        with np.errstate(invalid='ignore'):
            assert same(sd, np.sqrt(np.diag(cov))), nt
        assert np.array_equal(cov, cov.T), nt


# one ragged batch of every shape at both hyper sets: nt differs from cell to
# cell, one cell has no target
RAGGED_NT = (65, 1, 130, 0, 64, 63, 130, 65, 1, 64)


def _ragged():
    cases = [(n, M, h) for h in MC.HNAMES for n, M in MC.SHAPES]
    assert len(cases) == len(RAGGED_NT)
    cells = [MC.case_cell(n, M) for n, M, _ in cases]
    xyt = np.concatenate([c[0] for c in cells])
    y = np.concatenate([c[1] for c in cells])
    offs = np.cumsum([0] + [n for n, _, _ in cases])
    sel = np.concatenate([NC.N.inducing_indices(n, M) for n, M, _ in cases])
    soffs = np.cumsum([0] + [M for _, M, _ in cases])
    hyp = np.array([(lambda e, a, b: e + [a, b])(*MC.linear(h)) for _, _, h in cases])
    xs = np.concatenate([MC.targets(n, nt) for (n, _, _), nt in zip(cases, RAGGED_NT)])
    toffs = np.cumsum((0,) + RAGGED_NT)
    return cases, (xyt, y, offs, sel, soffs, hyp, xs, toffs)


def test_ragged_batch_equals_single_cell_calls():
    cases, args = _ragged()
    toffs = args[-1]
    fs, sd, cov, st = _lib.nystrom_predict_multi(*args, mean=MC.MEAN, cov=True)
    assert not st.any()
    covs = _lib.split_cov(cov, toffs)
    for c, ((n, M, h), nt) in enumerate(zip(cases, RAGGED_NT)):
        a, b = toffs[c], toffs[c + 1]
        assert covs[c].shape == (nt, nt)
        if nt == 0:
            continue
        f1, s1, c1, _ = single(n, M, h, nt)
        assert same(fs[a:b], f1) and same(sd[a:b], s1) and same(covs[c], c1), (c, n, M, h, nt)
    fs0, sd0, cov0, st0 = _lib.nystrom_predict_multi(*args, mean=MC.MEAN, cov=False)
    assert cov0 is None and not st0.any()
    assert same(fs0, fs) and same(sd0, sd)


@pytest.mark.parametrize('hname', MC.HNAMES)
def test_results_do_not_depend_on_the_other_targets(hname):
    n, M = 193, 96
    sub = [0, 64, 129]
    fs, sd, cov, _ = single(n, M, hname, 130)
    for want_cov in (True, False):
        f3, s3, c3, st = call(n, M, hname, MC.targets(n, 130)[sub], cov=want_cov)
        assert st[0] == 0
        assert same(f3, fs[sub]) and same(s3, sd[sub])
        if want_cov:
            assert same(c3, cov[np.ix_(sub, sub)])


def test_one_target_agrees_with_the_single_target_path():
    """nt = 1 at XS against oi_nystrom_batch's predict: fs within 1e-10, sd
    within 1e-9 (scale max(1, |ref|)) and NaN in the same cells; not bitwise,
    the two paths reduce in different orders."""
    for hname in MC.HNAMES:
        cases = NC.screen([NC.Case(n, M, NC.HYPERS[hname]) for n, M in MC.SHAPES])
        b = NC.Batch(cases)
        _, _, pred, st = _lib.nystrom_batch(b.xyt, b.y, b.offs, b.sel, b.soffs, b.hyp, xs=b.xs, mean=MC.MEAN,
                                            objective=False, predict=True)
        fs, sd, cov, st2 = _lib.nystrom_predict_multi(b.xyt, b.y, b.offs, b.sel, b.soffs, b.hyp, b.xs,
                                                      np.arange(len(cases) + 1), mean=MC.MEAN, cov=True)
        assert not st.any() and not st2.any()
        assert np.all(np.abs(fs - pred[:, 0]) <= 1e-10 * np.maximum(1.0, np.abs(pred[:, 0])))
        assert np.array_equal(np.isnan(sd), np.isnan(pred[:, 1]))
        ok = ~np.isnan(sd)
        assert np.all(np.abs(sd[ok] - pred[ok, 1]) <= 1e-9 * np.maximum(1.0, np.abs(pred[ok, 1])))
        with np.errstate(invalid='ignore'):
            assert same(sd, np.sqrt(cov))                 # nt = 1: cov is the cells' 1 x 1 matrices


def test_nan_inducing_row_propagates():
    """A NaN coordinate in an inducing row: numpy's eigh returns NaNs (no
    LinAlgError), so the oracle's fs and cov are NaN throughout -- and so is
    the single-target path's prediction, with its status; the many-target
    path gives the same class."""
    n, M, hname = 70, 31, 'H1'
    x = MC.case_cell(n, M)[0].copy()
    x[NC.N.inducing_indices(n, M)[3], 0] = np.nan
    xs = MC.targets(n, 65)
    fs, sd, cov, st = call(n, M, hname, xs, x=x)
    ell, sf2, sn2 = MC.linear(hname)
    y = MC.case_cell(n, M)[1]
    _, _, pred, st1 = _lib.nystrom_batch(x, y, [0, n], NC.N.inducing_indices(n, M), [0, M], [ell + [sf2, sn2]],
                                         xs=xs[:1], mean=MC.MEAN, objective=False, predict=True)
    with np.errstate(all='ignore'):
        Ki, A = NC.N.nystroem(x, y, M=M, ell=ell, sf2=sf2, sn2=sn2)
    assert np.isnan(Ki).all() and np.isnan(A).all()       # the reference's class
    assert np.isnan(pred[0, 0]) and np.isnan(pred[0, 1])  # the single-target path's
    assert st[0] == st1[0]
    assert np.isnan(fs).all() and np.isnan(sd).all() and np.isnan(cov).all()


def test_nan_target_poisons_its_own_row_and_column_only():
    n, M, nt, bad = 129, 65, 65, 10
    for hname in MC.HNAMES:
        xs = MC.targets(n, nt).copy()
        xs[bad, 1] = np.nan
        fs, sd, cov, st = call(n, M, hname, xs)
        f0, s0, c0, _ = single(n, M, hname, nt)
        keep = np.arange(nt) != bad
        assert st[0] == 0
        assert np.isnan(fs[bad]) and np.isnan(sd[bad])
        assert np.isnan(cov[bad, :]).all() and np.isnan(cov[:, bad]).all()
        assert same(fs[keep], f0[keep]) and same(sd[keep], s0[keep])
        assert same(cov[np.ix_(keep, keep)], c0[np.ix_(keep, keep)])


def test_device_inputs_equal_host_inputs():
    import torch
    cases, args = _ragged()
    ref = _lib.nystrom_predict_multi(*args, mean=MC.MEAN, cov=True)
    xd = torch.as_tensor(args[0], dtype=torch.float64, device='cuda:0').contiguous()
    yd = torch.as_tensor(args[1], dtype=torch.float64, device='cuda:0').contiguous()
    got = _lib.nystrom_predict_multi(xd, yd, *args[2:], mean=MC.MEAN, cov=True, device_inputs=True)
    for a, b in zip(got, ref):
        assert same(a, b)


def test_workspace_that_does_not_fit_is_nomem():
    n, M = 70, 31
    with pytest.raises(_lib.OiError, match=r'error -3: .*does not fit'):
        call(n, M, 'H1', MC.targets(n, 65), pool_bytes=4096)


def test_gpr_multi_surface():
    n, M, hname, nt = 70, 31, 'H2', 65
    x, y = MC.case_cell(n, M)
    ell, sf2, sn2 = MC.linear(hname)
    xs = MC.targets(n, nt)
    f1, s1, c1, _ = single(n, M, hname, nt)
    fs, sd = nystrom.GPR_multi(x, y, xs, ell, sf2, sn2, MC.MEAN, M=M)
    assert fs.shape == (nt, 1) and sd.shape == (nt,)
    assert same(fs[:, 0], f1) and same(sd, s1)
    fs, sd, sp, cov = nystrom.GPR_multi(x, y, xs, ell, sf2, sn2, MC.MEAN, M=M, returnprior=True, cov=True)
    assert sp == np.sqrt(sf2) and cov.shape == (nt, nt) and same(cov, c1)
    # M = None: NB1's int(n / 5) inducing rows
    fs5, sd5 = nystrom.GPR_multi(x, y, xs[:3], ell, sf2, sn2, MC.MEAN)
    k = NC.matern32(x, ell, sf2, xs=xs[:3])
    Ki, A = NC.N.nystroem(x, y, M=n // 5, ell=ell, sf2=sf2, sn2=sn2)
    ref = MC.MEAN + np.dot(k.T, A)
    assert np.all(np.abs(fs5 - ref) <= 1e-10 * np.maximum(1.0, np.abs(ref)))
    with pytest.raises(NotImplementedError, match='one target'):
        nystrom.GPR(x, y, xs[:2], ell, sf2, sn2, MC.MEAN, approx=True, M=M)


def test_fit_predict_multi_batch(golden):
    """Two small cells of the fixture tests/golden/nystrom.npz: the hypers are
    bitwise fit_batch's, and fs at the cell's own target (the fixture's xs,
    first of three targets here) is within 1e-8 -- the bar of
    test_fit_matches_scipy_on_oracle -- of the oracle's prediction at those
    hypers, and of what fit_predict_batch returns for that target."""
    d = golden('nystrom.npz')
    pick = (0, 6)
    cells = [(d['x'][d['offs'][c]:d['offs'][c + 1]], d['y'][d['offs'][c]:d['offs'][c + 1]], int(d['M'][c]))
             for c in pick]
    xyt = np.concatenate([c[0] for c in cells])
    y = np.concatenate([c[1] for c in cells])
    offs = np.cumsum([0] + [len(c[1]) for c in cells])
    Ms = np.array([c[2] for c in cells])
    mean = float(d['mean'])
    xs = np.concatenate([np.concatenate([d['xs'], MC.TGRID[3 * k:3 * k + 2]]) for k in range(len(cells))])
    toffs = [0, 3, 6]
    fs, sd, covs, st, xh, info = nystrom.fit_predict_multi_batch(xyt, y, offs, xs, toffs, mean, Ms, cov=True)
    xh0, info0 = nystrom.fit_batch(xyt, y, offs, Ms)
    assert np.array_equal(xh, xh0) and np.array_equal(info, info0)
    pred, _, _ = nystrom.fit_predict_batch(xyt, y, offs, np.repeat(d['xs'], len(cells), axis=0), mean, Ms)
    assert not st.any() and fs.shape == (6,) and sd.shape == (6,) and [c.shape for c in covs] == [(3, 3)] * 2
    for k, (x, yy, M) in enumerate(cells):
        h = np.exp(xh[k])
        ref, _, _ = NC.N.predict(x, yy, d['xs'], list(h[:3]), h[3], h[4], mean, M)
        ref = float(np.asarray(ref).item())
        print(k, 'fs', fs[3 * k], 'oracle', ref, 'single-target path', pred[k, 0])
        assert abs(fs[3 * k] - ref) <= 1e-8 * max(1.0, abs(ref))
        assert abs(fs[3 * k] - pred[k, 0]) <= 1e-8 * max(1.0, abs(pred[k, 0]))
