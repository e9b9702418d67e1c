"""Edge shapes, long batches and the fit's grouping of the Nystrom path
(csrc/oi_nystrom.hip, csrc/oi_nystrom_fit.hip) against the float64 oracle, with the bars of
tests/test_gpu_nystrom.py (tests/nystrom_cases.assert_cell) and bitwise
equality wherever the same per-cell arithmetic runs in another arrangement.

The fixture cells of tests/test_gpu_nystrom.py have M <= 64 < n, one padded
size per batch and at most ten cells; every index or leading-dimension
decision below is one they cannot tell from a wrong one.  What trips where:

  M = 1, M = n                      test_edge_shapes_vs_oracle: (1,1) (2,1) (65,1); (2,2) (5,5) (63,63)
                                    (64,64) (65,65) (128,128)
  M in 65..128 (Tk = 2, nd64_ = 2)  test_edge_shapes_vs_oracle: (65,65) (129,65) (193,96) (128,128),
                                    nlz / grad / sd of those cells; with n <= 200 here
  n < 64 (masked tiles)             test_edge_shapes_vs_oracle: grad of (1,1) .. (63,63)
  n = 65, 128, 129 (ntri 3 and 6,   test_edge_shapes_vs_oracle: grad of (65,*) (128,128) (129,65)
   one-row last tile, k_gemm128)    (130,129); test_edge_shapes_alternate_paths: OI_GEMM128=0 bitwise
  per-cell Mp inside mpmax_^2 slots test_edge_shapes_vs_oracle: (33,32) (65,64) (127,64) (193,96)
                                    (128,128) share one Runner with Mp = 160; OI_NYS_PAD=0 run;
                                    test_batch_equals_singles_any_order (alone, Mp = mpmax_)
  > 64 cells per call               test_more_cells_than_a_chunk: oracle per cell, 130 = 65 + 65 bitwise
  order_ not the identity           every batch (edge_cases is not M-sorted);
                                    test_batch_equals_singles_any_order: reversed order bitwise
  sel not ascending                 test_unsorted_inducing_rows
  predict-only calls                test_objective_only_and_predict_only
  OI_NYS_GROUPS, unequal groups     test_fit_grouping_is_bitwise_neutral
  OI_NYS_CAP on the one-shot fit    test_cap_knob_leaves_one_shot_fit_alone
  tickets of unequal means, rounds  test_session_tickets_keep_their_own_mean
   that hold cells of both
  NaN cell beside healthy cells     test_nan_cell_leaves_mates_unchanged

All inputs come from seeds (tests/nystrom_cases.py); nothing is read from
tests/golden.  Worst error / bar ratios measured on the MI355X are in DESIGN.md.
"""
import numpy as np
import pytest

import nystrom_cases as C
from optimalinterpolation_amd import _lib

pytestmark = pytest.mark.gpu


def run(batch, objective=True, predict=True, **kw):
    """One _lib.nystrom_batch call: (nlz, grad, pred, status), None where not asked for."""
    return _lib.nystrom_batch(batch.xyt, batch.y, batch.offs, batch.sel, batch.soffs, batch.hyp,
                              xs=batch.xs if predict else None, mean=C.MEAN, objective=objective,
                              predict=predict, **kw)


def cell_of(res, k):
    """(nlz, grad, fs, sd, sprior) of cell k of a run; None where not computed."""
    nlz, grad, pred, _ = res
    return (None if nlz is None else nlz[k], None if grad is None else grad[k],
            *((None, None, None) if pred is None else pred[k]))


def same(a, b):
    """Bitwise equality of two results (NaN equal to NaN)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_vs_oracle(res, cases, title):
    """assert_cell on every clean case of a run; prints the worst error / bar
    ratio per quantity and the shape it occurred at."""
    worst = C.Worst()
    for k, c in enumerate(cases):
        if not c.clean:
            continue
        assert res[3][k] == 0, (title, c, res[3][k])
        worst.add(C.assert_cell(cell_of(res, k), C.reference(c), f"{k} {c} [{title}]"), f"({c.n},{c.M})")
    worst.report(f"{title}: worst error / bar")
    return worst


def assert_same_cell(a, ka, b, kb, what, fields=(0, 1, 2, 3)):
    for f in fields:
        if a[f] is None or b[f] is None:
            continue
        assert same(a[f][ka], b[f][kb]), (what, ('nlz', 'grad', 'pred', 'status')[f], a[f][ka], b[f][kb])


@pytest.fixture(scope='module')
def edge():
    """{hyper set: (cases, batch, default run)} -- run once per hyper set."""
    cache = {}

    def get(hname):
        if hname not in cache:
            cases = C.screen(C.edge_cases(C.HYPERS[hname]))
            b = C.Batch(cases)
            cache[hname] = (cases, b, run(b))
        return cache[hname]
    return get


@pytest.mark.parametrize('hname', ['H1', 'H2', 'H3'])
def test_edge_shapes_vs_oracle(edge, hname):
    """All EDGE_SHAPES in ONE ragged call (objective and prediction), listed in
    an order that is not M-sorted, every cell against the oracle."""
    cases, b, res = edge(hname)
    check_vs_oracle(res, cases, f"edge shapes {hname}")


def test_edge_shapes_alternate_paths(edge, monkeypatch):
    """The H1 batch on the unfused objective (OI_NYS_FUSED=0: oila::gemm forming
    Ki, then k_nys_grad), without padding (OI_NYS_PAD=0: every cell its own
    Mp = M) and on 64 x 64 GEMM tiles only (OI_GEMM128=0): each against the
    oracle; the last bitwise equal to the default."""
    cases, b, res = edge('H1')
    for var in ('OI_NYS_FUSED', 'OI_NYS_PAD', 'OI_GEMM128'):
        with monkeypatch.context() as m:
            m.setenv(var, '0')
            alt = run(b)
        check_vs_oracle(alt, cases, f"edge shapes H1, {var}=0")
        if var == 'OI_GEMM128':
            for f in range(4):
                assert same(alt[f], res[f]), (var, f)


def test_batch_equals_singles_any_order(edge):
    """The H2 batch, the same cells in reversed order, and each cell alone (its
    own nmax, mmax, Mp = mpmax_): bitwise equal per cell."""
    cases, b, res = edge('H2')
    nc = len(cases)
    rev = run(C.Batch(cases[::-1]))
    for k, c in enumerate(cases):
        assert_same_cell(res, k, rev, nc - 1 - k, f"reversed batch, cell {c}")
        assert_same_cell(res, k, run(C.Batch([c])), 0, f"cell {c} alone")


def test_more_cells_than_a_chunk():
    """130 cells in one call (Runner::enqueue's chunks of 64 + 64 + 2 in M-sorted
    order): every cell against the oracle, and bitwise equal to two calls of
    65 (chunks of 64 + 1 over other M-sorted positions)."""
    cases = C.screen(C.chunk_cases())
    assert len(cases) == 130
    res = run(C.Batch(cases))
    check_vs_oracle(res, cases, "130 cells")
    for a in (0, 65):
        half = run(C.Batch(cases[a:a + 65]))
        for k in range(65):
            assert_same_cell(res, a + k, half, k, f"cell {a + k} {cases[a + k]} in a call of 65")


def test_objective_only_and_predict_only(edge):
    """(objective, predict) = (True, False), (False, True), (True, True): the
    predict-only Runner allocates no objective scratch and k_nys_scale gets
    sq == nullptr; results bitwise equal between the runs that produce them,
    and each within the bars."""
    cases = C.screen([C.Case(n, M, C.H2) for n, M in ((129, 65), (1, 1), (128, 128), (65, 1), (40, 33), (65, 65))])
    b = C.Batch(cases)
    obj, pred, both = run(b, True, False), run(b, False, True), run(b, True, True)
    assert obj[2] is None and pred[0] is None and pred[1] is None
    for r, t in ((obj, 'objective only'), (pred, 'predict only'), (both, 'both')):
        check_vs_oracle(r, cases, t)
    assert same(obj[0], both[0]) and same(obj[1], both[1]), "nlz / grad differ without the prediction"
    assert same(pred[2], both[2]), "pred differs without the objective"
    assert same(obj[3], both[3]) and same(pred[3], both[3])


def test_unsorted_inducing_rows():
    """sel reversed and sel shuffled, passed straight to the ABI (which asks for
    no order): the Nystrom quantities are invariant under a permutation of the
    inducing rows up to summation order, so each run meets the oracle's bars."""
    rng = np.random.default_rng(77)
    for hname in ('H1', 'H2'):
        cases = C.screen([C.Case(n, M, C.HYPERS[hname]) for n, M in ((70, 31), (129, 65), (65, 65))])
        for name, perm in (('reversed', lambda s: s[::-1]), ('shuffled', lambda s: rng.permutation(s))):
            sels = [perm(c.sel) for c in cases]
            assert all(np.any(np.diff(s) < 0) for s in sels)
            check_vs_oracle(run(C.Batch(cases, sel=sels)), cases, f"sel {name} {hname}")


@pytest.mark.parametrize('shape', [(65, 65), (33, 32)])
def test_nan_cell_leaves_mates_unchanged(edge, shape):
    """One NaN coordinate in an inducing row of one cell of the H1 batch: every
    other cell is bitwise what it was, and the NaN cell gives what it gives
    alone (NaN objective, as the oracle)."""
    cases, b, res = edge('H1')
    k = [(c.n, c.M) for c in cases].index(shape)
    bad = cases[k].with_nan(int(cases[k].sel[3]))
    mixed = cases[:k] + [bad] + cases[k + 1:]
    got = run(C.Batch(mixed))
    for j, c in enumerate(cases):
        if j != k:
            assert_same_cell(got, j, res, j, f"mate {c} of the NaN cell {shape}")
    ref = C.reference(bad)
    assert np.isnan(ref[0]), "the oracle's objective of the NaN cell is not NaN"
    assert np.isnan(got[0][k]), (shape, got[0][k])
    alone = run(C.Batch([bad]))
    assert_same_cell(got, k, alone, 0, f"NaN cell {shape} alone", fields=(0, 1, 3))


# ------------------------------------------------------------------- the fit --
def _fit(cases, **kw):
    b = C.Batch(cases)
    return _lib.nystrom_fit_batch(b.xyt, b.y, b.offs, b.sel, b.soffs, C.H1, b.xs, C.MEAN,
                                  maxiter=C.FIT_MAXITER, **kw)


@pytest.fixture(scope='module')
def fit_default():
    cases = C.screen(C.fit_cases())
    return cases, _fit(cases)


def test_fit_grouping_is_bitwise_neutral(fit_default, monkeypatch):
    """oi_nystrom_fit_batch on five cells (maxiter 30): the default two groups
    (3 and 2 cells), one group, three groups (2, 2, 1), each cell alone, and a
    session with OI_NYS_CAP=2 give bitwise the same out, status and info.

    The session gets (65,65) as a first ticket and (5,5), (70,31) as a second.
    All three start in the same round and (65,65) needs the fewest evaluations
    (70 against 104 and 108 in scipy; asserted below on the fit's own counts),
    so waiting for the first ticket leaves the other two in rounds in flight
    when the last batch arrives with the larger nmax = 129, and build_runners
    rebuilds the Runners with cells still active."""
    cases, ref = fit_default
    assert ref[2][:, 0].max() <= C.FIT_MAXITER
    print('fit info (nit, status, nfev, nobj):', ref[2].tolist())
    parts = [[1], [4, 0], [2, 3]]
    assert min(ref[2][i, 3] for i in parts[1]) > ref[2][parts[0][0], 3] + 5, \
        "the first ticket's cell no longer finishes first: reorder the session's tickets"
    for G in ('1', '3'):
        with monkeypatch.context() as m:
            m.setenv('OI_NYS_GROUPS', G)
            got = _fit(cases)
        for f in range(3):
            assert same(got[f], ref[f]), (f"OI_NYS_GROUPS={G}", f, got[f], ref[f])
    for k, c in enumerate(cases):
        got = _fit([c])
        for f in range(3):
            assert same(got[f][0], ref[f][k]), (f"cell {c} alone", f, got[f][0], ref[f][k])
    assert max(cases[i].n for i in parts[2]) > max(cases[i].n for i in parts[0] + parts[1])
    monkeypatch.setenv('OI_NYS_CAP', '2')
    with _lib.NystromSession(maxiter=C.FIT_MAXITER) as s:
        tickets = []
        for j, idx in enumerate(parts):
            b = C.Batch([cases[i] for i in idx])
            tickets.append(s.submit(b.xyt, b.y, b.offs, b.sel, b.soffs, C.H1, b.xs, C.MEAN))
            if j == 1:
                first = s.wait(tickets[0])
        res = [first, s.wait(tickets[1]), s.wait(tickets[2])]
    for idx, r in zip(parts, res):
        for q, i in enumerate(idx):
            for f in range(3):
                assert same(r[f][q], ref[f][i]), (f"session, cell {cases[i]}", f, r[f][q], ref[f][i])


def test_fit_matches_scipy_where_decidable(fit_default):
    """The same fit against scipy's minimize(method='CG', jac=True) on the
    oracle objective (as test_fit_matches_scipy_on_oracle): same nit and
    status, hypers within 1e-6 -- for the cells that pass the CPU screen
    nystrom_cases.fit_screen (nit and status unchanged under a 1 +- 1e-13
    scaling of the oracle's f and g); at least three of the five must, and
    with the seeds of nystrom_cases.FIT_SEED_STEP all five do."""
    cases, (out, status, info) = fit_default
    xh = np.log(out[:, 3:])
    admitted = 0
    for k, c in enumerate(cases):
        r, ok = C.fit_screen(c)
        print(c, 'gpu', info[k].tolist(), np.exp(xh[k]), '| scipy', r.nit, r.status, r.nfev, np.exp(r.x),
              '| admitted' if ok else '| not decidable')
        if not ok:
            continue
        admitted += 1
        assert info[k, 0] == r.nit and info[k, 1] == r.status, (c, info[k], r.nit, r.status)
        assert np.all(np.abs(xh[k] - r.x) <= 1e-6 * np.maximum(1.0, np.abs(r.x))), (c, xh[k], r.x)
    assert admitted >= 3, admitted


def _nys_launches():
    k = _lib.profile_json()['kernels']
    return {n: k[n]['launches'] for n in k if n.startswith('nys_')}


def test_cap_knob_leaves_one_shot_fit_alone(monkeypatch):
    """OI_NYS_CAP sizes a session's groups only: the one-shot fit of the five
    fit cells with OI_NYS_CAP=1 and without it gives bitwise the same out,
    status and info, and the same profiled nys_* launch counts (the batched
    factorisations are launched once per run of equal padded M in a round, so
    groups of one cell would launch more of them)."""
    cases = C.screen(C.fit_cases())
    runs = []
    for cap in ('1', None):
        with monkeypatch.context() as m:
            if cap is None:
                m.delenv('OI_NYS_CAP', raising=False)
            else:
                m.setenv('OI_NYS_CAP', cap)
            _lib.profile_reset()
            res = _fit(cases, profile=True)
            runs.append((res, _nys_launches()))
    _lib.profile_reset()
    (capped, lc), (plain, lp) = runs
    print('nys_* launches:', lp)
    assert lp and lp.get('nys_grad', 0) > 0, lp
    for f in range(3):
        assert same(capped[f], plain[f]), ('OI_NYS_CAP=1', f, capped[f], plain[f])
    assert lc == lp, (lc, lp)


@pytest.mark.parametrize('groups', [None, '1'])
def test_session_tickets_keep_their_own_mean(groups, monkeypatch):
    """Two tickets with different prior means, submitted back to back to one
    session with OI_NYS_CAP=2 before any wait: (40,33), (65,64) at 0.28 and
    (33,32), (70,31) at -1.5.  Each ticket's rows equal nystrom_fit_batch of
    its cells at its own mean, bitwise.  With the default two groups each
    ticket fills one group; with OI_NYS_GROUPS=1 the second ticket's cells are
    admitted as the first's finish, so rounds hold cells of both tickets: only
    that case mixes means within a round.  A guard, not a regression test: no
    objective round has ever read a mean, and now none is given one.

    That the comparison would notice a wrong mean: the first ticket's cells
    fitted at the other mean differ from it in fs (column 0) in every row, and
    in nothing else."""
    shapes = ([(40, 33), (65, 64)], [(33, 32), (70, 31)])
    means = (0.28, -1.5)
    for s in shapes[0] + shapes[1]:
        assert s in C.EDGE_SHAPES
    tickets = [C.screen([C.Case(n, M, C.H1) for n, M in part]) for part in shapes]
    monkeypatch.setenv('OI_NYS_CAP', '2')
    if groups is None:
        monkeypatch.delenv('OI_NYS_GROUPS', raising=False)
    else:
        monkeypatch.setenv('OI_NYS_GROUPS', groups)

    def one_shot(cases, mean):
        b = C.Batch(cases)
        return _lib.nystrom_fit_batch(b.xyt, b.y, b.offs, b.sel, b.soffs, C.H1, b.xs, mean, maxiter=C.FIT_MAXITER)
    ref = [one_shot(cases, mean) for cases, mean in zip(tickets, means)]
    other = one_shot(tickets[0], means[1])
    assert np.all(other[0][:, 0] != ref[0][0][:, 0]), (other[0][:, 0], ref[0][0][:, 0])
    assert np.all(np.abs((ref[0][0][:, 0] - other[0][:, 0]) - (means[0] - means[1])) <= 1e-12)
    assert same(other[0][:, 1:], ref[0][0][:, 1:]) and same(other[2], ref[0][2])
    with _lib.NystromSession(maxiter=C.FIT_MAXITER) as s:
        ids = []
        for cases, mean in zip(tickets, means):
            b = C.Batch(cases)
            ids.append(s.submit(b.xyt, b.y, b.offs, b.sel, b.soffs, C.H1, b.xs, mean))
        got = [s.wait(t) for t in ids]
    for j in range(2):
        for f in range(3):
            assert same(got[j][f], ref[j][f]), (f"ticket {j} (mean {means[j]})", f, got[j][f], ref[j][f])
