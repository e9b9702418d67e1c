"""GPU parity of ``k_svgp_train`` (csrc/oi_svgp.hip) away from its default
configuration: every accepted thread count, the three LDS / global layout
modes with their fallbacks, the shape limits and degenerate shapes, per-cell
inputs, the failure status and the timing diagnostic.  Companion of
tests/test_gpu_svgp.py (whose header states the tolerance form).

Oracle: oracle/svgp_oracle.py (``O.train``, ``O.predict_f``, ``O.notebook_Z``),
each case computed once and shared.  Every case is 12-20 Adam steps, n <= 300:
  parameters   |gpu - ref| <= 1e-10 * max(1, |ref|)
  ELBO log     relative 1e-12 (1e-10 at n = 300, M = 64, B = 256, where K_uu is
               conditioned at ~70 and the oracle's own one-ulp input
               sensitivity is 3.2e-13 on the final parameters)
  predict_f    mean / variance 1e-10 * max(1, |ref|)
Runs that differ only in where the panels are stored, in a diagnostic, or in
which launch a cell belongs to are compared bitwise.
"""
import functools
import re

import numpy as np
import pytest

from oracle import svgp_oracle as O
from optimalinterpolation_amd import _lib

pytestmark = pytest.mark.gpu

INIT = (25e3, 25e3, 1.0, 1.0, 0.1, 0.3)  # NB2: lengthscales, kernel var, noise var .1, mean
XS = (1e4, -2e4, 4.0)
TOL = 1e-10


def _cell(rng, n):
    x = np.stack([rng.uniform(-3e5, 3e5, n), rng.uniform(-3e5, 3e5, n),
                  rng.integers(0, 9, n).astype(float)], 1)
    y = 0.3 + 0.05 * np.sin(x[:, 0] / 1e5) + 0.02 * np.cos(x[:, 1] / 7e4) + rng.normal(0, 0.02, n)
    return x, y


@functools.lru_cache(maxsize=None)
def _case(n, M, B, random_Z=False):
    """Data and inducing inputs of one shape (read-only: shared between tests)."""
    rng = np.random.default_rng(1000 * n + 10 * M + B)
    x, y = _cell(rng, n)
    if random_Z:  # inside the box the data are drawn from (notebook_Z repeats rows at n = 1)
        Z = np.stack([rng.uniform(-3e5, 3e5, M), rng.uniform(-3e5, 3e5, M), rng.uniform(0, 8, M)], 1)
    else:
        Z = O.notebook_Z(x, M)
    for a in (x, y, Z):
        a.setflags(write=False)
    return x, y, Z


@functools.lru_cache(maxsize=None)
def _oracle(n, M, B, iters, log_every, random_Z=False, seed=7, init=INIT, xs=XS):
    x, y, Z = _case(n, M, B, random_Z)
    p, log = O.train(x, y, Z, init[:3], init[3], init[4], init[5], B=B, iterations=iters, seed=seed,
                     log_every=log_every)
    m, v = O.predict_f(p, np.array([xs]))
    th = p.flat()
    th.setflags(write=False)
    log.setflags(write=False)
    return m[0], v[0], th, log


def _gpu(n, M, B, iters, log_every, random_Z=False, seed=7, init=INIT, xs=XS):
    x, y, Z = _case(n, M, B, random_Z)
    pred, st, th, elbo = _lib.svgp_batch(x, y, [0, n], Z[None], [init], [xs], batch=B, iterations=iters,
                                         log_every=log_every, seed=seed, want_params=True)
    return pred[0], int(st[0]), th[0], (elbo[0] if elbo is not None else None)


def _same(a, b):
    """Bitwise equality of two _gpu results (or of rows of two batches)."""
    ok = np.array_equal(a[0], b[0], equal_nan=True) and a[1] == b[1] and np.array_equal(a[2], b[2], equal_nan=True)
    if a[3] is None or b[3] is None:
        return ok and a[3] is None and b[3] is None
    return ok and np.array_equal(a[3], b[3], equal_nan=True)


def _check(label, gpu, ref, elbo_tol=1e-12):
    pred, st, th, elbo = gpu
    m, v, th_ref, log = ref
    d = np.abs(th - th_ref) / np.maximum(1.0, np.abs(th_ref))
    dp = max(abs(pred[0] - m) / max(1.0, abs(m)), abs(pred[1] - v) / max(1.0, abs(v)))
    de = np.max(np.abs(elbo - log) / np.abs(log)) if len(log) else 0.0
    print(label, 'status', st, 'param rel', d.max(), 'elbo rel', de, 'pred rel', dp)
    assert st == 0
    assert np.isfinite(th).all() and d.max() <= TOL
    if len(log):
        assert elbo is not None and elbo.shape == log.shape
        assert np.allclose(elbo, log, rtol=elbo_tol, atol=0)
    else:
        assert elbo is None
    assert dp <= 1e-10


# ------------------------------------------------------------ a. thread counts
THREADS_CASE = (300, 13, 40, 20, 7)  # log_every = 7 does not divide 20: logs after steps 0, 7, 14


@pytest.mark.parametrize('threads', ['64', '128', '192', '256', '320', '512', '1024', '100'])
def test_thread_counts_vs_oracle(monkeypatch, threads):
    """Every accepted OI_SVGP_THREADS trains on the full gradient.  The kernel
    derivatives are split into four parts dealt to waves; below 256 threads (4
    waves) a wave has to take more than one part.  Summation grouping differs
    between thread counts, so each is held to the oracle, not to the others."""
    monkeypatch.setenv('OI_SVGP_THREADS', threads)
    gpu = _gpu(*THREADS_CASE)
    assert gpu[3].shape == (3,)
    _check('threads %s' % threads, gpu, _oracle(*THREADS_CASE))


def test_thread_count_rounds_down_to_a_wave_multiple(monkeypatch):
    """OI_SVGP_THREADS=100 runs as 64: bitwise equal."""
    monkeypatch.setenv('OI_SVGP_THREADS', '100')
    a = _gpu(*THREADS_CASE)
    monkeypatch.setenv('OI_SVGP_THREADS', '64')
    b = _gpu(*THREADS_CASE)
    assert _same(a, b)


# ------------------------------------------------------------ b. layout modes
# (n, M, B, default mode): mode 1 needs M <= B and the LDS panels within 160 KB
# (M = B = 64 needs 176 KB); mode 2 needs M <= B; everything else is mode 0
MODE_CASES = [(300, 16, 50, 1), (300, 32, 33, 1), (257, 50, 100, 1), (300, 64, 64, 0), (60, 13, 7, 0)]


def _mode_used(capfd):
    """The layout mode the library reports on its OI_SVGP_TIMING line."""
    err = capfd.readouterr().err
    found = re.findall(r'svgp phase cycles \(cell 0, threads \d+, mode (\d)\)', err)
    assert len(found) == 1, err
    return int(found[0])


@pytest.mark.parametrize('n,M,B,default_mode', MODE_CASES)
def test_layout_modes_bitwise_equal(monkeypatch, capfd, n, M, B, default_mode):
    """OI_SVGP_PANELS unset / 0 / 1 / 2 store the M x B panels and T3 in
    different places and compute the same arithmetic: bitwise equal, and the
    unset run meets the oracle.  The mode each request resolves to (read from
    the timing line, itself shown not to change results below) follows the
    documented fallbacks."""
    case = (n, M, B, 15, 4)
    monkeypatch.delenv('OI_SVGP_PANELS', raising=False)
    base = _gpu(*case)
    _check('modes M %d B %d' % (M, B), base, _oracle(*case))
    monkeypatch.setenv('OI_SVGP_TIMING', '1')
    capfd.readouterr()
    want = {None: default_mode, '0': 0, '1': default_mode, '2': 2 if M <= B else 0}
    for req, mode in want.items():
        if req is not None:
            monkeypatch.setenv('OI_SVGP_PANELS', req)
        got = _gpu(*case)
        assert _mode_used(capfd) == mode, (req, mode)
        assert _same(got, base), req


# ------------------------------------------------------------ c. limits and degenerate shapes
@pytest.mark.parametrize('n,M,B,iters,log_every,random_Z,elbo_tol', [
    (300, 64, 256, 12, 5, False, 1e-10),  # M and B at their limits: chol_lds / trinv_lds at full size
    (100, 64, 256, 12, 5, False, 1e-12),  # one batch spans three epochs of the permutation
    (1, 2, 4, 15, 4, True, 1e-12),        # permute cycle-walks a 4-element domain down to 1
    (2, 3, 1, 15, 4, False, 1e-12),       # B = 1, M > B
    (257, 50, 100, 12, 0, False, 1e-12),  # no logging passes: elbo NULL, batch number = step
    (300, 13, 40, 12, 50, False, 1e-12),  # log_every > iterations: one entry
])
def test_limits_vs_oracle(n, M, B, iters, log_every, random_Z, elbo_tol):
    gpu = _gpu(n, M, B, iters, log_every, random_Z)
    ref = _oracle(n, M, B, iters, log_every, random_Z)
    assert len(ref[3]) == (0 if log_every == 0 else -(-iters // log_every))
    _check('limits n %d M %d B %d' % (n, M, B), gpu, ref, elbo_tol)


def test_zero_iterations_predicts_from_the_initial_parameters():
    """iterations = 0, log_every = 0: predict_f on untouched Params, which come
    back as Params(...).flat().  Z, q_mu, q_sqrt and the mean are copies: exactly
    equal.  The five softplus-transformed entries are y + log(-expm1(-y)) on
    both sides by two maths libraries: log lands near -2.35 for the noise
    variance, where an ulp is 2 eps, and log, expm1 and the final sum may each
    differ by an ulp between the libraries: 8 eps of max(1, |ref|)."""
    n, M, B = 40, 5, 3
    x, y, Z = _case(n, M, B)
    pred, st, th, elbo = _gpu(n, M, B, 0, 0)
    p = O.Params(Z, INIT[:3], INIT[3], INIT[4], INIT[5])
    ref = p.flat()
    m, v = O.predict_f(p, np.array([XS]))
    d = np.abs(th[:5] - ref[:5]) / np.maximum(1.0, np.abs(ref[:5]))
    print('zero iterations: raw hyper rel', d.max(), 'pred', pred, m[0], v[0])
    assert st == 0 and elbo is None
    assert np.array_equal(th[5:], ref[5:])
    assert d.max() <= 8 * np.finfo(float).eps
    assert abs(pred[0] - m[0]) <= 1e-10 * max(1, abs(m[0])) and abs(pred[1] - v[0]) <= 1e-10 * max(1, abs(v[0]))


# ------------------------------------------------------------ d / e. batches
def _batch3(M, ns=(200, 150, 120), rng_seed=21):
    rng = np.random.default_rng(rng_seed)
    cells = [_cell(rng, n) for n in ns]
    Z = np.stack([O.notebook_Z(c[0], M) for c in cells])
    return cells, Z


def _run_batch(cells, Z, init, xs, B, iters, log_every, seed):
    X = np.concatenate([c[0] for c in cells])
    Y = np.concatenate([c[1] for c in cells])
    offs = np.cumsum([0] + [len(c[1]) for c in cells])
    pred, st, th, elbo = _lib.svgp_batch(X, Y, offs, Z, init, xs, batch=B, iterations=iters,
                                         log_every=log_every, seed=seed, want_params=True)
    return [(pred[c], int(st[c]), th[c], elbo[c]) for c in range(len(cells))]


def test_per_cell_init_and_target():
    """Each cell of a launch reads its own init row and its own target: with
    three different rows of each, cell c is bitwise equal to a one-cell call
    with its row and seed + c, and one of them meets the oracle."""
    M, B, iters, log_every, seed = 12, 40, 20, 7, 5
    init = np.array([[25e3, 25e3, 1.0, 1.0, 0.1, 0.3],
                     [40e3, 18e3, 1.5, 0.6, 0.05, 0.25],
                     [15e3, 33e3, 0.7, 1.8, 0.2, 0.35]])
    xs = np.array([[1e4, -2e4, 4.0], [-1.2e5, 5e4, 2.0], [2e5, 1.5e5, 7.0]])
    cells, Z = _batch3(M)
    got = _run_batch(cells, Z, init, xs, B, iters, log_every, seed)
    for c in range(3):
        one = _run_batch(cells[c:c + 1], Z[c:c + 1], init[c:c + 1], xs[c:c + 1], B, iters, log_every, seed + c)
        assert got[c][1] == 0 and _same(got[c], one[0]), c
    x, y = cells[1]
    p, log = O.train(x, y, Z[1], init[1, :3], init[1, 3], init[1, 4], init[1, 5], B=B, iterations=iters,
                     seed=seed + 1, log_every=log_every)
    m, v = O.predict_f(p, xs[1:2])
    _check('per-cell inputs, cell 1', got[1], (m[0], v[0], p.flat(), log))


@pytest.mark.parametrize('where', ['y', 'Z0'])
def test_failed_cell_reports_status_and_leaves_its_neighbours(where):
    """One non-finite value in the middle cell's y (or in a row of its Z0): that
    cell reports status 1 with NaN predictions, and cells 0 and 2 are bitwise
    what they are when the middle cell is clean.  (The kernel's control flow
    depends on the shapes only, so NaN arithmetic runs the same instructions.)
    n = 60, B = 30, 12 steps: the stream passes over every row several times."""
    M, B, iters, log_every, seed = 10, 30, 12, 5, 2
    init = np.tile(INIT, (3, 1))
    xs = np.tile(XS, (3, 1))
    cells, Z = _batch3(M, ns=(70, 60, 50), rng_seed=22)
    clean = _run_batch(cells, Z, init, xs, B, iters, log_every, seed)
    assert [r[1] for r in clean] == [0, 0, 0]
    bad_cells, bad_Z = [(c[0], c[1].copy()) for c in cells], Z.copy()
    if where == 'y':
        bad_cells[1][1][17] = np.nan
    else:
        bad_Z[1, 3, 1] = np.inf
    bad = _run_batch(bad_cells, bad_Z, init, xs, B, iters, log_every, seed)
    assert bad[1][1] == 1 and np.isnan(bad[1][0]).all()
    assert _same(bad[0], clean[0]) and _same(bad[2], clean[2])


# ------------------------------------------------------------ f. diagnostics
def test_timing_diagnostic_leaves_results_unchanged(monkeypatch, capfd):
    case = (300, 16, 50, 15, 4)
    monkeypatch.delenv('OI_SVGP_TIMING', raising=False)
    base = _gpu(*case)
    monkeypatch.setenv('OI_SVGP_TIMING', '1')
    capfd.readouterr()
    timed = _gpu(*case)
    _mode_used(capfd)  # the phase line was printed: the diagnostic was on
    assert _same(timed, base)
