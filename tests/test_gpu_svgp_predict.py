"""GPU parity of ``oi_svgp_predict`` / ``oi_svgp_elbo``: GPflow's
``SVGP.predict_f`` / ``predict_y`` at many targets per cell and
``model.elbo((X, Y))`` on all of a cell's data, from ``params`` rows of the
layout ``oi_svgp_batch`` writes (``oracle.svgp_oracle.Params.flat``).

Oracle: ``oracle/svgp_oracle.py`` -- ``predict_f(p, xs)`` and
``-loss_and_grad(p, X, y, len(y), grad=False)``; the full covariance is the
NumPy ``K_ss - A'A + (S'A)'(S'A)`` built from ``O.matern32``.  Models are
synthetic (nothing trains) unless a test says otherwise: notebook inducing
points on ``_cell`` data, lengthscales (25 km, 25 km, 1 day), kernel variance
1, noise 0.1, mean 0.3, q_mu ~ N(0, 1), S = tril(N(0, 0.3)) with a U(0.2, 1.2)
diagonal.  Tolerances are the project's (tests/test_gpu_svgp.py, DESIGN T1):
mean and variance 1e-10 max(1, |ref|), covariance 1e-10 max(kvar, |ref|),
ELBO rtol 1e-12.  With such models cond(K_uu + jitter) is 1-70 and the oracle
itself moves by <= 9e-16 (solve against explicit inverse) and <= 1.7e-16
relative in the ELBO (row order), so the reference sits far inside each bound.
Every test prints the worst error it saw.
"""
import numpy as np
import pytest

from oracle import svgp_oracle as O
from optimalinterpolation_amd import _lib, svgp

pytestmark = pytest.mark.gpu

INIT = [25e3, 25e3, 1.0, 1.0, 0.1, 0.3]
TOL = 1e-10


def _cell(rng, n):
    x = np.stack([rng.uniform(-3e5, 3e5, n), rng.uniform(-3e5, 3e5, n),
                  rng.integers(0, 9, n).astype(float)], 1)
    y = 0.3 + 0.05 * np.sin(x[:, 0] / 1e5) + 0.02 * np.cos(x[:, 1] / 7e4) + rng.normal(0, 0.02, n)
    return x, y


def _model(rng, M, x=None, Z=None):
    if Z is None:
        Z = O.notebook_Z(x if x is not None else _cell(rng, 200)[0], M)
    p = O.Params(Z, [25e3, 25e3, 1], 1.0, 0.1, 0.3)
    p.q_mu = rng.normal(0, 1, M)
    S = np.tril(rng.normal(0, 0.3, (M, M)))
    S[np.diag_indices(M)] = rng.uniform(0.2, 1.2, M)
    p.S = S
    return p


def _targets(rng, p, nt):
    """nt targets; from nt = 4 on, row 1 equals an inducing point (the r2
    clamps) and the last row duplicates row 2."""
    xs = np.stack([rng.uniform(-3e5, 3e5, nt), rng.uniform(-3e5, 3e5, nt), rng.uniform(0, 8, nt)], 1)
    if nt >= 4:
        xs[1] = p.Z[len(p.Z) // 2]
        xs[-1] = xs[2]
    return xs


def _ref(p, xs):
    """(mean, var, cov) of the oracle; cov = K_ss - A'A + (S'A)'(S'A)."""
    m, v = O.predict_f(p, xs)
    ls, kv, _ = O.constrained(p)
    M = len(p.Z)
    L = np.linalg.cholesky(O.matern32(p.Z, p.Z, ls, kv)[0] + O.JITTER * np.eye(M))
    A = np.linalg.solve(L, O.matern32(p.Z, xs, ls, kv)[0])
    SA = np.tril(p.S).T @ A
    return m, v, O.matern32(xs, xs, ls, kv)[0] - A.T @ A + SA.T @ SA


def _err(got, ref, floor=1.0):
    return float(np.max(np.abs(got - ref) / np.maximum(floor, np.abs(ref)))) if len(ref) else 0.0


def _rows(ps):
    return np.stack([p.flat() for p in ps])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class Batch:
    """A ragged batch of synthetic models and targets (M shared)."""

    def __init__(self, seed, M, nts):
        rng = np.random.default_rng(seed)
        self.ps = [_model(rng, M) for _ in nts]
        self.xs = [_targets(rng, p, nt) for p, nt in zip(self.ps, nts)]
        self.toffs = np.cumsum([0] + list(nts))
        self.params = _rows(self.ps)
        self.XS = np.concatenate(self.xs)

    def run(self, cells=None, **kw):
        cells = range(len(self.ps)) if cells is None else cells
        xs = [self.xs[c] for c in cells]
        return _lib.svgp_predict(self.params[list(cells)], np.concatenate(xs),
                                 np.cumsum([0] + [len(a) for a in xs]), **kw)


NTS = (1, 63, 0, 64, 65, 130, 257)  # tile edges of 64 (cov) and 128 (targets), and a cell without targets


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize('M', [1, 12, 50, 64])
def test_predict_f_vs_oracle(M):
    b = Batch(100 + M, M, NTS)
    mean, var, cov, st = b.run(cov=True)
    mean0, var0, none, st0 = b.run()
    assert none is None and _same(mean0, mean) and _same(var0, var) and _same(st0, st)
    assert np.all(st == 0)
    covs = _lib.split_cov(cov, b.toffs)
    worst = [0.0, 0.0, 0.0]
    for c, (p, xs) in enumerate(zip(b.ps, b.xs)):
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        m, v, C = _ref(p, xs)
        kv = O.constrained(p)[1]
        worst[0] = max(worst[0], _err(mean[t0:t1], m))
        worst[1] = max(worst[1], _err(var[t0:t1], v))
        worst[2] = max(worst[2], _err(covs[c].ravel(), C.ravel(), kv))
        assert np.array_equal(covs[c], covs[c].T), c
        assert np.array_equal(covs[c].diagonal(), var[t0:t1]), c
        if len(xs) >= 4:  # the duplicated target: equal rows (and columns), equal mean / var
            assert np.array_equal(covs[c][2], covs[c][-1]), c
            assert mean[t0 + 2] == mean[t1 - 1] and var[t0 + 2] == var[t1 - 1]
    print(f'M {M}: mean {worst[0]:.2e} var {worst[1]:.2e} cov/kvar {worst[2]:.2e}')
    assert max(worst) <= TOL


# ---------------------------------------------------------------- 2. clustered Z
def test_moderately_clustered_inducing_points():
    """M = 16, the odd rows of Z 10 km east of the even rows, targets within 5 km
    of the inducing points: cond(K_uu + jitter) 12, the oracle within 3.4e-13
    of an 80-bit evaluation.  A gap of 100 m or less is deliberately not tested:
    there the reference's own expanded-distance rounding moves its answer by
    about 1e-10 (measured 4.6e-11 .. 3.3e-10 at cond 9e4 .. 2e6), so a 1e-10
    bound would test the reference, not the kernel."""
    rng = np.random.default_rng(16)
    Z = np.empty((16, 3))
    Z[0::2] = O.notebook_Z(_cell(rng, 200)[0], 8)
    Z[1::2] = Z[0::2] + [1e4, 0.0, 0.0]
    p = _model(rng, 16, Z=Z)
    nt = 130
    r, phi = rng.uniform(0, 5e3, nt), rng.uniform(0, 2 * np.pi, nt)
    xs = Z[rng.integers(0, 16, nt)] + np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros(nt)], 1)
    mean, var, cov, st = _lib.svgp_predict(p.flat(), xs, [0, nt], cov=True)
    m, v, C = _ref(p, xs)
    e = (_err(mean, m), _err(var, v), _err(cov, C.ravel(), O.constrained(p)[1]))
    print('clustered Z: mean %.2e var %.2e cov/kvar %.2e' % e)
    assert st[0] == 0 and max(e) <= TOL


# ---------------------------------------------------------------- 3. predict_y
def test_predict_y_adds_the_noise_variance():
    b = Batch(3, 12, (5, 130))
    mean, var, _, _ = b.run()
    my, vy, none, st = b.run(with_noise=True)
    assert none is None and np.all(st == 0)
    assert np.array_equal(my, mean)
    worst = 0.0
    for c, p in enumerate(b.ps):
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        worst = max(worst, _err(vy[t0:t1], var[t0:t1] + O.constrained(p)[2]))
        worst = max(worst, _err(vy[t0:t1], O.predict_f(p, b.xs[c])[1] + O.constrained(p)[2]))
    print(f'predict_y var {worst:.2e}')
    assert worst <= TOL


# ---------------------------------------------------------------- 4. training
def test_agrees_with_the_training_kernels_predict():
    rng = np.random.default_rng(312)
    x, y = _cell(rng, 300)
    xs = np.array([[1e4, -2e4, 4.0]])
    pred, st, params, _ = _lib.svgp_batch(x, y, [0, 300], O.notebook_Z(x, 12)[None], [INIT], xs, batch=40,
                                          iterations=15, seed=7, want_params=True)
    mean, var, _, st2 = _lib.svgp_predict(params, xs, [0, 1])
    d = (abs(mean[0] - pred[0, 0]), abs(var[0] - pred[0, 1]))
    print('predict vs oi_svgp_batch pred: mean %.2e var %.2e' % d, 'bitwise', d == (0.0, 0.0))
    assert st[0] == 0 and st2[0] == 0
    assert d[0] <= TOL * max(1, abs(pred[0, 0])) and d[1] <= TOL * max(1, abs(pred[0, 1]))


# ---------------------------------------------------------------- 5. determinism
def test_batch_equals_single_calls_bitwise():
    b = Batch(5, 12, (130, 65, 257))
    mean, var, cov, st = b.run(cov=True)
    covs = _lib.split_cov(cov, b.toffs)
    for c in range(3):
        m1, v1, c1, s1 = b.run([c], cov=True)
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        assert _same(m1, mean[t0:t1]) and _same(v1, var[t0:t1]) and _same(c1, covs[c].ravel()) and s1[0] == st[c]


def test_chunking_does_not_change_results():
    """640 KiB of workspace holds the 257-target cell alone (591 KB with its
    covariance), so the three cells take more than one chunk."""
    b = Batch(5, 12, (130, 65, 257))
    whole = b.run(cov=True)
    _lib.profile_reset()
    parts = b.run(cov=True, pool_bytes=640 * 1024, profile=True)
    chunks = _lib.profile_json()['kernels']['svgp_model']['launches']
    _lib.profile_reset()
    print('chunks', chunks)
    assert chunks >= 2
    assert all(_same(a, c) for a, c in zip(whole, parts))
    with pytest.raises(_lib.OiError, match='liboi error -3'):
        b.run(cov=True, pool_bytes=64 * 1024)


def test_device_inputs_equal_host_inputs():
    import torch
    b = Batch(5, 12, (130, 0, 257))
    host = b.run(cov=True)
    dev = _lib.svgp_predict(b.params, torch.from_numpy(b.XS).cuda(), b.toffs, cov=True, device_inputs=True)
    assert all(_same(a, c) for a, c in zip(host, dev))


def test_position_in_the_target_list_does_not_matter():
    rng = np.random.default_rng(8)
    p = _model(rng, 50)
    xs = _targets(rng, p, 257)
    x0 = np.array([2.5e4, -1.25e5, 3.5])
    first, last = xs.copy(), xs.copy()
    first[0] = x0
    last[-1] = x0
    mf, vf, _, _ = _lib.svgp_predict(p.flat(), first, [0, 257])
    ml, vl, _, _ = _lib.svgp_predict(p.flat(), last, [0, 257])
    assert mf[0] == ml[-1] and vf[0] == vl[-1]
    assert np.array_equal(mf[1:-1], ml[1:-1]) and np.array_equal(vf[1:-1], vl[1:-1])


# ---------------------------------------------------------------- 6. status
def test_nan_lengthscale_fails_its_cell_only():
    b = Batch(6, 12, (70, 130, 5))
    good = b.run(cov=True)
    b.params[1, 0] = np.nan
    mean, var, cov, st = b.run(cov=True)
    assert list(st) == [0, 1, 0]
    covs, gcovs = _lib.split_cov(cov, b.toffs), _lib.split_cov(good[2], b.toffs)
    t0, t1 = b.toffs[1], b.toffs[2]
    assert np.isnan(mean[t0:t1]).all() and np.isnan(var[t0:t1]).all() and np.isnan(covs[1]).all()
    for c in (0, 2):
        m1, v1, c1, s1 = b.run([c], cov=True)
        a0, a1 = b.toffs[c], b.toffs[c + 1]
        assert _same(m1, mean[a0:a1]) and _same(v1, var[a0:a1]) and _same(c1, covs[c].ravel())
        assert _same(covs[c], gcovs[c]) and _same(mean[a0:a1], good[0][a0:a1])
    e, se = _lib.svgp_elbo(b.params, np.concatenate(b.xs), np.zeros(b.toffs[-1]), b.toffs)
    assert list(se) == [0, 1, 0] and np.isnan(e[1]) and np.isfinite(e[[0, 2]]).all()


# ---------------------------------------------------------------- 7. ELBO parity
@pytest.fixture(scope='module')
def elbo_batch():
    """Cells of n in {1, 63, 64, 65, 300, 4600} for each M in {1, 12, 50}, with the
    oracle's ELBO of each."""
    out = {}
    for M in (1, 12, 50):
        rng = np.random.default_rng(700 + M)
        cells = [_cell(rng, n) for n in (1, 63, 64, 65, 300, 4600)]
        ps = [_model(rng, M, x=_cell(rng, 200)[0]) for _ in cells]
        ref = np.array([-O.loss_and_grad(p, x, y, len(y), grad=False) for p, (x, y) in zip(ps, cells)])
        out[M] = (cells, ps, ref)
    return out


@pytest.mark.parametrize('M', [1, 12, 50])
def test_elbo_vs_oracle(elbo_batch, M):
    import torch
    cells, ps, ref = elbo_batch[M]
    X = np.concatenate([c[0] for c in cells])
    Y = np.concatenate([c[1] for c in cells])
    offs = np.cumsum([0] + [len(c[1]) for c in cells])
    e, st = _lib.svgp_elbo(_rows(ps), X, Y, offs)
    rel = np.abs(e - ref) / np.abs(ref)
    print(f'M {M}: elbo rel', rel)
    assert np.all(st == 0)
    assert np.allclose(e, ref, rtol=1e-12, atol=0)
    for c, (p, (x, y)) in enumerate(zip(ps, cells)):
        e1, s1 = _lib.svgp_elbo(p.flat(), x, y, [0, len(y)])
        assert e1[0] == e[c] and s1[0] == 0
    ed, sd = _lib.svgp_elbo(_rows(ps), torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), offs,
                            device_inputs=True)
    assert np.array_equal(ed, e) and np.array_equal(sd, st)
    ec, _ = _lib.svgp_elbo(_rows(ps), X, Y, offs, max_pool=2)  # three chunks
    assert np.array_equal(ec, e)


# ---------------------------------------------------------------- 8. training log
def test_elbo_equals_the_last_training_log_entry():
    """n = B: every minibatch is a permutation of all the data.  With 11
    iterations and log_every = 10 the last log entry is evaluated after the last
    update, so it is the final parameters' ELBO."""
    rng = np.random.default_rng(88)
    x, y = _cell(rng, 100)
    pred, st, params, log = _lib.svgp_batch(x, y, [0, 100], O.notebook_Z(x, 8)[None], [INIT],
                                            [[0.0, 0.0, 4.0]], batch=100, iterations=11, log_every=10,
                                            seed=5, want_params=True)
    e, se = _lib.svgp_elbo(params, x, y, [0, 100])
    print('elbo', e[0], 'log[-1]', log[0, -1], 'rel', abs(e[0] - log[0, -1]) / abs(log[0, -1]))
    assert st[0] == 0 and se[0] == 0 and log.shape == (1, 2)
    assert np.allclose(e[0], log[0, -1], rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 9. device ordinal
def test_bad_device_ordinal_then_a_good_call():
    b = Batch(9, 8, (3,))
    y = np.zeros(3)
    for name, call in (('svgp_predict', lambda **k: b.run(**k)),
                       ('svgp_elbo', lambda **k: _lib.svgp_elbo(b.params, b.XS, y, [0, 3], **k))):
        with pytest.raises(_lib.OiError) as e:
            call(device=99)
        print(name, '->', e.value)
        assert 'bad device ordinal' in str(e.value) and str(e.value).startswith('liboi error -1:'), name
        assert np.all(np.isfinite(call(device=0)[0])), name


# ---------------------------------------------------------------- 10. Python surface
def test_python_surface():
    rng = np.random.default_rng(2)
    x, y = _cell(rng, 600)
    Z = svgp.notebook_Z(x, 20)
    xs = np.array([[0.0, 0.0, 4.0], [1e4, -2e4, 3.0], [-5e4, 7e4, 1.0], [2e5, 2e5, 8.0], [0.0, 0.0, 4.0]])
    kw = dict(lengthscales=[25e3, 25e3, 1], kernel_variance=1, noise_variance=.1, mean=0.3, batchsize=100,
              iterations=60)
    m, v, model = svgp.SVGP(x, y, xs, Z, **kw)
    m1, v1, model1 = svgp.SVGP(x, y, xs[:1], Z, **kw)
    assert m.shape == (5, 1) and v.shape == (5, 1) and m1.shape == (1, 1) and np.all(v > 0)
    assert np.array_equal(model['theta'], model1['theta']) and model['Z'].shape == (20, 3)
    d = (abs(m[0, 0] - m1[0, 0]), abs(v[0, 0] - v1[0, 0]))
    print('SVGP row 0 vs one-target call: mean %.2e var %.2e' % d)
    assert d[0] <= TOL * max(1, abs(m1[0, 0])) and d[1] <= TOL * max(1, abs(v1[0, 0]))
    mf, C = svgp.predict_f(model, xs, full_cov=True)
    assert C.shape == (5, 5) and np.array_equal(mf, m) and np.array_equal(C.diagonal(), v[:, 0])
    my, vy = svgp.predict_y(model, xs)
    assert my.shape == (5, 1) and np.array_equal(my, m) and np.all(vy > v)
    p = O.Params(model['Z'], [1, 1, 1], 1.0, 0.1, 0.0)
    p.set_flat(model['theta'])
    mo, vo = O.predict_f(p, xs)
    assert _err(m[:, 0], mo) <= TOL and _err(v[:, 0], vo) <= TOL
    e = svgp.elbo(model, x, y)
    print('elbo', e)
    assert np.isfinite(e)
