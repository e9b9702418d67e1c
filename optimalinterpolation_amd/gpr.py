"""Reference-shaped Python surface of the hot path, backed by liboi (HIP).

Mirrors ``2021_paper_production/GPR_CS2S3.py`` (``GPR:`` below):

* ``SMLII(hypers, x, y, mX)``  -- GPR:107-141, same arguments / return shapes
  (nlZ shape (1,), dnlZ (6,)), +inf on a non-PD covariance.
* ``GPR3D(index, opt=True)``   -- GPR:143-191, reads the same module globals
  (``X_tree, X, x_train, y_train, t_train, z, radius, mean, T_mid, x0,
  ellXs, sf2xs, sn2xs``) and returns the same 8-tuple / 2-tuple, NaNs on
  failure.
* ``GPR3D_batch(indices, opt=True)`` -- what the per-cell loops GPR:258-261
  and GPR:316-319 become: one call for all of a rank's cells.

All arithmetic runs on the GPU through liboi; the neighbour query (cKDTree,
GPR:159) stays on the host exactly as in the reference.
"""
import numpy as np

from . import _lib

# ---- module globals GPR3D reads (GPR:159-172); the driver assigns them ----
X_tree = None
X = None
x_train = None
y_train = None
t_train = None
z = None
radius = 300            # km (GPR:208)
mean = None             # prior mean (GPR:212)
T_mid = 4               # (GPR:207)
x0 = [np.log(25 * 1000), np.log(25 * 1000), np.log(1.), np.log(1.), np.log(1.), np.log(.1)]  # GPR:217
ellXs = None
sf2xs = None
sn2xs = None

# liboi options used by every call (device, stream, pool size, profiling ...)
options = {}


def SMLII(hypers, x, y, mX):
    """Negative log marginal likelihood and gradient of one cell (GPR:107-141)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    mX = np.broadcast_to(np.asarray(mX, dtype=np.float64), y.shape)
    h = np.asarray(hypers, dtype=np.float64).reshape(1, 6)
    nlz, grad, status = _lib.nlml_grad_batch(x, y, mX, np.array([0, len(y)]), h, **options)
    if status[0] != 0:
        return np.inf, np.ones(6) * np.inf
    return np.array([nlz[0]]), grad[0]


def SMLII_batch(hypers, cells):
    """SMLII for many cells at once: ``cells`` is a synthetic.RaggedCells-like
    object (xyt, z, offs, mean); returns (nlZ [ncell], dnlZ [ncell x 6])."""
    mX = np.full(len(cells.z), cells.mean)
    nlz, grad, _ = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, hypers, **options)
    return nlz, grad


def _neighbours(indices):
    """GPR:159-164 for a list of cell indices -> ragged arrays."""
    ids = [X_tree.query_ball_point(x=X[i, :], r=radius * 1000) for i in indices]
    offs = np.zeros(len(indices) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(i) for i in ids])
    cat = np.concatenate([np.asarray(i, dtype=np.int64) for i in ids]) if ids else np.zeros(0, np.int64)
    xyt = np.stack([x_train[cat], y_train[cat], t_train[cat]], axis=1) if len(cat) else np.zeros((0, 3))
    xs = np.stack([X[indices, 0], X[indices, 1], np.full(len(indices), float(T_mid))], axis=1)
    return xyt, z[cat], offs, xs


_lookup_cache = {'key': None, 'first': None}


def _first_match_rows():
    """GPR:170 ``np.where((X[:,0]==X[index,0]) & (X[:,1]==X[index,1]))`` then
    ``[0]`` (GPR:171): for every cell the FIRST row of ``X`` with the same
    coordinates.  Built once per content of ``X`` (keyed on its bytes) instead
    of once per call, so the reference-style per-cell loop stays O(ncell)."""
    Xa = np.ascontiguousarray(X, dtype=np.float64)
    key = (Xa.shape, hash(Xa.tobytes()))
    if _lookup_cache['key'] != key:
        # rows sorted by (x, y) with ties by index: a group's first row is its first match
        order = np.lexsort((np.arange(len(Xa)), Xa[:, 1], Xa[:, 0]))
        xs, ys = Xa[order, 0], Xa[order, 1]
        new = np.ones(len(order), dtype=bool)
        new[1:] = (xs[1:] != xs[:-1]) | (ys[1:] != ys[:-1])
        grp = np.cumsum(new) - 1
        first = np.empty(len(Xa), dtype=np.int64)
        first[order] = order[new][grp]
        _lookup_cache.update(key=key, first=first)
    return _lookup_cache['first']


def _smoothed_hypers(indices):
    """GPR:170-172: hyper lookup by exact coordinate match (first match)."""
    rows = _first_match_rows()[np.asarray(indices, dtype=np.int64)]
    return np.column_stack([ellXs[rows, 0], ellXs[rows, 1], ellXs[rows, 2], sf2xs[rows], sn2xs[rows]])


def GPR3D_batch(indices, opt=True):
    """GPR3D for every index in one batched GPU call; returns a list of tuples."""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    if len(indices) == 0:
        return []
    xyt, zz, offs, xs = _neighbours(indices)
    if opt:
        out, status, _ = _lib.gpr_batch(xyt, zz, offs, xs, mean, x0=np.asarray(x0, float)[:6],
                                        opt=True, **options)
        return [tuple(np.float64(v) for v in row) for row in out]
    out, status, _ = _lib.gpr_batch(xyt, zz, offs, xs, mean, opt=False,
                                    hyp=_smoothed_hypers(indices), **options)
    return [(np.float64(row[0]), np.float64(row[1])) for row in out]


def GPR3D(index, opt=True):
    """Gaussian Process Regression for one grid cell (GPR:143-191)."""
    return GPR3D_batch([index], opt=opt)[0]


def gpr_cells(cells, opt=True, x0=None, hyp=None, info=False, **kw):
    """Lower-level batched entry on a RaggedCells object (xyt, z, offs, xs, mean)."""
    o = dict(options)
    o.update(kw)
    if x0 is None:
        x0 = globals()['x0']
    return _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean,
                          x0=np.asarray(x0, float)[:6] if opt else None, opt=opt,
                          hyp=hyp, info=info, **o)


def _fit_then(cells, opt, x0, hyp, kw):
    """The four functions below begin so: (the module's options merged with
    ``kw`` for their own liboi call, ``gpr_cells``' out8 and status under the
    caller's ``kw``, the hypers [ncell x 5] to go on with)."""
    o = dict(options)
    o.update(kw)
    out8, status, _ = gpr_cells(cells, opt=opt, x0=x0, hyp=hyp, **kw)
    h = out8[:, 3:8] if opt else np.asarray(hyp, dtype=np.float64).reshape(-1, 5)
    return o, out8, status, h


def gpr_cells_multi(cells, xs, toffs, opt=True, x0=None, hyp=None, cov=False, **kw):
    """Predict every cell of a RaggedCells object at a list of targets of its
    own -- the notebook's ``GPR(x, y, xs, ...)`` with ``xs`` ns x 3 -- with the
    full posterior covariance ``Kxs - v'v`` on request.

    ``xs`` [T x 3] holds the targets of all cells, cell c owning rows
    ``toffs[c]:toffs[c+1]``.  ``opt=True`` fits the hypers exactly as
    ``gpr_cells(opt=True)`` does (one ``oi_gpr_batch`` call, results unchanged)
    and predicts at the fitted hypers; ``opt=False`` predicts at ``hyp``
    [ncell x 5].  Returns ``(fs [T], sd [T], cov_list or None, out8, status)``:
    ``out8`` is what ``gpr_cells`` returns for the cells' own targets
    ``cells.xs`` (fs, sd, lZ, hypers), ``cov_list[c]`` the nt_c x nt_c matrix of
    cell c, ``status[c]`` non-zero where the fit's or the prediction's
    covariance was not positive definite (NaN outputs)."""
    o, out8, status, h = _fit_then(cells, opt, x0, hyp, kw)
    fs, sd, _, cv, st = _lib.gpr_predict_multi(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean,
                                               h, cov=cov, lz=False, **o)
    return fs, sd, (_lib.split_cov(cv, toffs) if cov else None), out8, np.maximum(status, st)


def loo_cells(cells, opt=True, x0=None, hyp=None, **kw):
    """Leave-one-out cross-validation of every cell of a RaggedCells object
    (``oi_gpr_loo``: one factorisation per cell, not one per observation).

    ``opt=True`` fits the hypers exactly as ``gpr_cells(opt=True)`` does (one
    ``oi_gpr_batch`` call, results unchanged) and cross-validates at the fitted
    hypers; ``opt=False`` does so at ``hyp`` [ncell x 5].  Returns ``(mu [N],
    sd [N], lpl [ncell], out8, status)``: ``mu[i]`` / ``sd[i]`` predict
    observation i (noise included) from the other observations of its cell, so
    the standardised residual is ``(cells.z - mu) / sd``; ``lpl`` is the log
    pseudo-likelihood per cell, ``out8`` what ``gpr_cells`` returns, and
    ``status[c]`` the maximum of the fit's and the cross-validation's (non-zero:
    a covariance was not positive definite, NaN outputs)."""
    o, out8, status, h = _fit_then(cells, opt, x0, hyp, kw)
    mu, sd, lpl, st = _lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, h, **o)
    return mu, sd, lpl, out8, np.maximum(status, st)


def lgo_cells(cells, group, opt=True, x0=None, hyp=None, **kw):
    """Leave-group-out cross-validation of every cell of a RaggedCells object
    (``oi_gpr_lgo``: one factorisation per cell, not one per group).

    ``group`` [N] labels every observation (any int64, compared inside a cell
    only): a site (``site_groups``), a pass, a day, a satellite.  The fit is
    exactly ``loo_cells``': ``opt=True`` fits the hypers as ``gpr_cells(opt=True)``
    does and cross-validates at the fitted hypers; ``opt=False`` does so at
    ``hyp`` [ncell x 5].  Returns ``(mu [N], sd [N], lpd [N], d2 [N], lpl [ncell],
    out8, status)``: ``mu[i]`` / ``sd[i]`` predict observation i (noise included)
    from the observations outside its group; ``lpd[i]`` / ``d2[i]`` are the joint
    log density and the squared Mahalanobis distance (chi^2 with g degrees under
    the model) of i's group, repeated for every member; ``lpl`` sums ``lpd`` over
    a cell's groups; ``status[c]`` is the maximum of the fit's and the
    cross-validation's."""
    o, out8, status, h = _fit_then(cells, opt, x0, hyp, kw)
    mu, sd, lpd, d2, lpl, st = _lib.gpr_lgo(cells.xyt, cells.z, cells.offs, group, cells.mean, h, **o)
    return mu, sd, lpd, d2, lpl, out8, np.maximum(status, st)


def sample_cells(cells, xs, toffs, nsamp, opt=True, x0=None, hyp=None, **kw):
    """Joint posterior draws for every cell of a RaggedCells object at its own
    list of targets (``oi_gpr_sample``; ``xs`` [T x 3], cell c owning rows
    toffs[c]:toffs[c+1]).

    The fit is exactly ``loo_cells``': ``opt=True`` fits the hypers as
    ``gpr_cells(opt=True)`` does and draws at the fitted hypers; ``opt=False``
    draws at ``hyp`` [ncell x 5].  ``noise``, ``jitter``, ``seed``, ``streams``
    and ``xi`` go to ``_lib.gpr_sample`` (pass the grid-cell indices as
    ``streams`` so that sharding the cells does not change a draw); the other
    keywords are options.  Returns ``(samples [T x nsamp], fs [T], sd [T],
    out8, status)``: column s of a cell's rows of ``samples`` is one joint
    realisation of the field at the cell's targets, ``fs`` / ``sd`` are
    ``gpr_predict_multi``'s, ``out8`` is what ``gpr_cells`` returns, and
    ``status[c]`` the maximum of the fit's and the draw's."""
    draw = {k: kw.pop(k) for k in ('noise', 'jitter', 'seed', 'streams', 'xi') if k in kw}
    o, out8, status, h = _fit_then(cells, opt, x0, hyp, kw)
    samples, fs, sd, st = _lib.gpr_sample(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, h, nsamp,
                                          **draw, **o)
    return samples, fs, sd, out8, np.maximum(status, st)


def grad_cells(cells, xs, toffs, opt=True, x0=None, hyp=None, **kw):
    """The posterior of the field's gradient for every cell of a RaggedCells
    object at its own list of targets (``oi_gpr_predict_grad``; ``xs`` [T x 3],
    cell c owning rows toffs[c]:toffs[c+1]).

    The fit is exactly ``loo_cells``': ``opt=True`` fits the hypers as
    ``gpr_cells(opt=True)`` does and differentiates at the fitted hypers;
    ``opt=False`` does so at ``hyp`` [ncell x 5].  ``blk`` and ``cov`` go to
    ``_lib.gpr_predict_grad``; the other keywords are options.  Returns ``(grad
    [T x 3], gsd [T x 3], fs [T], sd [T], blk [T x 4 x 4] | None, cov_list |
    None, out8, status)``: ``grad`` / ``gsd`` are the posterior mean and
    standard deviation of (df/dx, df/dy, df/dt) -- the slope in m/m and the
    growth rate in m/day -- ``fs`` / ``sd`` are ``gpr_predict_multi``'s,
    ``cov_list[c]`` the (4 nt_c) x (4 nt_c) joint covariance of cell c (index
    4 t + k), ``out8`` what ``gpr_cells`` returns, and ``status[c]`` the maximum
    of the fit's and the gradient's."""
    want = {k: kw.pop(k) for k in ('blk', 'cov') if k in kw}
    o, out8, status, h = _fit_then(cells, opt, x0, hyp, kw)
    grad, gsd, fs, sd, blk, cv, st = _lib.gpr_predict_grad(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, h,
                                                           **want, **o)
    return (grad, gsd, fs, sd, blk, (_lib.split_jcov(cv, toffs) if cv is not None else None), out8,
            np.maximum(status, st))


def site_groups(xyt, offs):
    """Labels [N] that join the bitwise-equal (x, y, t) rows of a cell -- the
    observations of several satellites binned to one site -- for
    leave-one-site-out through ``lgo_cells``.  A label is the batch row of the
    site's first observation, so it is unique across cells too."""
    xyt = np.ascontiguousarray(xyt, dtype=np.float64).reshape(-1, 3)
    offs = np.asarray(offs, dtype=np.int64).reshape(-1)
    bits = xyt.view(np.int64)    # equal bits, not equal values: -0.0 and 0.0 are two sites, a NaN equals itself
    out = np.empty(len(xyt), dtype=np.int64)
    for a, e in zip(offs[:-1], offs[1:]):
        first = {}
        for i in range(int(a), int(e)):
            out[i] = first.setdefault(bits[i].tobytes(), i)
    return out
