"""Shared cases for the edge tests of the Nystrom variant
(tests/test_nystrom_oracle_edges.py on the CPU, tests/test_gpu_nystrom_edges.py
on the GPU): seeded cells on DISTINCT sites, the three hyper sets, the edge
shapes, the float64 oracle per cell (computed once and cached) and the bars of
tests/test_gpu_nystrom.py.  A plain module (tests import it), not a conftest;
it holds no test and reads nothing but the seeds below.

Why distinct sites: a repeated site among the inducing rows makes K_mm exactly
singular, and the notebook's ``s[s <= 0] = 1e-12`` clamp is then taken or not
according to the sign of a rounding-level eigenvalue -- in numpy itself, so the
reference is not a function of its inputs there.  Every cell here draws its n
rows WITHOUT replacement from a 9 x 9 x 9 lattice.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nystrom_oracle as N  # noqa: E402
from oracle.gp_oracle import matern32  # noqa: E402

# 729 sites: {-4..4} * 25 km  x  {-4..4} * 25 km  x  {0..8} days
_G = np.arange(-4, 5) * 25e3
LATTICE = np.array([(a, b, t) for a in _G for b in _G for t in range(9)], dtype=np.float64)
XS = np.array([[0.0, 0.0, 4.0]])   # the prediction target
MEAN = 0.28                        # the prior mean added back by GPR

# log-hypers (ell_x, ell_y, ell_t, sf2, sn2)
H1 = np.log([2.5e4, 2.5e4, 1.0, 1.0, 0.1])      # nystrom.default_x0()
H2 = np.log([6e4, 9e4, 3.0, 6e-3, 3e-3])        # the notebook-size test's hypers
H3 = np.log([1e-3, 1e-3, 1e-3, 1.0, 0.1])       # K = sf2 I exactly: an M-fold eigenvalue cluster
HYPERS = {'H1': H1, 'H2': H2, 'H3': H3}

# (n, M): M = 1 and M = n; n < 64; n = 65, 128, 129 (tile decode, blocks(n, 64));
# M in 65..128 (two k-tiles, two diagonal-block inverses); M = 32, 64, 96, 128
# (own padded size) beside M = 31, 33, 63, 65, 129
EDGE_SHAPES = ((1, 1), (2, 1), (2, 2), (5, 5), (33, 32), (40, 33), (63, 63), (64, 64), (65, 1), (65, 64),
               (65, 65), (70, 31), (127, 64), (128, 128), (129, 65), (130, 129), (193, 96))

# bars of tests/test_gpu_nystrom.py: |got - ref| <= bar * scale with scale =
# max(1, |ref|), for the gradient max(1, max |grad_ref|)
BARS = {'nlz': 1e-10, 'grad': 1e-10, 'fs': 1e-10, 'sd': 1e-9, 'sprior': 1e-10}
QUANTITIES = tuple(BARS)


def cell_seed(n, M):
    return 1000 * n + M


def _draw(rng, n):
    return LATTICE[rng.choice(len(LATTICE), n, replace=False)]


def sites(n, seed):
    """n distinct rows of LATTICE, drawn by default_rng(seed)."""
    return _draw(np.random.default_rng(seed), n)


def cell(n, seed):
    """(x [n x 3], y [n]): x = sites(n, seed) and, from the same generator,
    y = 0.05 sin(x / 2e5) + 0.01 (t - 4) + N(0, 0.02)."""
    rng = np.random.default_rng(seed)
    x = _draw(rng, n)
    y = 0.05 * np.sin(x[:, 0] / 2e5) + 0.01 * (x[:, 2] - 4) + rng.normal(0, 0.02, n)
    return x, y


def oracle_cell(h, x, y, M):
    """(nlz, grad [5], fs, sd, sprior) of oracle/nystrom_oracle.py at log-hypers
    h, target XS and mean MEAN; inducing rows N.inducing_indices(n, M), which
    is what nystrom._ragged_sel draws."""
    h = np.asarray(h, dtype=np.float64)
    ell, sf2, sn2 = list(np.exp(h[:3])), np.exp(h[3]), np.exp(h[4])
    with np.errstate(all='ignore'):
        f, g = N.neg_log_ml(h, x, y, M)
        fs, sd, sp = N.predict(x, y, XS, ell, sf2, sn2, MEAN, M)
    return (float(np.asarray(f).item()), np.asarray(g, dtype=np.float64), float(np.asarray(fs).item()),
            float(np.asarray(sd).item()), float(sp))


def sd_margin(h, x, y, M):
    """(sf2 - k*' Ki k*) / sf2 in the oracle: the argument of sd's square root,
    relative to sf2."""
    h = np.asarray(h, dtype=np.float64)
    ell, sf2, sn2 = list(np.exp(h[:3])), np.exp(h[3]), np.exp(h[4])
    k = matern32(x, ell, sf2, xs=XS)
    Ki, _ = N.nystroem(x, y, M=M, ell=ell, sf2=sf2, sn2=sn2)
    return float((sf2 - np.linalg.multi_dot([k.T, Ki, k]).item()) / sf2)


class Case:
    """One cell of a batch: n rows (seeded), M inducing rows, log-hypers h.
    ``x`` may be replaced (a NaN coordinate) before the batch is assembled."""

    def __init__(self, n, M, h, seed=None):
        self.n, self.M, self.h = int(n), int(M), np.asarray(h, dtype=np.float64)
        self.seed = cell_seed(n, M) if seed is None else seed
        self.x, self.y = cell(self.n, self.seed)
        self.sel = N.inducing_indices(self.n, self.M)
        self.clean = True

    def with_nan(self, row, col=0):
        c = Case(self.n, self.M, self.h, self.seed)
        c.x = c.x.copy()
        c.x[row, col] = np.nan
        c.clean = False
        return c

    @property
    def key(self):
        return (self.n, self.M, self.seed, self.h.tobytes())

    def __repr__(self):
        return f"(n={self.n}, M={self.M})"


_ORACLE = {}   # clean cases only: key -> (reference, sd margin)


def reference(case):
    """oracle_cell of a case, computed once per (n, M, seed, h)."""
    if not case.clean:
        return oracle_cell(case.h, case.x, case.y, case.M)
    if case.key not in _ORACLE:
        _ORACLE[case.key] = (oracle_cell(case.h, case.x, case.y, case.M),
                             sd_margin(case.h, case.x, case.y, case.M))
    return _ORACLE[case.key][0]


def screen(cases):
    """Every GPU test passes its clean cases through here.  Raises when a case
    has |sf2 - err| < 1e-6 sf2 in the oracle: whether its sd is a number or NaN
    then hangs on rounding, so the case has to be replaced by another seed --
    never dropped."""
    for c in cases:
        if not c.clean:
            continue
        reference(c)
        m = _ORACLE[c.key][1]
        if not abs(m) >= 1e-6:
            raise AssertionError(f"case {c} seed {c.seed}: (sf2 - err) / sf2 = {m:.3g}: the sign of sd's "
                                 "argument is not decidable; choose another seed")
    return cases


def edge_cases(h):
    """EDGE_SHAPES in an order that is NOT sorted by M (the list reversed and
    interleaved front / back), all at log-hypers h."""
    s = list(EDGE_SHAPES)[::-1]
    order = [s[i // 2] if i % 2 == 0 else s[len(s) - 1 - i // 2] for i in range(len(s))]
    assert sorted(order) == sorted(EDGE_SHAPES)
    Ms = [M for _, M in order]
    assert Ms != sorted(Ms)
    return [Case(n, M, h) for n, M in order]


def chunk_cases(ncell=130, seed=64):
    """More cells than a Runner's 64-cell chunk: n from 5..70, M from 1..n (so
    the M-sort reorders them across the chunks), H1 and H2 alternately."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(ncell):
        n = int(rng.integers(5, 71))
        M = int(rng.integers(1, n + 1))
        out.append(Case(n, M, H1 if k % 2 == 0 else H2, seed=7000 + k))
    return out


# The fit cells.  Seed cell_seed(n, M) + 100000 s, with s chosen on the CPU from
# s = 1..12 as the first of those with the most scipy iterations among the
# seeds that (a) pass fit_screen and (b) keep scipy's (nit, status) in six runs
# with independent relative noise of 1e-11 on every f and g -- an order above
# the oracle's own error against mpmath along such a path (<= 1.4e-12 in the
# gradient near the optimum, where K_mm has lambda_min / lambda_max ~ 2e-5).
# (b) matters: with the plain seed, (65,65) passes (a) at (27, 2) but noise of
# 1e-12 already gives (26, 2) or (30, 1) in six of eight runs, so scipy's path
# there is not decided by the reference to its own accuracy.  Every fit ends
# with status 2 (precision loss in the line search): the notebook's gradient
# doubles components 3 and 4, so it is not the gradient of nlZ and CG never
# meets gtol.
FIT_SHAPES = ((70, 31), (65, 65), (129, 65), (40, 33), (5, 5))
FIT_SEED_STEP = {(70, 31): 2, (65, 65): 8, (129, 65): 4, (40, 33): 2, (5, 5): 12}
FIT_MAXITER = 30


def fit_cases():
    """The cells of the fit tests; h is the start point nystrom.default_x0() = H1."""
    return [Case(n, M, H1, seed=cell_seed(n, M) + 100000 * FIT_SEED_STEP[n, M]) for n, M in FIT_SHAPES]


_FITS = {}


def scipy_fit(case, scale=1.0, maxiter=FIT_MAXITER):
    """scipy's minimize(method='CG', jac=True) from case.h on the oracle
    objective with f and g multiplied by ``scale``."""
    import scipy.optimize
    key = (case.key, scale, maxiter)
    if key not in _FITS:
        def f(h):
            with np.errstate(all='ignore'):
                a, b = N.neg_log_ml(h, case.x, case.y, case.M)
            return scale * float(np.asarray(a).item()), scale * b
        _FITS[key] = scipy.optimize.minimize(f, x0=case.h, method='CG', jac=True, options={'maxiter': maxiter})
    return _FITS[key]


def fit_screen(case, maxiter=FIT_MAXITER):
    """(scipy's result, admitted): a cell is admitted to the comparison with
    scipy only if nit and status do not move when the oracle's f and g are
    scaled by 1 +- 1e-13 -- otherwise a line search or the stop test sits on a
    rounding-level tie and the reference's own path is not decidable."""
    r = scipy_fit(case, 1.0, maxiter)
    same = all((q.nit, q.status) == (r.nit, r.status)
               for q in (scipy_fit(case, 1.0 + 1e-13, maxiter), scipy_fit(case, 1.0 - 1e-13, maxiter)))
    return r, same


class Batch:
    """The arguments of _lib.nystrom_batch / nystrom_fit_batch for a list of cases."""

    def __init__(self, cases, sel=None):
        self.cases = list(cases)
        self.xyt = np.concatenate([c.x for c in self.cases])
        self.y = np.concatenate([c.y for c in self.cases])
        self.offs = np.concatenate([[0], np.cumsum([c.n for c in self.cases])]).astype(np.int64)
        sels = [c.sel for c in self.cases] if sel is None else sel
        self.sel = np.concatenate(sels).astype(np.int64)
        self.soffs = np.concatenate([[0], np.cumsum([len(s) for s in sels])]).astype(np.int64)
        self.hyp = np.exp(np.stack([c.h for c in self.cases]))     # LINEAR hypers
        self.xs = np.repeat(XS, len(self.cases), axis=0)


def cell_errors(got, ref):
    """{quantity: |got - ref| / scale} on the scales of tests/test_gpu_nystrom.py
    (max(1, |ref|); the gradient's max(1, max |grad_ref|)).  ``got`` and ``ref``
    are (nlz, grad, fs, sd, sprior); entries of ``got`` may be None (not
    computed).  sd must be NaN exactly where the reference's is (then its
    error is 0); every other quantity must be finite where the reference is."""
    out = {}
    for name, g, r in zip(QUANTITIES, got, ref):
        if g is None:
            continue
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        if name == 'sd' and np.isnan(r):
            assert np.isnan(g), f"sd = {g} where the reference is NaN"
            out[name] = 0.0
            continue
        assert np.isfinite(r).all(), f"{name}: reference not finite ({r})"
        assert np.isfinite(g).all(), f"{name} = {g} where the reference is {r}"
        out[name] = float(np.max(np.abs(g - r)) / max(1.0, float(np.max(np.abs(r)))))
    return out


def assert_cell(got, ref, k, bars=BARS):
    """The bars of tests/test_gpu_nystrom.py on one cell; ``k`` names it in the
    message.  Returns {quantity: error / bar}."""
    try:
        err = cell_errors(got, ref)
    except AssertionError as e:
        raise AssertionError(f"cell {k}: {e}") from None
    for name, e in err.items():
        assert e <= bars[name], f"cell {k}: {name} error {e:.3g} above {bars[name]:g} (got {got}, ref {ref})"
    return {name: e / bars[name] for name, e in err.items()}


class Worst:
    """Keeps the worst error / bar ratio per quantity and where it occurred."""

    def __init__(self):
        self.w = {}

    def add(self, ratios, where):
        for name, r in ratios.items():
            if name not in self.w or r > self.w[name][0]:
                self.w[name] = (r, where)

    def report(self, title):
        print(title + ': ' + ', '.join(f"{q} {self.w[q][0]:.3g} at {self.w[q][1]}" for q in QUANTITIES
                                       if q in self.w))
