"""GPU parity of ``oi_gpr_sample``: joint posterior draws per cell
(include/oi.h), against tests/sample_ref.py.

Bounds, fixed before any GPU run:
  samples  |gpu - ref| <= 1e-10 * max(sqrt(sf2), |ref|)   (the project's T1 scaled to the draw)
  fs, sd   |gpu - ref| <= 1e-10 * max(1, |ref|), and bit for bit oi_gpr_predict_multi's
  words    bit for bit the reference's Philox4x32-10
on cells whose C = cov + (noise ? sn2 : 0) I + jitter I has cond(C) <= 1e4 in
the reference (asserted for every cell compared; that is why the cells with no
or one observation, whose latent covariance at 63 or more targets has cond 8e4
to 2.4e5, draw their many-target cases with noise or jitter only, and why 200
targets go with 333 observations: with 65 the latent cond is 1.1e4).  The
normals' bound is measured (see K_NORMAL).  Batch mates, chunking, device
inputs, the batch's order and the number of draws must not change a bit of a
cell's results.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, gpr, nystrom, synthetic
import sample_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
HYP = np.array([2e5, 2e5, 6.0, 5e-3, 1e-3])   # the hypers of scripts/loo_timing.py
JITTER = 2e-4
COND_MAX = 1e4
NSAMP = (1, 2, 63, 64, 65, 257)
# (n, nt) of the ragged batch: every n of {0, 1, 65, 333} and every nt of
# {0, 1, 2, 63, 64, 65, 128, 129, 200}
PAIRS = [(0, 2), (1, 1), (1, 0), (65, 63), (333, 64), (65, 65), (333, 128), (65, 129), (333, 200), (65, 128),
         (0, 1), (333, 0)]
# prior and one-observation cells with many targets: drawn with noise or jitter
PAIRS_PRIOR = [(0, 63), (0, 200), (1, 64), (1, 129), (0, 0)]
CONFIGS = {'latent': dict(noise=False, jitter=0.0), 'noise': dict(noise=True, jitter=0.0),
           'jitter': dict(noise=False, jitter=JITTER)}
SEED = 20181205

# The normals' tolerance: err = max over the set of |gpu - longdouble ref| /
# max(1, r) in units of 2^-52 must not exceed K_NORMAL x the same distance for
# numpy's float64 evaluation of the mapping.  K_NORMAL = (err / err64 measured
# on the MI355X, profiles/sample/ratios.json) rounded up to a power of two,
# times 2; a ratio above 256 would be a finding, not a tolerance.  Measured:
# err 2.157, err64 2.127, ratio 1.014 (OI_SAMPLE_RATIOS_OUT=FILE writes the
# measurement of a run to FILE).
K_NORMAL = 4.0


def _lattice(centre, nt, spacing=25e3):
    """nt targets on a square lattice (25 km) centred on ``centre``, at its t."""
    side = int(np.ceil(np.sqrt(max(nt, 1))))
    g = (np.arange(side) - (side - 1) / 2) * spacing
    gx, gy = np.meshgrid(g, g, indexing='ij')
    p = np.stack([centre[0] + gx.ravel(), centre[1] + gy.ravel(), np.full(side * side, centre[2])], axis=1)
    return p[:nt]


def _same(a, b):
    """Bit for bit (NaN equal to NaN)."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def hook_normals(seed, stream, first, count, words=False):
    """The library's own device function: normals [count] (and the words of the blocks touched)."""
    fn = _lib.load().oi_test_sample_normals
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_uint32)]
    out = np.empty(count)
    nb = ((first + count - 1) >> 1) - (first >> 1) + 1 if count else 0
    w = np.zeros((nb, 4), dtype=np.uint32) if words else None
    rc = fn(seed, stream, first, count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if words else None)
    assert rc == 0, _lib.load().oi_last_error()
    return (out, w) if words else out


def cell_doubles(n, nt, nsamp, host=True):
    fn = _lib.load().oi_test_sample_cell_doubles
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int64] * 3 + [ctypes.c_int32]
    return fn(n, nt, nsamp, 2 if host else 0)


class Batch:
    """A ragged batch with a list of targets per cell, its normals and its references."""

    def __init__(self, pairs, seed, hyp=HYP):
        self.pairs = list(pairs)
        self.cells = synthetic.make_cells([n for n, _ in pairs], seed=seed)
        self.mean = self.cells.mean
        tg = [_lattice(self.cells.xs[c], nt) for c, (_, nt) in enumerate(pairs)]
        self.xs = np.ascontiguousarray(np.concatenate(tg))
        self.toffs = np.concatenate([[0], np.cumsum([nt for _, nt in pairs])]).astype(np.int64)
        self.hyp = np.tile(hyp, (len(pairs), 1))
        self.xi = np.random.default_rng(seed + 100).standard_normal((int(self.toffs[-1]), max(NSAMP)))
        self._ref = {}

    def ref(self, config):
        """Per cell (fs, sd, Lc, cond(C)) under a configuration, computed once."""
        if config not in self._ref:
            out = []
            for c in range(len(self.pairs)):
                x, y, _ = self.cells.cell(c)
                t0, t1 = self.toffs[c], self.toffs[c + 1]
                _, fs, sd, C, Lc = R.sample_cell(x, y, self.xs[t0:t1], self.mean, self.hyp[c],
                                                 np.zeros((t1 - t0, 0)), **CONFIGS[config])
                out.append((fs, sd, Lc, np.linalg.cond(C) if len(C) else 1.0))
            self._ref[config] = out
        return self._ref[config]

    def run(self, nsamp, cells=None, hyp=None, **kw):
        """gpr_sample on the whole batch, or on the cells ``cells`` in that order."""
        idx = list(range(len(self.pairs))) if cells is None else list(cells)
        sub = self.cells.subset(idx)
        xs = [self.xs[self.toffs[c]:self.toffs[c + 1]] for c in idx]
        toffs = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.int64)
        if kw.get('xi') is True:
            kw['xi'] = np.ascontiguousarray(np.concatenate(
                [self.xi[self.toffs[c]:self.toffs[c + 1], :nsamp] for c in idx]))
        h = self.hyp if hyp is None else hyp
        return _lib.gpr_sample(sub.xyt, sub.z, sub.offs, np.concatenate(xs), toffs, self.mean, h[idx], nsamp, **kw)

    def cut(self, res, c, toffs=None):
        """Cell c's (samples, fs, sd, status [1]) out of a result over cells with offsets ``toffs``."""
        toffs = self.toffs if toffs is None else toffs
        a, e = toffs[c], toffs[c + 1]
        return res[0][a:e], res[1][a:e], res[2][a:e], res[3][c:c + 1]


@pytest.fixture(scope='module')
def batch():
    return Batch(PAIRS, seed=11)


@pytest.fixture(scope='module')
def prior_batch():
    return Batch(PAIRS_PRIOR, seed=12)


@pytest.fixture(scope='module')
def rng_result(batch):
    """The device generator's draws, 65 per cell, streams = the cells' indices."""
    return batch.run(65, seed=SEED)


def _check_against_ref(b, config, nsamp, res):
    samples, fs, sd, st = res
    assert samples.shape == (b.toffs[-1], nsamp) and not st.any()
    sq = np.sqrt(b.hyp[0, 3])
    worst = 0.0
    for c, (rfs, rsd, Lc, cond) in enumerate(b.ref(config)):
        t0, t1 = b.toffs[c], b.toffs[c + 1]
        assert cond <= COND_MAX, (c, cond)
        want = rfs[:, None] + Lc @ b.xi[t0:t1, :nsamp]
        err = np.abs(samples[t0:t1] - want) / np.maximum(sq, np.abs(want))
        worst = max(worst, err.max(initial=0.0))
        assert np.all(np.abs(fs[t0:t1] - rfs) <= RTOL * np.maximum(1.0, np.abs(rfs))), c
        assert np.all(np.abs(sd[t0:t1] - rsd) <= RTOL * np.maximum(1.0, np.abs(rsd))), c
        assert np.all(err <= RTOL), (c, b.pairs[c], err.max())
    print(f"{config} nsamp {nsamp}: worst |gpu - ref| / max(sqrt(sf2), |ref|) {worst:.3e}")


# ------------------------------------------------------------------ generator

FIRSTS = (0, 1, 2 ** 33 - 3)
COUNTS = (1, 2, 3, 255, 256, 257)


def test_generator_words_are_the_reference_bit_for_bit():
    seed, stream = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    for first in FIRSTS:
        for count in COUNTS:
            _, w = hook_normals(seed, stream, first, count, words=True)
            blocks = np.arange(first >> 1, ((first + count - 1) >> 1) + 1, dtype=np.uint64)
            assert np.array_equal(w.astype(np.uint64), R.block_words(seed, stream, blocks)), (first, count)


def test_generator_normals_within_the_measured_bound():
    sets = [(0x0123456789ABCDEF, 0xFEDCBA9876543210, first, count) for first in FIRSTS for count in COUNTS]
    sets.append((SEED, 3, 0, 121 * 256))
    err = err64 = 0.0
    for seed, stream, first, count in sets:
        z = hook_normals(seed, stream, first, count)
        z64, _ = R.normals(seed, stream, first, count)
        zl, rl = R.normals(seed, stream, first, count, np.longdouble)
        scale = np.maximum(1.0, rl) * np.longdouble(2.0) ** -52
        err = max(err, float(np.max(np.abs(z - zl) / scale)))
        err64 = max(err64, float(np.max(np.abs(z64 - zl) / scale)))
    print(f"normals: err {err:.3f} err64 {err64:.3f} (units of 2^-52), ratio {err / err64:.3f}")
    out = os.environ.get('OI_SAMPLE_RATIOS_OUT')
    if out:
        json.dump({'normals': {'err_ulp52': round(err, 3), 'err64_ulp52': round(err64, 3),
                               'ratio': round(err / err64, 3), 'elements': int(sum(s[3] for s in sets))}},
                  open(out, 'w'), indent=1)
    assert err <= K_NORMAL * err64


def test_rng_mode_equals_given_xi_fed_the_hooks_normals(batch, rng_result):
    xi = np.concatenate([hook_normals(SEED, c, 0, nt * 65).reshape(65, nt).T for c, (_, nt) in enumerate(batch.pairs)])
    assert _same(batch.run(65, xi=np.ascontiguousarray(xi)), rng_result)
    # and the hook's normals are the reference's to the generator's bound: a stream's draws are the mapping's
    c = PAIRS.index((65, 129))
    z64, r = R.normals(SEED, c, 0, 129 * 65)
    blk = xi[batch.toffs[c]:batch.toffs[c + 1]]
    assert np.max(np.abs(blk - z64.reshape(65, 129).T)) <= 16 * K_NORMAL * 2.0 ** -52 * max(1.0, r.max())


# ------------------------------------------------- given Xi, against the reference

@pytest.mark.parametrize('config', list(CONFIGS))
@pytest.mark.parametrize('nsamp', NSAMP)
def test_given_xi_against_reference(batch, config, nsamp):
    _check_against_ref(batch, config, nsamp, batch.run(nsamp, xi=True, **CONFIGS[config]))


@pytest.mark.parametrize('config', ['noise', 'jitter'])
def test_prior_and_single_observation_cells_with_many_targets(prior_batch, config):
    _check_against_ref(prior_batch, config, 65, prior_batch.run(65, xi=True, **CONFIGS[config]))


def test_latent_condition_numbers_are_what_the_bound_assumes(batch):
    conds = [r[3] for r, (n, nt) in zip(batch.ref('latent'), PAIRS) if nt >= 63]
    print('latent cond(C):', ' '.join(f'{v:.1e}' for v in conds))
    assert max(conds) <= COND_MAX and min(conds) >= 1e2   # not trivially conditioned either


# ---------------------------------------------------------------------- bitwise

def test_fs_sd_are_predict_multis(batch, rng_result):
    fs, sd, _, _, st = _lib.gpr_predict_multi(batch.cells.xyt, batch.cells.z, batch.cells.offs, batch.xs, batch.toffs,
                                              batch.mean, batch.hyp, lz=False)
    assert not st.any() and _same((fs, sd), rng_result[1:3])
    for config in ('noise', 'jitter'):
        res = batch.run(2, seed=1, **CONFIGS[config])
        assert _same((fs, sd), res[1:3]) and not res[3].any()


def test_batch_equals_single_cells(batch, rng_result):
    given = batch.run(65, xi=True)
    for c in range(len(PAIRS)):
        one = batch.run(65, cells=[c], seed=SEED, streams=[c])
        assert _same(one, batch.cut(rng_result, c)), c
        assert _same(batch.run(65, cells=[c], xi=True), batch.cut(given, c)), c


def test_chunking_is_bitwise_neutral(batch, rng_result):
    pool = 8 * (11 * 32 + max(cell_doubles(n, nt, 65) for n, nt in PAIRS))   # the largest cell and the chunk's slack
    _lib.profile_reset()
    res = batch.run(65, seed=SEED, pool_bytes=pool, profile=True)
    prof = _lib.profile_json()['kernels']
    _lib.profile_reset()
    assert {'ps_generate', 'ps_cholesky', 'ps_solve', 'ps_reduce', 'ps_cov', 'ps_factor', 'ps_normals',
            'ps_product'} <= set(prof)
    assert prof['ps_product']['launches'] >= 4, prof['ps_product']
    assert _same(res, rng_result)
    assert _same(batch.run(65, seed=SEED, max_pool=1), rng_result)
    with pytest.raises(_lib.OiError, match=r"error -3: a cell's sampling workspace does not fit pool_bytes"):
        batch.run(65, seed=SEED, pool_bytes=pool - 8)


def test_device_inputs_equal_host_inputs(batch, rng_result):
    import torch
    x = torch.from_numpy(batch.cells.xyt).to('cuda:0')
    z = torch.from_numpy(batch.cells.z).to('cuda:0')
    res = _lib.gpr_sample_device(x, z, batch.cells.offs, batch.xs, batch.toffs, batch.mean, batch.hyp, 65,
                                 seed=SEED, device=0)
    assert _same(res, rng_result)


def test_first_columns_of_a_longer_call(batch, rng_result):
    longer = batch.run(257, seed=SEED)
    assert _same((longer[0][:, :65], longer[1], longer[2], longer[3]), rng_result)
    one = batch.run(1, seed=SEED)
    assert _same((longer[0][:, :1],), (one[0],))
    none = batch.run(0, seed=SEED)
    assert none[0].shape == (batch.toffs[-1], 0) and _same(none[1:], rng_result[1:])


def test_permuting_or_subsetting_keeps_a_cells_draws(batch, rng_result):
    for idx in ([9, 3, 0, 11, 8, 2, 5], [8], list(reversed(range(len(PAIRS))))):
        res = batch.run(65, cells=idx, seed=SEED, streams=idx)
        toffs = np.concatenate([[0], np.cumsum([PAIRS[c][1] for c in idx])])
        for q, c in enumerate(idx):
            assert _same(batch.cut(res, q, toffs), batch.cut(rng_result, c)), (idx, c)
    # another stream or another seed is another draw
    c = PAIRS.index((65, 63))
    assert not np.array_equal(batch.run(65, cells=[c], seed=SEED, streams=[c + 1])[0], batch.cut(rng_result, c)[0])
    assert not np.array_equal(batch.run(65, cells=[c], seed=SEED + 1, streams=[c])[0], batch.cut(rng_result, c)[0])


def test_default_streams_are_the_cells_indices(batch, rng_result):
    assert _same(batch.run(65, seed=SEED, streams=np.arange(len(PAIRS))), rng_result)
    big = 2 ** 64 - 1 - np.arange(len(PAIRS), dtype=np.uint64)   # all 64 bits of a stream id arrive
    res = batch.run(65, seed=SEED, streams=big)
    c = PAIRS.index((333, 64))
    xi = hook_normals(SEED, int(big[c]), 0, 64 * 65).reshape(65, 64).T
    assert _same(batch.run(65, cells=[c], xi=np.ascontiguousarray(xi)), batch.cut(res, c))


def test_rng_draws_have_the_posterior_as_their_map(batch, rng_result):
    """The RNG mode against the reference end to end: the reference's float64
    normals through the reference's factor."""
    ref = batch.ref('latent')
    sq = np.sqrt(HYP[3])
    for c, (n, nt) in enumerate(PAIRS):
        if nt == 0:
            continue
        want = ref[c][0][:, None] + ref[c][2] @ R.cell_xi(SEED, c, nt, 65)
        got = batch.cut(rng_result, c)[0]
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(sq, np.abs(want))), c


# ----------------------------------------------------------------------- status

def _with_cell(batch, k, hyp_row):
    """The batch with cell k repeated in front of itself at other hypers: (cells, hyp)."""
    idx = list(range(k)) + [k] + list(range(k, len(PAIRS)))
    return idx, np.concatenate([batch.hyp[:k], hyp_row[None], batch.hyp[k:]])


def _mates(batch, res, idx, k, rng_result):
    toffs = np.concatenate([[0], np.cumsum([PAIRS[c][1] for c in idx])])
    for q, c in enumerate(idx):
        if q != k:
            assert _same(batch.cut(res, q, toffs), batch.cut(rng_result, c)), c
    return batch.cut(res, k, toffs)


def _run_with(batch, idx, hyp, **kw):
    sub = batch.cells.subset(idx)
    xs = [batch.xs[batch.toffs[c]:batch.toffs[c + 1]] for c in idx]
    toffs = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.int64)
    return _lib.gpr_sample(sub.xyt, sub.z, sub.offs, np.concatenate(xs), toffs, batch.mean, hyp, 65, seed=SEED,
                           streams=idx, **kw)


def test_failed_cell_is_nan_and_mates_unchanged(batch, rng_result):
    k = PAIRS.index((333, 128))
    bad = HYP.copy()
    bad[4] = -2.0 * bad[3]  # first pivot sf2 + sn2 <= 0
    x, y, _ = batch.cells.cell(k)
    with pytest.raises(np.linalg.LinAlgError):
        R.posterior(x, y, batch.xs[batch.toffs[k]:batch.toffs[k + 1]], batch.mean, bad)
    idx, hyp = _with_cell(batch, k, bad)
    res = _run_with(batch, idx, hyp)
    assert res[3][k] == 1 and res[3].sum() == 1
    samples, fs, sd, _ = _mates(batch, res, idx, k, rng_result)
    assert samples.shape == (128, 65) and np.isnan(samples).all() and np.isnan(fs).all() and np.isnan(sd).all()


def test_singular_covariance_is_status_2_and_noise_cures_it(batch, rng_result):
    k = PAIRS.index((65, 129))
    flat = HYP.copy()
    flat[3] = 0.0   # sf2 = 0: cov is exactly 0
    idx, hyp = _with_cell(batch, k, flat)
    res = _run_with(batch, idx, hyp)
    assert res[3][k] == 2 and res[3].sum() == 2
    samples, fs, sd, _ = _mates(batch, res, idx, k, rng_result)
    assert np.isnan(samples).all() and samples.shape == (129, 65)
    sub = batch.cells.subset(idx)
    toffs = np.concatenate([[0], np.cumsum([PAIRS[c][1] for c in idx])])
    xs = np.concatenate([batch.xs[batch.toffs[c]:batch.toffs[c + 1]] for c in idx])
    pfs, psd, _, _, pst = _lib.gpr_predict_multi(sub.xyt, sub.z, sub.offs, xs, toffs, batch.mean, hyp, lz=False)
    assert pst[k] == 0 and _same((fs, sd), (pfs[toffs[k]:toffs[k + 1]], psd[toffs[k]:toffs[k + 1]]))
    assert np.array_equal(fs, np.full(129, batch.mean)) and np.array_equal(sd, np.zeros(129))
    # a new observation of the same cell: C = sn2 I
    noisy = _run_with(batch, idx, hyp, noise=True)
    assert not noisy[3].any()
    nref = batch.run(65, seed=SEED, noise=True)
    toffs = np.concatenate([[0], np.cumsum([PAIRS[c][1] for c in idx])])
    for q, c in enumerate(idx):
        if q != k:
            assert _same(batch.cut(noisy, q, toffs), batch.cut(nref, c)), c
    got = batch.cut(noisy, k, toffs)[0]
    want = batch.mean + np.sqrt(flat[4]) * R.cell_xi(SEED, k, 129, 65)
    assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.sqrt(flat[3]), np.abs(want)))


# ---------------------------------------------------------------------- surface

def test_sample_cells_and_gpr_sample_surface():
    d = load_golden('gpr3d.npz')
    cells = synthetic.RaggedCells(d['x'], d['y'], d['offs'], d['xs'], float(d['mean'])).subset([5, 6, 7])
    xs = np.concatenate([_lattice(cells.xs[c], 9) for c in range(3)])
    toffs = np.array([0, 9, 18, 27])
    ref8, rst, _ = gpr.gpr_cells(cells, opt=True, x0=O.X0_PRODUCTION)
    samples, fs, sd, out8, st = gpr.sample_cells(cells, xs, toffs, 7, opt=True, x0=O.X0_PRODUCTION, seed=3,
                                                 streams=[40, 41, 42])
    assert np.array_equal(out8, ref8) and not st.any() and not rst.any()
    direct = _lib.gpr_sample(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, out8[:, 3:8], 7, seed=3,
                             streams=[40, 41, 42])
    assert samples.shape == (27, 7) and fs.shape == sd.shape == (27,)
    assert _same((samples, fs, sd), direct[:3]) and np.isfinite(samples).all()
    fixed = gpr.sample_cells(cells, xs, toffs, 7, opt=False, hyp=out8[:, 3:8], seed=3, streams=[40, 41, 42])
    assert _same(fixed[:3], direct[:3])
    # the notebook-style single cell: residual outputs in, the mean added back
    x, z, _ = cells.cell(1)
    h = out8[1, 3:8]
    s1, f1, d1 = nystrom.GPR_sample(x, z - cells.mean, xs[9:18], list(h[:3]), h[3], h[4], cells.mean, 7, seed=3)
    one = _lib.gpr_sample(x, z - cells.mean, [0, len(z)], xs[9:18], [0, 9], 0.0, h[None], 7, seed=3)
    assert s1.shape == (9, 7) and _same((s1, f1, d1), (cells.mean + one[0], cells.mean + one[1], one[2]))
    g1, gs = nystrom.GPR(x, z - cells.mean, xs[9:18], list(h[:3]), h[3], h[4], cells.mean)
    assert _same((f1, d1), (g1, gs))
    noisy = nystrom.GPR_sample(x, z - cells.mean, xs[9:18], list(h[:3]), h[3], h[4], cells.mean, 7, seed=3, noise=True)
    assert not np.array_equal(noisy[0], s1) and _same(noisy[1:], (f1, d1))
    bad = h.copy()
    bad[4] = -2.0 * bad[3]
    with pytest.raises(np.linalg.LinAlgError):
        nystrom.GPR_sample(x, z - cells.mean, xs[9:18], list(bad[:3]), bad[3], bad[4], cells.mean, 7)
