"""Bitwise A/B of two builds of liboi.so on the same inputs (a refactor that
must not change a single bit).  One small case per entry family:
  main engine   objective + gradient at fixed hypers on cells from n = 1 to
                3000 (every tile-boundary class), predict at FIXED_HYPERS, and
                full opt=True fits of a few day cells
  Nystrom       objective + predict, the one-shot fit and a session (two
                batches) on cells that cross the pad quantum 32 and the 64-tile
                in n and M; the one-shot fit in three and in two groups and a
                session with two cells per group, profiled, on seven unequal
                cells: their nys_* stage names and launch counts
  prediction    gpr_predict_multi with the covariance, n and nt around the
                64-tile, in one chunk and in several
  leave-one-out gpr_loo with lpl, n around the 64-tile, in one chunk and in several
  leave-group-out gpr_lgo with lpd, d2 and lpl, n around the 64-tile under four
                labellings (singletons, a group across the tile boundary, one
                whole-cell group, interleaved), in one chunk, in several and on
                device tensors
  sampling      gpr_sample at nt around the 64-tile and 0, 1 and 3 draws: the
                device generator with given and with default streams, the
                caller's normals, noise, jitter, a covariance that does not
                factor (status 2); in one chunk and in several
  Nystrom multi nystrom_predict_multi without and with the covariance, n, M and
                nt around the 64-tile
  SVGP          a short Adam run with logging; predict_f with the covariance
                and the ELBO at its parameters, in one chunk and in several
  device inputs the Nystrom fit and the SVGP run again on device tensors
  day helpers   smooth_fields, ball query + gather
  profile       stage names and launch counts of the staged paths; the main
                engine's kernels with their launch counts and counted flops
Usage (GPU box):
    python tools/ab_bitwise.py run OUT.npz        # with OI_LIB set as wanted
    python tools/ab_bitwise.py cmp A.npz B.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _engine(_lib, synthetic):
    sizes = [1, 2, 40, 63, 64, 65, 128, 129, 200, 257, 333, 700, 1100, 1600, 2300, 3000]
    cells = synthetic.make_cells(sizes, seed=77)
    h = np.tile(np.array([np.log(2e5), np.log(2.5e5), np.log(7.), np.log(4e-3), np.log(1e-3), 0.]), (len(sizes), 1))
    nlz, grad, st = _lib.nlml_grad_batch(cells.xyt, cells.z, np.full(len(cells.z), cells.mean), cells.offs, h)
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    pred, pst, _ = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
    # the same two calls profiled: the engine's launch counts and its executed-flop
    # accounting per kernel (entries never launched are left out)
    _lib.profile_reset()
    _lib.nlml_grad_batch(cells.xyt, cells.z, np.full(len(cells.z), cells.mean), cells.offs, h, profile=True)
    _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp, profile=True)
    k = _lib.profile_json()['kernels']
    names = sorted(n for n in k if n.startswith('k_') and k[n]['launches'] > 0)
    prof = dict(eng_kernel_names=np.array(names),
                eng_kernel_launches=np.array([k[n]['launches'] for n in names], dtype=np.int64),
                eng_kernel_flops=np.array([k[n]['flops'] for n in names], dtype=np.float64))
    day = synthetic.make_day(seed=0, max_cells=40)
    fit, fst, info = _lib.gpr_batch(day.xyt, day.z, day.offs, day.xs, day.mean,
                                    x0=np.array([np.log(25e3), np.log(25e3), 0, 0, 0, np.log(.1)]), opt=True, info=True)
    return dict(nlz=nlz, grad=grad, st=st, pred=pred, pst=pst, fit=fit, fst=fst, info=info, **prof)


def _stages(_lib, prefix):
    """Sorted stage names and launches of the stages called `prefix`* (no times)."""
    k = _lib.profile_json()['kernels']
    names = sorted(n for n in k if n.startswith(prefix))
    return np.array(names), np.array([k[n]['launches'] for n in names], dtype=np.int64)


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _nystrom(_lib, synthetic):
    from optimalinterpolation_amd import nystrom
    ns, Ms = [70, 130, 200, 260], np.array([20, 33, 64, 65])
    c = synthetic.make_cells(ns, seed=5)
    y = c.z - c.mean
    sel, soffs = nystrom._ragged_sel(c.offs, Ms)
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(ns), 1))
    args = (c.xyt, y, c.offs, sel, soffs, hyp)
    nlz, grad, pred, st = _lib.nystrom_batch(*args, xs=c.xs, mean=c.mean)
    _lib.profile_reset()
    _lib.nystrom_batch(*args, xs=c.xs, mean=c.mean, profile=True)
    names, launches = _stages(_lib, 'nys_')
    x0 = nystrom.default_x0()
    fit, fst, finfo = _lib.nystrom_fit_batch(c.xyt, y, c.offs, sel, soffs, x0, c.xs, c.mean, maxiter=100)
    dfit = _lib.nystrom_fit_batch(*_cuda(c.xyt, y), c.offs, sel, soffs, x0, c.xs, c.mean, maxiter=100,
                                  device_inputs=True)
    with _lib.NystromSession(maxiter=100) as s:
        t = []
        for a, b in [(0, 2), (2, 4)]:
            po = c.offs[a:b + 1] - c.offs[a]
            ps, pso = nystrom._ragged_sel(po, Ms[a:b])
            t.append(s.submit(c.xyt[c.offs[a]:c.offs[b]], y[c.offs[a]:c.offs[b]], po, ps, pso, x0, c.xs[a:b], c.mean))
        res = [s.wait(k) for k in t]
    prof = _nystrom_fit_profiled(_lib, synthetic, nystrom)
    return dict(prof, nys_nlz=nlz, nys_grad=grad, nys_pred=pred, nys_st=st, nys_stage_names=names,
                nys_stage_launches=launches, nys_fit=fit, nys_fit_st=fst, nys_fit_info=finfo,
                nys_ses=np.concatenate([r[0] for r in res]), nys_ses_st=np.concatenate([r[1] for r in res]),
                nys_ses_info=np.concatenate([r[2] for r in res]),
                nys_dev_fit=dfit[0], nys_dev_fit_st=dfit[1], nys_dev_fit_info=dfit[2])


def _nystrom_fit_profiled(_lib, synthetic, nystrom):
    """The fit's scheduling: results are the same under any grouping of the
    cells, so what shows that the groups hold the same cells in the same rounds
    is the nys_* launch counts (the batched factorisations are launched once
    per run of equal padded M within a round).  Seven unequal cells: a one-shot
    fit in three groups (3, 2, 2 cells) and the default two, and a session of
    two tickets whose groups hold two cells each.

    Cells 0..6 have padded M 32, 64, 64, 96, 64, 32, 32.  In three groups cell
    c belongs to group c mod 3: group 1 is cells {1, 4} (both 64: one batched
    factorisation per round) and group 2 is cells {2, 5} (64 and 32: two).  A
    loop that let group 1 take cell 2 from the queue would make them {1, 4, 2}
    and {5}, one factorisation each, and the counts would show it.  The two
    knobs are set here and put back as the caller had them."""
    ns, Ms = [70, 130, 200, 260, 90, 150, 100], np.array([20, 33, 64, 65, 40, 31, 32])
    c = synthetic.make_cells(ns, seed=6)
    y = c.z - c.mean
    sel, soffs = nystrom._ragged_sel(c.offs, Ms)
    x0 = nystrom.default_x0()
    r = {}

    knobs = ('OI_NYS_GROUPS', 'OI_NYS_CAP')
    saved = {k: os.environ[k] for k in knobs if k in os.environ}

    def env(**kw):
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(kw)
    for tag, kw in (('g3', dict(OI_NYS_GROUPS='3')), ('g2', {})):
        env(**kw)
        _lib.profile_reset()
        fit = _lib.nystrom_fit_batch(c.xyt, y, c.offs, sel, soffs, x0, c.xs, c.mean, maxiter=30, profile=True)
        names, launches = _stages(_lib, 'nys_')
        r.update({f'nysp_fit_{tag}': fit[0], f'nysp_fit_{tag}_st': fit[1], f'nysp_fit_{tag}_info': fit[2],
                  f'nysp_fit_{tag}_stage_names': names, f'nysp_fit_{tag}_stage_launches': launches})
    env(OI_NYS_CAP='2')
    _lib.profile_reset()
    with _lib.NystromSession(maxiter=30, profile=True) as s:
        t = []
        for a, b in [(0, 4), (4, 7)]:
            po = c.offs[a:b + 1] - c.offs[a]
            ps, pso = nystrom._ragged_sel(po, Ms[a:b])
            t.append(s.submit(c.xyt[c.offs[a]:c.offs[b]], y[c.offs[a]:c.offs[b]], po, ps, pso, x0, c.xs[a:b], c.mean))
        res = [s.wait(k) for k in t]
    env(**saved)
    names, launches = _stages(_lib, 'nys_')
    _lib.profile_reset()
    r.update(nysp_ses=np.concatenate([q[0] for q in res]), nysp_ses_st=np.concatenate([q[1] for q in res]),
             nysp_ses_info=np.concatenate([q[2] for q in res]), nysp_ses_stage_names=names,
             nysp_ses_stage_launches=launches)
    return r


def _predict(_lib, synthetic):
    ns, nts = [1, 63, 64, 65, 130], [1, 64, 65]
    sizes = [n for n in ns for _ in nts]
    c = synthetic.make_cells(sizes, seed=9)
    rng = np.random.default_rng(10)
    toffs = np.concatenate([[0], np.cumsum(nts * len(ns))])
    xs = np.repeat(c.xs, nts * len(ns), axis=0) + rng.normal(0, 1.0, (toffs[-1], 3)) * [5e4, 5e4, 1.0]
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    args = (c.xyt, c.z, c.offs, xs, toffs, c.mean, hyp)
    fs, sd, lz, cov, st = _lib.gpr_predict_multi(*args, cov=True)
    # the largest cell needs ~63 000 doubles, all of them ~360 000: 1 MiB (131 072) makes >= 3 chunks
    fs2, sd2, lz2, cov2, st2 = _lib.gpr_predict_multi(*args, cov=True, pool_bytes=1 << 20)
    _lib.profile_reset()
    _lib.gpr_predict_multi(*args, cov=True, pool_bytes=1 << 20, profile=True)
    names, launches = _stages(_lib, 'pm_')
    assert launches.max() >= 2, "pool_bytes did not force a second chunk"
    return dict(pm_fs=fs, pm_sd=sd, pm_lz=lz, pm_cov=cov, pm_st=st, pm_fs2=fs2, pm_sd2=sd2, pm_lz2=lz2,
                pm_cov2=cov2, pm_st2=st2, pm_stage_names=names, pm_stage_launches=launches)


def _loo(_lib, synthetic):
    ns = [1, 63, 64, 65, 128, 130, 333]
    c = synthetic.make_cells(ns, seed=13)
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(ns), 1))
    args = (c.xyt, c.z, c.offs, c.mean, hyp)
    mu, sd, lpl, st = _lib.gpr_loo(*args)
    # 1.6 MiB (209 715 doubles) holds the n = 333 cell but not it and its neighbours: >= 2 chunks
    mu2, sd2, lpl2, st2 = _lib.gpr_loo(*args, pool_bytes=1677721)
    _lib.profile_reset()
    _lib.gpr_loo(*args, pool_bytes=1677721, profile=True)
    names, launches = _stages(_lib, 'loo_')
    assert launches.max() >= 2, "pool_bytes did not force a second chunk"
    return dict(loo_mu=mu, loo_sd=sd, loo_lpl=lpl, loo_st=st, loo_mu2=mu2, loo_sd2=sd2, loo_lpl2=lpl2, loo_st2=st2,
                loo_stage_names=names, loo_stage_launches=launches)


def _lgo(_lib, synthetic):
    ns = [1, 63, 64, 65, 130]

    def straddle(n):  # rows 60..69 are one group: behind 60 singletons it lies across rows 64
        lab = np.arange(n)
        lab[60:70] = 60
        return lab
    kinds = [np.arange, straddle, lambda n: np.zeros(n, dtype=np.int64), lambda n: np.arange(n) % 3]
    sizes = [n for _ in kinds for n in ns]
    c = synthetic.make_cells(sizes, seed=17)
    lab = np.concatenate([k(n) for k in kinds for n in ns])
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    args = (c.offs, lab, c.mean, hyp)
    keys = ('mu', 'sd', 'lpd', 'd2', 'lpl', 'st')
    r = {}
    for tag, res in (('', _lib.gpr_lgo(c.xyt, c.z, *args)), ('2', _lib.gpr_lgo(c.xyt, c.z, *args, max_pool=2)),
                     ('_dev', _lib.gpr_lgo(*_cuda(c.xyt, c.z), *args, device_inputs=True))):
        r.update({f'lgo_{k}{tag}': v for k, v in zip(keys, res)})
    _lib.profile_reset()
    _lib.gpr_lgo(c.xyt, c.z, *args, max_pool=2, profile=True)
    names, launches = _stages(_lib, 'lgo_')
    assert launches.max() >= 2, "max_pool did not force a second chunk"
    return dict(r, lgo_stage_names=names, lgo_stage_launches=launches)


def _sample(_lib, synthetic):
    sizes, nts = [63, 64, 65, 64, 64], [0, 1, 64, 65, 2]
    c = synthetic.make_cells(sizes, seed=19)
    rng = np.random.default_rng(20)
    toffs = np.concatenate([[0], np.cumsum(nts)])
    xs = np.repeat(c.xs, nts, axis=0) + rng.normal(0, 1.0, (toffs[-1], 3)) * [5e4, 5e4, 1.0]
    xs[-1] = xs[-2]  # the last cell's two targets coincide: its latent covariance does not factor
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(sizes), 1))
    args = (c.xyt, c.z, c.offs, xs, toffs, c.mean, hyp)
    streams = np.array([7, 2 ** 63 + 5, 0, 2 ** 32, 11], dtype=np.uint64)
    r = {}
    for nsamp in (0, 1, 3):
        xi = rng.standard_normal((toffs[-1], nsamp))
        for tag, kw in (('rng', dict(seed=3)), ('streams', dict(seed=3, streams=streams)), ('xi', dict(xi=xi)),
                        ('noise', dict(seed=3, noise=True)), ('jitter', dict(seed=3, jitter=1e-6))):
            for ctag, ckw in (('', {}), ('_chunked', dict(max_pool=2))):
                res = _lib.gpr_sample(*args, nsamp, **kw, **ckw)
                r.update({f'ps_{k}_{tag}{nsamp}{ctag}': v for k, v in zip(('samples', 'fs', 'sd', 'st'), res)})
    assert r['ps_st_rng3'][-1] == 2 and r['ps_st_noise3'][-1] == 0, "the duplicated target did not give status 2"
    _lib.profile_reset()
    _lib.gpr_sample(*args, 3, seed=3, max_pool=2, profile=True)
    names, launches = _stages(_lib, 'ps_')
    assert launches.max() >= 2, "max_pool did not force a second chunk"
    return dict(r, ps_stage_names=names, ps_stage_launches=launches)


def _nystrom_multi(_lib, synthetic):
    from optimalinterpolation_amd import nystrom
    ns, Ms, nts = [70, 130, 200, 260], np.array([20, 33, 64, 65]), [1, 64, 65, 130]
    c = synthetic.make_cells(ns, seed=14)
    sel, soffs = nystrom._ragged_sel(c.offs, Ms)
    hyp = np.tile(synthetic.FIXED_HYPERS, (len(ns), 1))
    rng = np.random.default_rng(15)
    toffs = np.concatenate([[0], np.cumsum(nts)])
    xs = np.repeat(c.xs, nts, axis=0) + rng.normal(0, 1.0, (toffs[-1], 3)) * [5e4, 5e4, 1.0]
    args = (c.xyt, c.z - c.mean, c.offs, sel, soffs, hyp, xs, toffs)
    r = {}
    for tag, cov in (('', False), ('_cov', True)):
        _lib.profile_reset()
        fs, sd, cv, st = _lib.nystrom_predict_multi(*args, mean=c.mean, cov=cov, profile=True)
        names, launches = _stages(_lib, 'nys_')
        r.update({f'nysm_fs{tag}': fs, f'nysm_sd{tag}': sd, f'nysm_st{tag}': st, f'nysm_stage_names{tag}': names,
                  f'nysm_stage_launches{tag}': launches})
    r['nysm_cov'] = cv
    _lib.profile_reset()
    return r


def _svgp(_lib):
    rng = np.random.default_rng(11)
    n, M, nc = 90, 8, 2
    x = np.stack([rng.uniform(-3e5, 3e5, nc * n), rng.uniform(-3e5, 3e5, nc * n),
                  rng.integers(0, 9, nc * n).astype(float)], 1)
    y = 0.3 + 0.05 * np.sin(x[:, 0] / 1e5) + rng.normal(0, 0.02, nc * n)
    Z = np.stack([x[k * n:k * n + M] for k in range(nc)])
    init = np.tile([25e3, 25e3, 1.0, 1.0, 0.1, 0.3], (nc, 1))
    xs = np.tile([1e4, -2e4, 4.0], (nc, 1))
    kw = dict(batch=16, iterations=50, log_every=10, seed=3, want_params=True)
    offs = [0, n, 2 * n]
    pred, st, params, elbo = _lib.svgp_batch(x, y, offs, Z, init, xs, **kw)
    dev = _lib.svgp_batch(*_cuda(x, y), offs, Z, init, xs, device_inputs=True, **kw)
    r = dict(svgp_pred=pred, svgp_st=st, svgp_params=params, svgp_elbo=elbo, svgp_dev_pred=dev[0],
             svgp_dev_st=dev[1], svgp_dev_params=dev[2], svgp_dev_elbo=dev[3])
    _lib.profile_reset()
    _lib.svgp_batch(x, y, offs, Z, init, xs, profile=True, **kw)
    k = _lib.profile_json()['kernels']['k_svgp_train']
    r.update(svgp_train_launches=np.array([k['launches']]), svgp_train_flops=np.array([k['flops']]))
    # predict_f with the covariance at 3 and 70 targets, and the ELBO: one chunk, then one cell per chunk
    toffs = [0, 3, 73]
    ts = x[:73] + rng.normal(0, 1.0, (73, 3)) * [5e3, 5e3, 0.5]
    for tag, ckw in (('', {}), ('_chunked', dict(max_pool=1))):
        _lib.profile_reset()
        mean, var, cov, pst = _lib.svgp_predict(params, ts, toffs, cov=True, profile=True, **ckw)
        el, est = _lib.svgp_elbo(params, x, y, offs, profile=True, **ckw)
        names, launches = _stages(_lib, 'svgp_')
        r.update({f'svgp_pf_mean{tag}': mean, f'svgp_pf_var{tag}': var, f'svgp_pf_cov{tag}': cov,
                  f'svgp_pf_st{tag}': pst, f'svgp_full_elbo{tag}': el, f'svgp_full_elbo_st{tag}': est,
                  f'svgp_stage_names{tag}': names, f'svgp_stage_launches{tag}': launches})
    assert r['svgp_stage_launches_chunked'].max() > r['svgp_stage_launches'].max(), "max_pool=1 made no second chunk"
    return r


def _day(_lib):
    rng = np.random.default_rng(12)
    f = rng.normal(0.3, 0.1, (2, 40, 40))
    f[rng.random(f.shape) < 0.3] = np.nan
    mask = (rng.random((40, 40)) < 0.8).astype(float)
    g = np.arange(-4, 5)
    kern = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / 2.0)
    sm = _lib.smooth_fields(f, 1.0, mask, kern / kern.sum())
    pts = rng.uniform(0, 1e6, (500, 2))
    offs, idx = _lib.ball_query(pts, rng.uniform(0, 1e6, (20, 2)), 2e5)
    cols = [pts[:, 0], pts[:, 1], rng.integers(0, 9, 500).astype(float), rng.normal(0, 1, 500)]
    xyt, z = _lib.gather_rows(*cols, idx)
    return dict(day_smooth=sm, day_offs=offs, day_idx=idx, day_xyt=xyt, day_z=z)


def run(out):
    from optimalinterpolation_amd import _lib, synthetic
    r = _engine(_lib, synthetic)
    r.update(_nystrom(_lib, synthetic))
    r.update(_predict(_lib, synthetic))
    r.update(_loo(_lib, synthetic))
    r.update(_lgo(_lib, synthetic))
    r.update(_sample(_lib, synthetic))
    r.update(_nystrom_multi(_lib, synthetic))
    r.update(_svgp(_lib))
    r.update(_day(_lib))
    np.savez(out, **r)


def cmp(a, b):
    A, B = np.load(a), np.load(b)

    def same(x, y):
        return np.array_equal(x, y, equal_nan=x.dtype.kind == 'f')
    bad = [k for k in A.files if k not in B.files or not same(A[k], B[k])]
    for k in bad:
        if k in B.files and A[k].shape == B[k].shape and A[k].dtype.kind in 'fi' and A[k].size:
            d = np.abs(A[k].astype(float) - B[k].astype(float))
            print(f"DIFF {k}: max abs {np.nanmax(d):.3e} at {np.unravel_index(np.nanargmax(d), d.shape)}")
        else:
            print(f"DIFF {k}: {A[k] if A[k].size < 40 else A[k].shape} vs "
                  f"{(B[k] if B[k].size < 40 else B[k].shape) if k in B.files else 'missing'}")
    print("bitwise equal" if not bad else f"{len(bad)} arrays differ", [f for f in A.files])
    return 0 if not bad else 1


if __name__ == '__main__':
    sys.exit(run(sys.argv[2]) if sys.argv[1] == 'run' else cmp(sys.argv[2], sys.argv[3]))
