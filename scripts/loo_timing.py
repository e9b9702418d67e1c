"""Time oi_gpr_loo against the two routes that exist without it.

    python scripts/loo_timing.py [--out FILE.json] [--repeats K]

Two batches of synthetic cells (synthetic.make_cells, seed 11) at the hypers
(2e5 m, 2e5 m, 6 d, 5e-3, 1e-3):
    small   64 cells x n =  500
    large   16 cells x n = 3000
For each:
  new       one oi_gpr_loo call (host clock around the call, which returns with
            its outputs on the host), one warm-up, then the median and min .. max
            of the repeats; and the per-stage split of oi_profile_json over as
            many further profiled calls (HIP events around each stage)
  (a) brute the parent commit's only route: a cell of n observations as n cells
            of n - 1 observations with one target each in one
            oi_gpr_predict_multi call.  Timed for ONE cell of the batch and
            SCALED by the cell count.
  (b) parts what the existing parts give without a new kernel: oila::cholesky and
            oila::trsm_right_lt on an n x n identity (L^-T, whose column norms and
            product with zt give q and alpha) for the same matrices, through
            tests/oila_ref.py's run_cholesky / run_trsm, HIP events around each.
The new call's mu is compared with route (a)'s on the timed cell, so a wrong
answer is not timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from optimalinterpolation_amd import _lib, synthetic  # noqa: E402

HYP = np.array([2.0e5, 2.0e5, 6.0, 5.0e-3, 1.0e-3])


def spread(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), repeats=len(ts))


def timed(fn, repeats, warm=True):
    if warm:
        fn()  # code objects, workspace
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def brute(cells, c, hyp):
    """Cell c as n cells of n - 1 observations, each predicting the one left out."""
    x, z, _ = cells.cell(c)
    n = len(z)
    keep = [np.arange(n) != i for i in range(n)]
    xyt = np.concatenate([x[k] for k in keep])
    zz = np.concatenate([z[k] for k in keep])
    offs = np.arange(n + 1, dtype=np.int64) * (n - 1)
    toffs = np.arange(n + 1, dtype=np.int64)
    h = np.tile(hyp, (n, 1))
    return lambda: _lib.gpr_predict_multi(xyt, zz, offs, x, toffs, cells.mean, h, lz=False)


def parts(cells, repeats):
    """oila::cholesky, then oila::trsm_right_lt on an identity, for the batch's
    matrices K + sn2 I (generated with torch: plumbing, not timed)."""
    import torch
    import oila_ref as R
    ell = torch.tensor(HYP[:3], device='cuda')
    Ks, work = [], []
    for c in range(cells.ncell):
        x, _, _ = cells.cell(c)
        s = np.sqrt(3.0) * torch.from_numpy(x).cuda() / ell
        Q = torch.cdist(s, s)
        Ks.append(HYP[3] * (1 + Q) * torch.exp(-Q) + HYP[4] * torch.eye(len(x), device='cuda', dtype=torch.float64))
        n = len(x)
        work.append(dict(A=torch.empty_like(Ks[-1]), X=torch.empty_like(Ks[-1]),
                         dinv=torch.zeros(((n + 63) // 64) * 4096, device='cuda', dtype=torch.float64),
                         info=torch.zeros(1, device='cuda', dtype=torch.int32), n=n))
    chol = [R.Chol(w['A'].data_ptr(), w['dinv'].data_ptr(), w['info'].data_ptr(), w['n'], w['n']) for w in work]
    trsm = [R.TrsmRLT(w['X'].data_ptr(), w['A'].data_ptr(), w['dinv'].data_ptr(), w['n'], w['n'], w['n'], w['n'])
            for w in work]
    tc, ts = [], []
    for r in range(repeats + 1):
        for K, w in zip(Ks, work):
            w['A'].copy_(K)   # symmetric: row-major = column-major
            w['X'].copy_(torch.eye(w['n'], device='cuda', dtype=torch.float64))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        R.run_cholesky(chol)
        ev[1].record()
        R.run_trsm(trsm)
        ev[2].record()
        torch.cuda.synchronize()
        if r:  # the first pass is the warm-up
            tc.append(ev[0].elapsed_time(ev[1]))
            ts.append(ev[1].elapsed_time(ev[2]))
    assert all(int(w['info'].item()) == 0 for w in work)
    return dict(cholesky=spread(tc), trsm_identity=spread(ts))


def case(name, ncell, n, repeats, brute_repeats):
    cells = synthetic.make_cells([n] * ncell, seed=11)
    hyp = np.tile(HYP, (ncell, 1))

    def new(**kw):
        return _lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, hyp, **kw)

    res = dict(name=name, ncell=ncell, n=n)
    res['new'] = timed(new, repeats)
    stages = {}
    for _ in range(repeats):
        _lib.profile_reset()
        new(profile=True)
        k = _lib.profile_json()['kernels']
        for s in k:
            if s.startswith('loo_'):
                stages.setdefault(s, []).append(k[s]['total_ms'])
    _lib.profile_reset()
    res['stages'] = {s: spread(v) for s, v in stages.items()}
    one, last = brute(cells, 0, HYP), []
    # no warm-up of its own at n = 3000 (seconds per call; the code objects are warm by then)
    t = timed(lambda: last.append(one()), brute_repeats, warm=(n <= 1000))
    res['brute_one_cell'] = t
    res['brute_scaled_to_batch_ms'] = t['median_ms'] * ncell
    res['max_abs_mu_difference_to_brute'] = float(np.abs(new()[0][:n] - last[-1][0]).max())
    res['parts'] = parts(cells, repeats)
    sw, tr = res['stages']['loo_sweep'], res['parts']['trsm_identity']
    res['sweep_faster_than_trsm_ranges_disjoint'] = bool(sw['max_ms'] < tr['min_ms'])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--brute-repeats', type=int, default=2)
    a = ap.parse_args()
    out = [case('small', 64, 500, a.repeats, a.brute_repeats),
           case('large', 16, 3000, a.repeats, a.brute_repeats)]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
