"""Time oi_gpr_lgo against the only route that exists without it.

    python scripts/lgo_timing.py [--out FILE.json] [--repeats K]

Two batches of synthetic cells (synthetic.make_cells, seed 11) at the hypers
(2e5 m, 2e5 m, 6 d, 5e-3, 1e-3):
    small   64 cells x n =  500
    large   16 cells x n = 3000
each with four groupings of every cell:
    singletons   one group per observation (beside oi_gpr_loo on the same cells)
    sites        gpr.site_groups: the bitwise-equal (x, y, t) rows
    36 groups    observation i in group i mod 36
    4 groups     observation i in group i mod 4
For each:
  new    one oi_gpr_lgo call (host clock around the call, which returns with its
         outputs on the host), one warm-up, then the median and min .. max of
         the repeats; and the per-stage split of oi_profile_json over as many
         further profiled calls (HIP events around each stage)
  brute  the parent commit's only route: one cell per group through ONE
         oi_gpr_predict_multi call with the covariance, that group removed and
         its members as targets (the noise and the joint density would still
         have to be added on the host: not timed).  Timed for ONE cell of the
         batch and SCALED by the cell count.
The new call's mu is compared with the brute route's on the timed cell, so a
wrong answer is not timed.  `ratios`: on the inputs of tests/test_gpu_lgo.py,
the worst error of the GPU against each numpy reference beside the two
references' own spread (tests/lgo_ref.py: closed form vs one refit per group).
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
from optimalinterpolation_amd import _lib, gpr, synthetic  # noqa: E402

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


def brute(cells, c, lab, hyp):
    """Cell c as one cell per group: the group removed, its members the targets."""
    import lgo_ref as R
    x, z, _ = cells.cell(c)
    members = R.groups_of(lab[cells.offs[c]:cells.offs[c + 1]])
    n = len(z)
    rest = [np.setdiff1d(np.arange(n), m) for m in members]
    xyt = np.concatenate([x[r] for r in rest])
    zz = np.concatenate([z[r] for r in rest])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rest])]).astype(np.int64)
    order = np.concatenate(members)
    toffs = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    h = np.tile(hyp, (len(members), 1))
    return order, lambda: _lib.gpr_predict_multi(xyt, zz, offs, x[order], toffs, cells.mean, h, cov=True, lz=False)


def groupings(cells):
    i = np.concatenate([np.arange(n) for n in cells.sizes])
    return [('singletons', i), ('sites', gpr.site_groups(cells.xyt, cells.offs)), ('36 groups', i % 36),
            ('4 groups', i % 4)]


def stage_split(fn, prefix, repeats):
    stages = {}
    for _ in range(repeats):
        _lib.profile_reset()
        fn(profile=True)
        k = _lib.profile_json()['kernels']
        for s in k:
            if s.startswith(prefix):
                stages.setdefault(s, []).append(k[s]['total_ms'])
    _lib.profile_reset()
    return {s: spread(v) for s, v in stages.items()}


def case(name, ncell, n, repeats, brute_repeats):
    cells = synthetic.make_cells([n] * ncell, seed=11)
    hyp = np.tile(HYP, (ncell, 1))
    res = dict(name=name, ncell=ncell, n=n, groupings=[])

    def loo(**kw):
        return _lib.gpr_loo(cells.xyt, cells.z, cells.offs, cells.mean, hyp, **kw)

    res['loo'] = dict(new=timed(loo, repeats), stages=stage_split(loo, 'loo_', repeats))
    for gname, lab in groupings(cells):
        def new(**kw):
            return _lib.gpr_lgo(cells.xyt, cells.z, cells.offs, lab, cells.mean, hyp, **kw)

        g = dict(grouping=gname, groups_in_cell_0=int(len(np.unique(lab[:n]))))
        g['new'] = timed(new, repeats)
        g['stages'] = stage_split(new, 'lgo_', repeats)
        out = new()
        assert not out[5].any()
        order, one = brute(cells, 0, lab, HYP)
        last = []
        # no warm-up of its own at n = 3000 (seconds per call; the code objects are warm by then)
        t = timed(lambda: last.append(one()), brute_repeats, warm=(n <= 1000))
        g['brute_one_cell'] = t
        g['brute_scaled_to_batch_ms'] = t['median_ms'] * ncell
        g['max_abs_mu_difference_to_brute'] = float(np.abs(out[0][:n][order] - last[-1][0]).max())
        res['groupings'].append(g)
        print(json.dumps(g), flush=True)
    return res


def ratios():
    import lgo_ref as R
    xyt, z, offs, lab, mean, hyp = R.batch()
    got = _lib.gpr_lgo(xyt, z, offs, lab, mean, hyp)
    keys = ('mu', 'sd', 'lpd', 'd2', 'lpl')
    worst = {k: dict(gpu_vs_closed=0.0, gpu_vs_brute=0.0, closed_vs_brute=0.0) for k in keys}
    for c, spec in enumerate(R.SPECS):
        closed, brute_ = R.refs(spec[0])
        a, e = offs[c], offs[c + 1]
        g = tuple(v[a:e] for v in got[:4]) + (got[4][c],)
        for tag, err in (('gpu_vs_closed', R.errors(g, closed)), ('gpu_vs_brute', R.errors(g, brute_)),
                         ('closed_vs_brute', R.errors(closed, brute_))):
            for k, v in zip(keys, err):
                worst[k][tag] = max(worst[k][tag], float(v))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--brute-repeats', type=int, default=2)
    a = ap.parse_args()
    out = dict(ratios=ratios(),
               cases=[case('small', 64, 500, a.repeats, a.brute_repeats),
                      case('large', 16, 3000, a.repeats, a.brute_repeats)])
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
