"""Time a one-shot oi_nystrom_fit_batch of many small, unequal cells: the shape
at which the fit's host loop and its grouping of the cells weigh most.

    [OI_LIB=/path/to/liboi.so] python scripts/nystrom_fit_timing.py [--out FILE.json] [--cells N] [--repeats K]

N seeded cells (default 256) with n drawn from 100..300 and M from 20..65
(M <= n), CG from nystrom.default_x0() with maxiter 30.  The timing is a host
clock around the call, which returns with its outputs on the host; one warm-up
call, then the median and the min .. max of the repeats.  A last, separate
call with profile=1 gives the nys_* stages' launches and times.  OI_LIB picks
the build (default: the tree's own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalinterpolation_amd import _lib, nystrom, synthetic  # noqa: E402

MAXITER = 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--cells', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(21)
    ns = rng.integers(100, 301, a.cells)
    Ms = rng.integers(20, 66, a.cells)
    c = synthetic.make_cells([int(n) for n in ns], seed=22)
    y = c.z - c.mean
    sel, soffs = nystrom._ragged_sel(c.offs, Ms)
    x0 = nystrom.default_x0()

    def fit(**kw):
        return _lib.nystrom_fit_batch(c.xyt, y, c.offs, sel, soffs, x0, c.xs, c.mean, maxiter=MAXITER, **kw)

    out, status, info = fit()  # warm-up: code objects
    ts = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        fit()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    _lib.profile_reset()
    fit(profile=True)
    k = _lib.profile_json()['kernels']
    _lib.profile_reset()
    res = dict(build='OI_LIB' if os.environ.get('OI_LIB') else 'tree', cells=int(a.cells), n=[int(ns.min()), int(ns.max())],
               M=[int(Ms.min()), int(Ms.max())], maxiter=MAXITER, repeats=int(a.repeats),
               median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
               calls_ms=[float(t) for t in ts], cells_failed=int((status != 0).sum()),
               evals_per_cell=float(info[:, 3].mean()), max_evals=int(info[:, 3].max()),
               profile={s: k[s] for s in k if s.startswith('nys_')})
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
