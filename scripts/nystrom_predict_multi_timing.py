"""Time oi_nystrom_predict_multi against the loop of single-target calls it replaces.

    python scripts/nystrom_predict_multi_timing.py [--out FILE.json] [--repeats K] [--loop-repeats K]

Two batches of seeded cells on distinct sites of a 25 km x 1 day lattice
(as the notebook-size test of tests/test_gpu_nystrom.py draws them), hypers
(6e4 m, 9e4 m, 3 d, 6e-3, 3e-3), targets on a 25 km lattice offset by 12.5 km
around (0, 0, 4.5):
    small      16 cells x n =  500, M = 100, nt =  25
    notebook    1 cell  x n = 4600, M = 925, nt = 121
For each: one oi_nystrom_predict_multi call without and with cov, and the loop
of nt oi_nystrom_batch predict calls (one target per cell per call) that gives
the same fs / sd without the new entry.  Every timing is a host clock around a
call that returns with its outputs on the host (the library synchronises its
stream before returning); one warm-up call, then the median and the min .. max
of the repeats.  A last, separate call with profile=1 gives oi_profile_json's
per-stage split.  The two routes' fs are compared so a wrong answer is not
timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalinterpolation_amd import _lib, nystrom  # noqa: E402

HYP = np.array([6e4, 9e4, 3.0, 6e-3, 3e-3])
MEAN = 0.28


def cells(ncell, n, seed):
    rng = np.random.default_rng(seed)
    g = np.arange(-12, 13) * 25e3
    sites = np.array([(a, b, t) for a in g for b in g for t in range(9)], dtype=np.float64)
    xyt = np.concatenate([sites[rng.choice(len(sites), n, replace=False)] for _ in range(ncell)])
    y = 0.05 * np.sin(xyt[:, 0] / 2e5) + 0.01 * (xyt[:, 2] - 4) + rng.normal(0, 0.02, len(xyt))
    return xyt, y, np.arange(ncell + 1, dtype=np.int64) * n


def lattice(side, spacing=25e3):
    g = (np.arange(side) - (side - 1) / 2) * spacing + 12.5e3
    gx, gy = np.meshgrid(g, g, indexing='ij')
    return np.stack([gx.ravel(), gy.ravel(), np.full(side * side, 4.5)], axis=1)


def timed(fn, repeats):
    fn()  # warm-up: code objects, workspace
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                repeats=int(repeats))


def case(name, ncell, n, M, side, repeats, loop_repeats):
    xyt, y, offs = cells(ncell, n, seed=5)
    nt = side * side
    xs = np.tile(lattice(side), (ncell, 1))
    toffs = np.arange(ncell + 1, dtype=np.int64) * nt
    hyp = np.tile(HYP, (ncell, 1))
    sel, soffs = nystrom._ragged_sel(offs, M)

    def multi(cov, **kw):
        return _lib.nystrom_predict_multi(xyt, y, offs, sel, soffs, hyp, xs, toffs, mean=MEAN, cov=cov, **kw)

    def loop():
        fs = np.empty((ncell, nt))
        for t in range(nt):
            _, _, pred, _ = _lib.nystrom_batch(xyt, y, offs, sel, soffs, hyp, xs=xs[t::nt], mean=MEAN,
                                               objective=False, predict=True)
            fs[:, t] = pred[:, 0]
        return fs

    res = dict(name=name, ncell=ncell, n=n, M=M, nt=nt)
    res['multi'] = timed(lambda: multi(False), repeats)
    res['multi_cov'] = timed(lambda: multi(True), repeats)
    res['loop_single_target'] = timed(loop, loop_repeats)
    fs = multi(False)[0].reshape(ncell, nt)
    ref = loop()
    res['max_abs_fs_difference'] = float(np.abs(fs - ref).max())
    _lib.profile_reset()
    multi(True, profile=True)
    k = _lib.profile_json()['kernels']
    res['profile_with_cov'] = {s: k[s] for s in k if s.startswith('nys_')}
    _lib.profile_reset()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--loop-repeats', type=int, default=3)
    a = ap.parse_args()
    out = [case('small', 16, 500, 100, 5, a.repeats, a.loop_repeats),
           case('notebook', 1, 4600, 925, 11, a.repeats, a.loop_repeats)]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
