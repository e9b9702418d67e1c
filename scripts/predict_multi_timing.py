"""Time oi_gpr_predict_multi against the loop of single-target calls it replaces.

    python scripts/predict_multi_timing.py [--out FILE.json] [--loop-repeats K]

Two batches of synthetic cells (synthetic.make_cells, seed 11), targets on a
25 km lattice around each cell's own target:
    small   64 cells x n =  500 x nt =  25
    large   16 cells x n = 3000 x nt = 121
For each: one oi_gpr_predict_multi call without and with cov, and the loop of
nt oi_gpr_batch(opt=0) calls (one target per cell per call) that gives the same
fs / sd without the new entry.  Every timing is a host clock around a call that
returns with its outputs on the host (the library synchronises its stream
before returning); one warm-up call, then the median and the min .. max of the
repeats.  A last, separate call with profile=1 gives oi_profile_json's per-stage
split.  The two routes' fs are compared so a wrong answer is not timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalinterpolation_amd import _lib, synthetic  # noqa: E402

HYP = np.array([2.0e5, 2.0e5, 6.0, 5.0e-3, 1.0e-3])


def lattice(centre, side, spacing=25e3):
    g = (np.arange(side) - (side - 1) / 2) * spacing
    gx, gy = np.meshgrid(g, g, indexing='ij')
    return np.stack([centre[0] + gx.ravel(), centre[1] + gy.ravel(), np.full(side * side, centre[2])], axis=1)


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


def case(name, ncell, n, side, repeats, loop_repeats):
    cells = synthetic.make_cells([n] * ncell, seed=11)
    nt = side * side
    xs = np.concatenate([lattice(cells.xs[c], side) for c in range(ncell)])
    toffs = np.arange(ncell + 1, dtype=np.int64) * nt
    hyp = np.tile(HYP, (ncell, 1))

    def multi(cov, **kw):
        return _lib.gpr_predict_multi(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, hyp,
                                      cov=cov, lz=True, **kw)

    def loop():
        fs = np.empty((ncell, nt))
        for t in range(nt):
            out, _, _ = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, xs[t::nt], cells.mean, opt=False,
                                       hyp=hyp)
            fs[:, t] = out[:, 0]
        return fs

    res = dict(name=name, ncell=ncell, n=n, nt=nt)
    res['multi'] = timed(lambda: multi(False), repeats)
    res['multi_cov'] = timed(lambda: multi(True), repeats)
    res['loop_single_target'] = timed(loop, loop_repeats)
    fs = multi(False)[0].reshape(ncell, nt)
    ref = loop()
    res['max_abs_fs_difference'] = float(np.abs(fs - ref).max())
    _lib.profile_reset()
    multi(True, profile=True)
    k = _lib.profile_json()['kernels']
    res['profile_with_cov'] = {s: k[s] for s in k if s.startswith('pm_')}
    _lib.profile_reset()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--loop-repeats', type=int, default=3)
    a = ap.parse_args()
    out = [case('small', 64, 500, 5, a.repeats, a.loop_repeats),
           case('large', 16, 3000, 11, a.repeats, a.loop_repeats)]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
