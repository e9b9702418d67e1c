"""Time oi_gpr_predict_grad against what there is without it.

    python scripts/grad_timing.py [--out FILE.json] [--repeats K]

The two batches of scripts/predict_multi_timing.py (synthetic.make_cells, seed
11, targets on a 25 km lattice around each cell's own target):
    small   64 cells x n =  500 x nt =  25
    large   16 cells x n = 3000 x nt = 121
For each: one oi_gpr_predict_grad call without and with cov; the
oi_gpr_predict_multi call at the same targets (the cost before the solve grew
from nt + 1 to 4 nt + 1 rows); and the finite-difference route, one
oi_gpr_predict_multi call at the 6 nt targets shifted by +-h_k = 1e-4 ell_k /
sqrt(3), which gives the gradient's mean only.  Every timing is a host clock
around a call that returns with its outputs on the host; one warm-up call, then
the median and the min .. max of the repeats.  Separate calls with profile=1
give oi_profile_json's per-stage split.  The two routes' gradients are
compared so that a wrong answer is not timed.
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


def stages(fn, prefix):
    _lib.profile_reset()
    fn()
    k = _lib.profile_json()['kernels']
    _lib.profile_reset()
    return {s: k[s] for s in k if s.startswith(prefix)}


def case(name, ncell, n, side, repeats):
    cells = synthetic.make_cells([n] * ncell, seed=11)
    nt = side * side
    xs = np.concatenate([lattice(cells.xs[c], side) for c in range(ncell)])
    toffs = np.arange(ncell + 1, dtype=np.int64) * nt
    hyp = np.tile(HYP, (ncell, 1))
    h = 1e-4 * HYP[:3] / np.sqrt(3.0)
    # per cell: its nt targets shifted by +h_x, -h_x, +h_y, -h_y, +h_t, -h_t
    shifts = np.concatenate([s * h[k] * np.eye(3)[k][None] for k in range(3) for s in (1.0, -1.0)])
    xs6 = (xs.reshape(ncell, 1, nt, 3) + shifts.reshape(1, 6, 1, 3)).reshape(-1, 3)

    def grad(cov, **kw):
        return _lib.gpr_predict_grad(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, hyp, blk=True, cov=cov,
                                     **kw)

    def multi(**kw):
        return _lib.gpr_predict_multi(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, hyp, cov=False, lz=True,
                                      **kw)

    def differences(**kw):
        fs = _lib.gpr_predict_multi(cells.xyt, cells.z, cells.offs, xs6, 6 * toffs, cells.mean, hyp, cov=False,
                                    lz=False, **kw)[0].reshape(ncell, 3, 2, nt)
        return ((fs[:, :, 0] - fs[:, :, 1]) / (2 * h[None, :, None])).transpose(0, 2, 1).reshape(-1, 3)

    res = dict(name=name, ncell=ncell, n=n, nt=nt)
    res['grad'] = timed(lambda: grad(False), repeats)
    res['grad_cov'] = timed(lambda: grad(True), repeats)
    res['predict_multi_same_targets'] = timed(multi, repeats)
    res['differences_6nt_targets'] = timed(differences, repeats)
    s = np.sqrt(3 * HYP[3]) / HYP[:3]
    res['max_scaled_grad_difference'] = float((np.abs(grad(False)[0] - differences()) / s).max())
    res['profile_grad'] = stages(lambda: grad(False, profile=True), 'pg_')
    res['profile_grad_cov'] = stages(lambda: grad(True, profile=True), 'pg_')
    res['profile_predict_multi'] = stages(lambda: multi(profile=True), 'pm_')
    res['profile_differences'] = stages(lambda: differences(profile=True), 'pm_')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=20)
    a = ap.parse_args()
    out = [case('small', 64, 500, 5, a.repeats), case('large', 16, 3000, 11, a.repeats)]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
