"""Time oi_gpr_sample against the prediction it rides on and the host route.

    python scripts/sample_timing.py [--out FILE.json] [--repeats K] [--host-repeats K]

Synthetic cells (synthetic.make_cells, seed 11) at the hypers (2e5 m, 2e5 m,
6 d, 5e-3, 1e-3), 121 targets per cell on an 11 x 11 lattice of 25 km:
    config2   1000 cells x n =  500, nsamp = 1 and 100
    large        1 cell  x n = 4600, nsamp = 100
For each, on the same batch:
  (a) sample   one oi_gpr_sample call in RNG mode (latent draws)
  (b) predict  one oi_gpr_predict_multi call without cov: (a) - (b) is the
               draw's own cost
  (c) host     the only route without oi_gpr_sample: gpr_predict_multi(cov=True),
               then per cell np.linalg.cholesky, standard_normal and the
               product on the host (numpy's BLAS threads as the environment
               sets them)
Host clock around each call, which returns with its outputs on the host; one
warm-up each, then (a) and (b) alternate for the repeats; median and min .. max.
The per-stage split of (a) comes from as many further profiled calls
(oi_profile_json, HIP events around each stage).  Before anything is timed,
oi_gpr_sample with given normals is compared with route (c)'s arithmetic on
the same normals, so a wrong answer is not timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from optimalinterpolation_amd import _lib, synthetic  # noqa: E402

HYP = np.array([2.0e5, 2.0e5, 6.0, 5.0e-3, 1.0e-3])
NT = 121


def spread(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), repeats=len(ts))


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def lattice(centre, nt, spacing=25e3):
    side = int(np.ceil(np.sqrt(nt)))
    g = (np.arange(side) - (side - 1) / 2) * spacing
    gx, gy = np.meshgrid(g, g, indexing='ij')
    return np.stack([centre[0] + gx.ravel(), centre[1] + gy.ravel(), np.full(side * side, centre[2])], axis=1)[:nt]


def host_draw(fs, cov, toffs, nsamp, rng=None, xi=None):
    """Route (c)'s host half: factor every cell's covariance and draw."""
    out = np.empty((len(fs), nsamp))
    for c, C in enumerate(_lib.split_cov(cov, toffs)):
        a, e = toffs[c], toffs[c + 1]
        L = np.linalg.cholesky(C)
        z = xi[a:e] if xi is not None else rng.standard_normal((e - a, nsamp))
        out[a:e] = fs[a:e, None] + L @ z
    return out


def case(name, ncell, n, nsamp, repeats, host_repeats):
    cells = synthetic.make_cells([n] * ncell, seed=11)
    hyp = np.tile(HYP, (ncell, 1))
    xs = np.concatenate([lattice(cells.xs[c], NT) for c in range(ncell)])
    toffs = np.arange(ncell + 1, dtype=np.int64) * NT
    args = (cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, hyp)

    def sample(**kw):
        return _lib.gpr_sample(*args, nsamp, seed=1, **kw)

    def predict(cov=False):
        return _lib.gpr_predict_multi(*args, cov=cov, lz=False)

    rng = np.random.default_rng(5)

    def host():
        fs, _, _, cov, _ = predict(cov=True)
        return host_draw(fs, cov, toffs, nsamp, rng=rng)

    res = dict(name=name, ncell=ncell, n=n, nt=NT, nsamp=nsamp)
    # the same normals through both routes
    xi = rng.standard_normal((ncell * NT, nsamp))
    got, fs, sd, st = sample(xi=xi)
    pfs, psd, _, cov, pst = predict(cov=True)
    assert not st.any() and not pst.any() and np.array_equal(fs, pfs) and np.array_equal(sd, psd)
    res['max_abs_difference_to_host_route'] = float(np.abs(got - host_draw(pfs, cov, toffs, nsamp, xi=xi)).max())
    assert res['max_abs_difference_to_host_route'] <= 1e-10 * np.sqrt(HYP[3])
    sample()
    predict()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(clock(sample))
        tb.append(clock(predict))
    res['sample'], res['predict'] = spread(ta), spread(tb)
    res['draw_cost_ms'] = res['sample']['median_ms'] - res['predict']['median_ms']
    host()
    res['host'] = spread([clock(host) for _ in range(host_repeats)])
    res['host_over_sample'] = res['host']['median_ms'] / res['sample']['median_ms']
    stages = {}
    for _ in range(repeats):
        _lib.profile_reset()
        sample(profile=True)
        k = _lib.profile_json()['kernels']
        for s in k:
            if s.startswith('ps_'):
                stages.setdefault(s, []).append(k[s]['total_ms'])
    _lib.profile_reset()
    res['stages'] = {s: spread(v) for s, v in stages.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--host-repeats', type=int, default=5)
    a = ap.parse_args()
    out = [case('config2', 1000, 500, 1, a.repeats, a.host_repeats),
           case('config2', 1000, 500, 100, a.repeats, a.host_repeats),
           case('large', 1, 4600, 100, a.repeats, a.host_repeats)]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
