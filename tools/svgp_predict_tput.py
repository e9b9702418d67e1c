"""oi_svgp_predict / oi_svgp_elbo: device time per stage (HIP events through
opts.profile -> oi_profile_json) and host wall time per call, for the shapes of
profiles/svgp_predict/README.md.  Synthetic models (nothing trains).

    python tools/svgp_predict_tput.py [reps] [out.json]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from oracle import svgp_oracle as O
from optimalinterpolation_amd import _lib

rng = np.random.default_rng(1)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STAGES = ('svgp_model', 'svgp_targets', 'svgp_cov', 'svgp_reduce')


def points(n):
    return np.stack([rng.uniform(-3e5, 3e5, n), rng.uniform(-3e5, 3e5, n), rng.uniform(0, 8, n)], 1)


def models(k, M):
    rows = []
    for _ in range(k):
        p = O.Params(O.notebook_Z(points(200), M), [25e3, 25e3, 1], 1.0, 0.1, 0.3)
        p.q_mu = rng.normal(0, 1, M)
        S = np.tril(rng.normal(0, 0.3, (M, M)))
        S[np.diag_indices(M)] = rng.uniform(0.2, 1.2, M)
        p.S = S
        rows.append(p.flat())
    return np.stack(rows)


def timed(name, call):
    call()  # warm: code objects, allocations
    _lib.profile_reset()
    wall = []
    for _ in range(reps):  # host clock around a call that returns with its outputs on the host
        t = time.perf_counter()
        st = call(profile=True)[-1]
        wall.append((time.perf_counter() - t) * 1e3)
    k = _lib.profile_json()['kernels']
    _lib.profile_reset()
    rec = dict(shape=name, reps=reps, wall_ms_median=float(np.median(wall)), wall_ms_min=min(wall),
               wall_ms_max=max(wall), failed_cells=int(st.sum()),
               stages={s: dict(ms_per_call=k[s]['total_ms'] / reps, launches_per_call=k[s]['launches'] / reps,
                               gflops=k[s]['flops'] / max(k[s]['total_ms'], 1e-9) / 1e6)
                       for s in STAGES if s in k})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    out = []
    M = 50
    th = models(1, M)
    xs = points(100_000)
    out.append(timed('predict: 1 model x 100000 targets, M=50',
                     lambda **k: _lib.svgp_predict(th, xs, [0, len(xs)], **k)))
    th = models(256, M)
    n = 4600
    X = points(256 * n)
    Y = 0.3 + 0.05 * np.sin(X[:, 0] / 1e5) + rng.normal(0, 0.02, len(X))
    offs = np.arange(257) * n
    out.append(timed('predict: 256 models x 4600 targets, M=50',
                     lambda **k: _lib.svgp_predict(th, X, offs, **k)))
    out.append(timed('elbo: 256 models x 4600 observations, M=50',
                     lambda **k: _lib.svgp_elbo(th, X, Y, offs, **k)))
    th16, nt = th[:16], 2000
    xs16 = points(16 * nt)
    out.append(timed('predict + cov: 16 models x 2000 targets, M=50',
                     lambda **k: _lib.svgp_predict(th16, xs16, np.arange(17) * nt, cov=True, **k)))
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
