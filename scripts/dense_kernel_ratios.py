"""Worst err / err64 per quantity and configuration of the per-tile dense-kernel
tests (tests/test_gpu_dense_kernels.py, DESIGN §2 "Per-tile tests"), the
spread of err64 over the grid and the k_q that follow from them; needs the
GPU.  Writes profiles/dense_kernels/ratios.json (or --out FILE); tests/dense_ref.py
K_Q holds the k_q recorded there.  Structural findings, if any, are printed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import dense_ref as R  # noqa: E402
import test_gpu_dense_kernels as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dense_kernels', 'ratios.json'))
args = ap.parse_args()

t0 = time.time()
cells = G.grid_cells()
grid = [(c, R.Ref(c), name, rc) for c, name, rc in cells]
t_ref = time.time() - t0
print('references: %d cells, %.1f s' % (len(grid), t_ref), flush=True)
BIG = {q: 1e300 for q in R.QUANTITIES}
out = {'reference_cpu_seconds': round(t_ref, 1), 'cells': len(grid), 'ratios': {}, 'worst_cell': {}}
for panel in G.PANELS:
    for fuse in G.FUSES:
        for modes in G.MODES:
            key = 'panel_%s/%s/%s' % (panel, 'fused' if fuse else 'separate', modes)
            t1 = time.time()
            dcs = [R.DevCell(c.with_(mode=G.mode_of(modes, k))) for k, (c, _, _, _) in enumerate(grid)]
            R.run_round(dcs, panel=panel, fuse=fuse)
            t_gpu = time.time() - t1
            w, wc, nf = {}, {}, 0
            for d, (c, ref, name, _) in zip(dcs, grid):
                st = d.fetch()
                rep = R.compare(st, ref, BIG)
                if st.status != 0:
                    print(key, 'STATUS', st.status, c.T, c.rT, name)
                for f in rep.findings[:5]:
                    print(key, (c.T, c.rT, name), 'STRUCTURAL', f)
                nf += len(rep.findings)
                for q, r in rep.ratios.items():
                    if r > w.get(q, 0.0):
                        w[q], wc[q] = r, [c.T, c.rT, name]
            out['ratios'][key] = {q: round(v, 3) for q, v in w.items()}
            out['worst_cell'][key] = wc
            print(key, 'round+alloc %.2fs total %.1fs findings %d' % (t_gpu, time.time() - t1, nf),
                  {q: round(v, 2) for q, v in w.items()}, flush=True)
worst = {q: max(v.get(q, 0.0) for v in out['ratios'].values()) for q in R.QUANTITIES}
spread = {q: max(r.err64[q] for _, r, _, _ in grid) / statistics.median(r.err64[q] for _, r, _, _ in grid)
          for q in R.QUANTITIES}
out['worst_ratio'] = {q: round(v, 3) for q, v in worst.items()}
out['err64_spread_max_over_median'] = {q: round(v, 3) for q, v in spread.items()}
out['err64_max'] = {q: float('%.3g' % max(r.err64[q] for _, r, _, _ in grid)) for q in R.QUANTITIES}
out['err64_median'] = {q: float('%.3g' % statistics.median(r.err64[q] for _, r, _, _ in grid)) for q in R.QUANTITIES}
k = {}
for q in R.QUANTITIES:
    x = worst[q] * spread[q]
    k[q] = float(2 ** int(np.ceil(np.log2(max(x, 1.0)))))
out['k_q'] = k
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
print('worst', worst)
print('spread', spread)
print('k_q', k)
