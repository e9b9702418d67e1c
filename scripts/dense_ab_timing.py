"""One gpr_lgo call and one gpr_sample call of the same shape, for an A/B of two
builds of liboi.so (OI_LIB names the one to load; default the tree's own).

    [OI_LIB=/path/to/liboi.so] python scripts/dense_ab_timing.py [TAG]

64 cells x n = 500: scripts/lgo_timing.py's `small` batch, its '36 groups'
labelling and its clock (one warm-up, 30 repeats, median and min .. max); the
draw is 100 samples at scripts/sample_timing.py's 121 targets per cell.
Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import lgo_timing as T  # noqa: E402
import sample_timing as S  # noqa: E402
from optimalinterpolation_amd import _lib, synthetic  # noqa: E402

ncell, n, repeats = 64, 500, 30
cells = synthetic.make_cells([n] * ncell, seed=11)
hyp = np.tile(T.HYP, (ncell, 1))
lab = dict(T.groupings(cells))['36 groups']
xs = np.concatenate([S.lattice(cells.xs[c], S.NT) for c in range(ncell)])
toffs = np.arange(ncell + 1, dtype=np.int64) * S.NT
lgo = T.timed(lambda: _lib.gpr_lgo(cells.xyt, cells.z, cells.offs, lab, cells.mean, hyp), repeats)
smp = T.timed(lambda: _lib.gpr_sample(cells.xyt, cells.z, cells.offs, xs, toffs, cells.mean, hyp, 100, seed=1), repeats)
print(json.dumps(dict(lib=os.path.basename(_lib.LIB_PATH), tag=sys.argv[1] if len(sys.argv) > 1 else '', ncell=ncell,
                      n=n, nt=S.NT, nsamp=100, gpr_lgo=lgo, gpr_sample=smp)))
