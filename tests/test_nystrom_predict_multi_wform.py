"""CPU check of the bars tests/test_gpu_nystrom_predict_multi.py holds the GPU
to.  ``oi_nystrom_predict_multi`` never forms the oracle's n x n Ki: it uses
cov = Kxs - (Kxsx'Kxsx / sn2 - V'V), V = W Kxsx, W' = C L^-T.  Restated in NumPy
(nystrom_multi_cases.wform) that algebra must agree with the oracle far inside
the GPU bars (1e-9 sf2 on cov, 1e-10 on fs) -- here within 1e-12 sf2 and 1e-13,
three orders below them -- so the bars measure the kernels, not the formula.
And the NaN class of sd must be decidable: no reference diagonal within
1e-6 sf2 of zero, with negative diagonals really present.  No GPU needed."""
import numpy as np
import pytest

import nystrom_multi_cases as MC


@pytest.mark.parametrize('hname', MC.HNAMES)
@pytest.mark.parametrize('shape', MC.SHAPES, ids=lambda s: f"n{s[0]}M{s[1]}")
def test_wform_equals_oracle_far_inside_the_gpu_bars(shape, hname):
    n, M = shape
    ell, sf2, sn2 = MC.linear(hname)
    x, y = MC.case_cell(n, M)
    for nt in (1, 65, 130):
        fs_ref, cov_ref = MC.reference(n, M, hname, nt)
        fs, cov = MC.wform(x, y, MC.targets(n, nt), ell, sf2, sn2, M)
        efs = np.max(np.abs(fs - fs_ref) / np.maximum(1.0, np.abs(fs_ref)))
        ecov = np.max(np.abs(cov - cov_ref) / np.maximum(sf2, np.abs(cov_ref)))
        print(f"n={n} M={M} {hname} nt={nt}: fs {efs:.3g} cov {ecov:.3g}")
        assert efs <= 1e-13 and ecov <= 1e-12


def test_nan_class_is_decidable_and_exercised():
    negative = {h: 0 for h in MC.HNAMES}
    for n, M in MC.SHAPES:
        for hname in MC.HNAMES:
            sf2 = MC.linear(hname)[1]
            for nt in MC.NTS:
                d = np.diag(MC.reference(n, M, hname, nt)[1])
                assert np.all(np.abs(d) >= 1e-6 * sf2), (n, M, hname, nt, np.abs(d).min() / sf2)
                negative[hname] = max(negative[hname], int((d < 0).sum()))
    print('most negative diagonals in one case:', negative)
    assert negative['H1'] > 0
