"""``oi_gpr_lgo`` without a GPU: the two numpy references of
tests/lgo_ref.py agree on every input of tests/test_gpu_lgo.py, the library's
host plan and workspace count equal their Python restatements, the symbol is
declared, exported and bound, ``gpr.site_groups`` joins exactly the repeated
sites, and every misuse is rejected with OI_E_ARG (-1) before any device work.
"""
import ctypes

import numpy as np
import pytest

import abi_ref
from optimalinterpolation_amd import _lib, gpr, nystrom
import lgo_ref as R

D, I64, I32 = ctypes.c_double, ctypes.c_int64, ctypes.c_int32
NAMES = [s[0] for s in R.SPECS]


# -- the references ---------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_closed_form_agrees_with_one_refit_per_group(name):
    """Within 1e-11 in the GPU test's own five figures: 100 x inside its bound,
    a condition on the inputs."""
    closed, brute = R.refs(name)
    e = R.errors(closed, brute)
    print(name, ' '.join(f'{v:.2e}' for v in e))
    assert max(e) <= 1e-11, e
    assert all(np.isfinite(a).all() for a in closed[:4]) and (closed[1] > 0).all()


def test_the_shapes_the_gpu_file_needs():
    cs, _ = R.cases()
    assert [len(c[2]) for c in cs] == [1, 2, 63, 64, 65, 130, 130, 333, 700]
    seen = set()
    for name, x, z, lab, sizes in cs:
        perm, start, size, _ = R.plan(lab)
        assert list(size) == sizes and sum(sizes) == len(z), name    # the sort puts the groups where SPECS says
        assert not np.array_equal(perm, np.arange(len(z))) or len(sizes) in (1, len(z)), name   # the order matters
        seen |= {(int(g), int(c0) % 64) for c0, g in zip(start, size)}
        assert len(np.unique(x, axis=0)) < len(z) or len(z) < 3, name   # repeated sites
    want = {(63, 0), (64, 0), (128, 0), (2, 0), (1, 1), (64, 1), (65, 1), (129, 1), (1, 63), (2, 63), (65, 63),
            (130, 63)}
    assert want <= seen, want - seen
    assert {g for g, _ in seen} >= {1, 2, 63, 64, 65, 128, 129, 130}
    labs = np.concatenate([c[3] for c in cs])
    assert labs.min() < -(1 << 61) and labs.max() > (1 << 61)
    sites = next(c for c in cs if c[0] == 'n130-sites')
    assert 1 < max(sites[4]) and len(sites[4]) == 90


def test_special_cases_of_the_references():
    cs, mean = R.cases()
    _, x, z, lab, _ = next(c for c in cs if c[0] == 'n64-whole')
    mu, sd, lpd, d2, lpl = R.lgo_closed(x, z, lab, mean, R.HYP)
    assert np.allclose(mu, mean, rtol=0, atol=1e-12) and np.allclose(sd, np.sqrt(R.HYP[3] + R.HYP[4]), rtol=1e-12)
    import loo_ref
    _, x, z, lab, _ = next(c for c in cs if c[0] == 'n63-singletons')
    mu, sd, lpd, d2, lpl = R.lgo_closed(x, z, lab, mean, R.HYP)
    lmu, lsd, llpl = loo_ref.loo_closed(x, z, mean, R.HYP)
    assert np.allclose(mu, lmu, rtol=1e-12) and np.allclose(sd, lsd, rtol=1e-12) and abs(lpl - llpl) < 1e-10
    assert np.allclose(d2, ((z - mu) / sd) ** 2, rtol=1e-10)


# -- the host plan and the workspace count ------------------------------------

def _labels():
    cs, _ = R.cases()
    rng = np.random.default_rng(5)
    out = [c[3] for c in cs]
    out.append(np.zeros(0, dtype=np.int64))
    out.append(rng.integers(-3, 3, 200))                      # few groups, scattered over every block
    out.append(np.repeat(np.arange(4), 64))                   # four aligned groups: diagonal tiles only
    out.append(np.arange(129)[::-1] // 2)                     # pairs, one straddling each boundary
    return out


@pytest.mark.parametrize('k', range(13))
def test_plan_equals_its_restatement(k):
    lab = _labels()[k]
    perm, start, size, tiles = R.lib_plan(lab)
    rperm, rstart, rsize, rtiles = R.plan(lab)
    assert np.array_equal(perm, rperm) and np.array_equal(start, rstart) and np.array_equal(size, rsize)
    assert sorted(np.asarray(perm).tolist()) == list(range(len(lab)))
    assert len(set(tiles)) == len(tiles) and tiles == rtiles        # none twice, none missing, dispatch order
    T = (len(lab) + 63) // 64
    assert {(A, A) for A in range(T)} <= set(tiles) and all(0 <= B <= A < T for A, B in tiles)
    # groups in the order of first appearance, members in observation order
    firsts = [perm[s] for s in start]
    assert firsts == sorted(firsts)
    for s, g in zip(start, size):
        assert len(set(lab[perm[s:s + g]].tolist())) == 1 and (np.diff(perm[s:s + g]) > 0).all()


def test_plan_lists_diagonal_tiles_only_for_aligned_groups():
    assert R.lib_plan(np.repeat(np.arange(4), 64))[3] == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert R.lib_plan(np.zeros(130, dtype=np.int64))[3] == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    assert R.lib_plan(np.array([7] + [3] * 64))[3] == [(0, 0), (1, 0), (1, 1)]


@pytest.mark.parametrize('host', [True, False])
def test_cell_doubles_equal_the_closed_form(host):
    cs, _ = R.cases()
    import workspace_ref as W
    for name, _, z, _, sizes in cs:
        n = len(z)
        got = R.lib_cell_doubles(n, sizes, host)
        assert got == R.cell_form(n, sizes, host), name
        assert got > W.cell_doubles(W.LOO, n, host=host)
    for n, sizes in [(3000, [3000]), (3000, [1] * 3000), (500, [125] * 4), (64, [64]), (1, [1])]:
        assert R.lib_cell_doubles(n, sizes, host) == R.cell_form(n, sizes, host), (n, len(sizes))
    assert R.lib_cell_doubles(0, [], host) == R.cell_form(0, [], host) == 2
    # one group, the worst case: the padded block and X, n^2 each, on leave-one-out's n^2
    assert 2.9 < R.lib_cell_doubles(3000, [3000], host) / W.cell_doubles(W.LOO, 3000, host=host) < 3.0
    assert R.lib_cell_doubles(10, [4, 5], host) == -1 and R.lib_cell_doubles(1, [0, 1], host) == -1


# -- gpr.site_groups ------------------------------------------------------------

def test_site_groups_joins_bitwise_equal_rows_per_cell():
    a, b, c = [1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [0.0, 2.0, 3.0]
    xyt = np.array([a, b, a, c, a, b,      # cell 0
                    a, a, [-0.0, 2.0, 3.0], c,    # cell 1: a again (another site there), -0.0 is not 0.0
                    ])
    offs = [0, 6, 6, 10]
    lab = gpr.site_groups(xyt, offs)
    assert lab.dtype == np.int64 and lab.tolist() == [0, 1, 0, 3, 0, 1, 6, 6, 8, 9]
    nan = np.array([[np.nan, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    assert gpr.site_groups(nan, [0, 2]).tolist() == [0, 0]
    assert gpr.site_groups(np.zeros((0, 3)), [0, 0]).shape == (0,)
    cs, _ = R.cases()
    x = next(c for c in cs if c[0] == 'n130-sites')[1]
    assert np.array_equal(gpr.site_groups(x, [0, len(x)]), R.site_labels(x))
    sizes = sorted(len(g) for g in R.groups_of(gpr.site_groups(x, [0, len(x)])))
    assert sizes == sorted(np.unique(x, axis=0, return_counts=True)[1].tolist())


# -- the ABI ------------------------------------------------------------------------

def test_symbol_exported_and_bound():
    assert 'oi_gpr_lgo' in _lib.SIGNATURES and abi_ref.nargs('oi_gpr_lgo') == 14 == len(_lib.SIGNATURES['oi_gpr_lgo'][1])
    assert {'oi_gpr_lgo', 'oi_test_lgo_plan', 'oi_test_lgo_cell_doubles'} <= abi_ref.exported()
    assert callable(_lib.gpr_lgo) and callable(_lib.gpr_lgo_device)
    assert callable(gpr.lgo_cells) and callable(gpr.site_groups) and callable(nystrom.GPR_lgo)


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None


def _i(*v):
    return np.array(v, dtype=np.int64)


def _call(lib, **over):
    """One cell with 3 observations in two groups; ``over`` replaces arguments."""
    a = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=_i(0, 3), ncell=1, group=_i(4, 9, 4), hyp=np.ones((1, 5)),
             mu=np.zeros(3), sd=np.zeros(3), lpd=np.zeros(3), d2=np.zeros(3), lpl=np.zeros(1),
             status=np.zeros(1, dtype=np.int32))
    a.update(over)
    return lib.oi_gpr_lgo(_p(a['xyt'], D), _p(a['z'], D), _p(a['offs'], I64), a['ncell'], _p(a['group'], I64), 0.0,
                          _p(a['hyp'], D), _p(a['mu'], D), _p(a['sd'], D), _p(a['lpd'], D), _p(a['d2'], D),
                          _p(a['lpl'], D), _p(a['status'], I32), None)


@pytest.mark.parametrize('over, word', [
    (dict(ncell=-1), b'ncell'),
    (dict(offs=None), b'null offs'),
    (dict(offs=_i(1, 3)), b'offs[0]'),
    (dict(offs=_i(0, 3, 2), ncell=2, hyp=np.ones((2, 5))), b'offs must be non-decreasing'),
    (dict(xyt=None), b'null xyt / z'),
    (dict(z=None), b'null xyt / z'),
    (dict(group=None), b'null group'),
    (dict(hyp=None), b'null hyp'),
    (dict(mu=None), b'null mu / sd'),
    (dict(sd=None), b'null mu / sd'),
    (dict(status=None), b'null status'),
    # Np^2 doubles reach 2 GiB from n = 16 321 (Np = 16 384); no array of that size is touched
    (dict(offs=_i(0, 16321)), b'cell too large'),
])
def test_misuse_is_oi_e_arg(over, word):
    lib = _lib.load()
    assert _call(lib, **over) == -1
    assert word in lib.oi_last_error()


def test_misuse_leaves_outputs_untouched_and_empty_batch_is_a_noop():
    lib = _lib.load()
    outs = {k: np.full(3, 7.0) for k in ('mu', 'sd', 'lpd', 'd2')}
    lpl = np.full(1, 7.0)
    assert _call(lib, offs=_i(1, 3), lpl=lpl, **outs) == -1
    assert all((v == 7.0).all() for v in outs.values()) and lpl[0] == 7.0
    assert _call(lib, ncell=0, offs=np.zeros(1, dtype=np.int64), xyt=None, z=None, group=None, hyp=None, mu=None,
                 sd=None, lpd=None, d2=None, lpl=None, status=None) == 0


def test_wrapper_rejects_inconsistent_batches():
    ok = dict(xyt=np.zeros((3, 3)), z=np.zeros(3), offs=[0, 3], group=[0, 0, 1], mean=0.0, hyp=np.ones((1, 5)))
    for over in (dict(hyp=np.ones((2, 5))), dict(offs=[0, 2]), dict(offs=[1, 3]), dict(xyt=np.zeros((2, 3))),
                 dict(group=[0, 1])):
        with pytest.raises(ValueError):
            _lib.gpr_lgo(**{**ok, **over})
