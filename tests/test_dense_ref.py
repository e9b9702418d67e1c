"""The harness of the per-tile dense-kernel tests (tests/dense_ref.py) checked
on the CPU: the cell generator gives the shapes it is asked for, the
longdouble reference reproduces the oracle's nlZ / gradient / prediction from
its per-tile partials, and the checker flags a corrupted state at exactly the
corrupted place -- and nothing in a faultless one."""
import ctypes

import numpy as np
import pytest

import dense_ref as R
from oracle import gp_oracle as O

HYP = (2e5, 2.5e5, 7.0, 4e-3, 1e-3)
HYP_ANISO = (9e4, 3e5, 3.0, 1e-2, 2e-3)


@pytest.mark.parametrize('T,rT,extra', [(1, 1, 0), (1, 64, 0), (2, 1, 0), (2, 63, 37), (3, 16, 5), (5, 17, 0),
                                        (13, 17, 100)])
def test_generator_yields_the_requested_shape(T, rT, extra):
    rc = R.shape_cell(T, rT, extra=extra, seed=3)
    m = 64 * (T - 1) + rT
    assert R.site_counts(rc) == [(m + extra, m, T, rT)]
    x, z, xs = rc.cell(0)
    assert len(z) == m + extra and not np.signbit(x).any()
    # lattice sites inside the disc; every site observed at least once, repeats where asked for
    assert np.all(x[:, :2] % 25e3 == 0) and np.all(x[:, 2] == np.round(x[:, 2]))
    assert np.all(np.hypot(x[:, 0] - xs[0, 0], x[:, 1] - xs[0, 1]) <= 300e3)
    c = R.Cell(rc, HYP)
    assert (c.m, c.T, c.rT, c.n_obs) == (m, T, rT, m + extra)
    assert np.isclose(np.sum(c.dw ** 2), m + extra) and (extra == 0) == bool(np.all(c.dw == 1.0))
    if extra == 0:
        assert np.array_equal(c.sites, x) and np.array_equal(c.v, z - rc.mean) and c.ssw == 0.0
    # another seed, another cell; the same seed, the same cell
    assert np.array_equal(R.shape_cell(T, rT, extra=extra, seed=3).xyt, rc.xyt)
    if m > 1:
        assert not np.array_equal(R.shape_cell(T, rT, extra=extra, seed=4).xyt, rc.xyt)


def test_generator_off_lattice_and_batches():
    rc = R.exact_cell(5000, 5000, seed=1, lattice=False)
    assert R.site_counts(rc) == [(5000, 5000, 79, 8)]
    with pytest.raises(AssertionError):
        R.exact_cell(5000, 5000, seed=1)          # more than the lattice holds
    b = R.exact_cells([63, 64, (65, 80), 129], seed=2)
    assert R.site_counts(b) == [(63, 63, 1, 63), (64, 64, 1, 64), (80, 65, 2, 1), (129, 129, 3, 1)]


def test_dedup_restatement():
    xyt = np.array([[1., 2, 3], [4, 5, 6], [1, 2, 3], [7, 8, 9], [4, 5, 6], [1, 2, 3]])
    r = np.array([.1, .2, .3, .4, .5, .6])
    sites, v, d, ssw, sabs, sid, fo = R.dedup_np(xyt, r)
    assert np.array_equal(sites, xyt[[0, 1, 3]]) and np.array_equal(sid, [0, 1, 0, 2, 1, 0])
    assert np.array_equal(d, np.sqrt([3., 2, 1])) and np.array_equal(v, [((.1 + .3) + .6) / np.sqrt(3.), (.2 + .5) / np.sqrt(2.), .4])
    mean0 = ((.1 + .3) + .6) / 3
    assert np.isclose(ssw, (.1 - mean0) ** 2 + (.3 - mean0) ** 2 + (.6 - mean0) ** 2 + 2 * .15 ** 2, rtol=1e-14)


def test_cell_record_matches_the_compiled_struct():
    assert ctypes.sizeof(R.OiCell) == R.lib().oi_test_sizeof_cell() == 184
    assert R.OiCell.n.offset == 80 and R.OiCell.hyp.offset == 96 and R.OiCell.ssw.offset == 168


def test_round_order_is_the_engines():
    class C:
        def __init__(self, T, mode):
            self.T, self.mode = T, mode
    cells = [C(2, 1), C(5, 0), C(5, 1), C(1, 0), C(7, 1), C(5, 0)]
    al, ev = R.round_order(cells)
    assert ev == [1, 5, 3] and al == [4, 1, 5, 2, 0, 3]


@pytest.fixture(scope='module')
def refs():
    out = {}
    for name, T, rT, extra, hyp in (('plain', 3, 17, 0, HYP), ('dup', 2, 33, 37, HYP), ('aniso', 2, 16, 11, HYP_ANISO)):
        rc = R.shape_cell(T, rT, extra=extra, seed=7)
        out[name] = (rc, R.Ref(R.Cell(rc, hyp)))
    return out


@pytest.mark.parametrize('name', ['plain', 'dup', 'aniso'])
def test_reference_reproduces_the_oracle(refs, name):
    """Summed per-tile partials, logdet and quad against the oracle's n x n
    computation (duplicates included: the (n - m) and SSW terms), to 1e-12 of
    the scales tests/test_gpu_parity.py uses at 1e-10."""
    rc, ref = refs[name]
    c = ref.cell
    x, y, xs = rc.cell(0)
    h = np.concatenate([np.log(c.hyp), [0.0]])
    mX = np.full(len(y), rc.mean)
    f, g = O.neg_log_ml(h, x, y, mX)
    f = float(np.asarray(f).item())
    nlz, gr = ref.out_eval()
    assert abs(float(nlz) - f) <= 1e-12 * max(1.0, abs(f)), (float(nlz), f)
    S = np.abs(g) + R.grad_scale(h, x, y, mX)
    err = np.abs(np.asarray(gr, dtype=np.float64) - g)
    assert np.all(err <= 1e-12 * S), (err / S)
    fs, sd, lZ = O.predict(x, y, xs, rc.mean, c.hyp[:3], c.hyp[3], c.hyp[4])
    for got, want in zip(ref.out_predict(), (fs[0], sd[0], lZ)):
        assert abs(float(got) - want) <= 1e-12 * max(1.0, abs(want)), (float(got), want)
    # the yardstick: plain fp64 LAPACK sits within a few hundred eps of the reference
    assert all(R.EPS <= e <= 1e-12 for e in ref.err64.values()), ref.err64


@pytest.mark.parametrize('mode', [R.MODE_EVAL, R.MODE_PREDICT])
def test_checker_passes_a_faultless_state(refs, mode):
    for name in refs:
        ref = refs[name][1]
        rep = R.compare(ref.as_state(mode), ref)
        assert not rep.findings, rep
        want = set(R.QUANTITIES) - ({'v'} if mode == R.MODE_EVAL else {'W', 'alpha', 'grad'})
        assert set(rep.ratios) == want and max(rep.ratios.values()) <= 1.0, rep.ratios


def test_checker_flags_exactly_the_corrupted_place(refs):
    ref = refs['plain'][1]            # T = 3, rT = 17: m = 145
    T, nt = 3, 6
    good = ref.as_state(R.MODE_EVAL)

    def keys(mutate, mode=R.MODE_EVAL):
        st = ref.as_state(mode)
        mutate(st)
        return R.compare(st, ref).keys()

    # one 16 x 16 block of one L tile, 1e-9 relative
    def blk(st):
        st.L[R.tri(2) + 1][16:32, 32:48] *= 1 + 1e-9
    assert keys(blk) == [('L', 2, 1, (1, 2))]
    # one padding element (row 148 >= m of the last diagonal tile)
    def pad(st):
        st.L[R.tri(2) + 2][20, 5] = 1e-300
    assert keys(pad) == [('L.pad', 2, 2, (1, 0))]
    def pad1(st):
        st.W[R.tri(2) + 2][40, 40] = np.nextafter(1.0, 2.0)     # the padding identity
    assert keys(pad1) == [('W.pad', 2, 2, (2, 2))]
    def padz(st):
        st.vec[R.NB * T + 150] = -1e-320                           # alpha's padding
    assert keys(padz) == [('alpha.pad', 2, None, (1, None))]
    # above the diagonal of a diagonal tile
    def up(st):
        st.Dinv[1][3, 60] = 1e-30
    assert keys(up) == [('Dinv.upper', 1, 1, (0, 3))]
    # one guard word
    def guard(st):
        st.W[nt + 1][3, 4] = 0.0
    assert keys(guard) == [('W.guard', 1, None, None)]
    def guard2(st):
        st.part[R.part_size(T) + 5] = good.part[0]
    assert keys(guard2) == [('part.guard', 0, None, None)]
    # a write where no kernel writes: the kstar slot
    def kstar(st):
        st.vec[2 * R.NB * T + 17] = 0.5
    assert keys(kstar) == [('vec.untouched', 1, None, None)]
    # two swapped gradient partials of tile (2, 1)
    def swap(st):
        x = 5 * (R.tri(2) + 1)
        st.part[x], st.part[x + 1] = st.part[x + 1], st.part[x]
    assert keys(swap) == [('grad', 2, 1, (0, None)), ('grad', 2, 1, (1, None))]
    # a NaN that is read; a sentinel left where a value belongs
    def nan(st):
        st.vec[70] = np.nan
    assert keys(nan) == [('z', 1, None, (0, None))]
    def unwritten(st):
        st.part[R.part_logdet(T) + 2] = R.SENT
    assert keys(unwritten) == [('logdet', 2, None, (0, None))]
    def vpred(st):
        st.vec[3 * R.NB * T + 5] *= 1 + 1e-9
    assert keys(vpred, R.MODE_PREDICT) == [('v', 0, None, (0, None))]
    # bit comparison of whole states
    other = good.copy()
    assert good.same_bits(other) and not good.poisoned()
    other.Dinv[0][0, 0] = np.nextafter(other.Dinv[0][0, 0], 0)
    assert not good.same_bits(other)
