"""oila::eigh (csrc/oi_linalg.hip: tridiagonalisation, bisection, inverse
iteration, orthogonalisation, back-transform) against numpy's eigh and
longdouble residuals on the host, on thirteen families of spectra -- among
them clusters of equal eigenvalues at the top and in the middle of the
spectrum, which the Nystrom variant's K_mm matrices never show.

Checks (oila_ref.eigh_ratios, formed in longdouble): w ascending,
|w - w_numpy| <= T M eps ||A||_2, max|U'U - I| <= T M eps,
max|A U - U diag(w)| <= T M eps ||A||_2, info == 0; for the zero matrix
|w| <= 1e-300 and the orthogonality check.  T = 4: numpy's own eigh stays at or
below 1 in these units on the same generators and the CPU model of the kernels
at or below 1.73 (tests/test_oila_ref.py asserts both); the rest covers the
kernels' different reduction order.

Measured worst ratios (eigenvalues, orthogonality, residual):
    numpy (CPU)                 0.83  0.96  0.92
    model (CPU, M <= 65)        1.30  0.85  1.73
    kernels (MI355X)            1.30  1.09  1.73
(the kernels' worst are at M = 1 and M = 3, where M eps is a few roundings; from
M = 31 on they stay below 0.36, 0.28 and 0.41 -- nothing above 2 to attribute).
Before the weak / collapse rules of k_mgs_panel the same kernels gave, on the
MI355X, a residual of 8.2e12 .. 4.9e13 on the projector family at every
M >= 31 (orthogonality and eigenvalues fine, info 0); the other two cluster
families passed there with these seeds (residual <= 0.3 from M = 31 on), while
the CPU model without the rules also fails on triples at M = 33, 64, 65
(5e12 .. 4e13) and, with them but without the weak rule, loses orthogonality
(9.8) on triples at M = 64.  A NaN entry used to give finite eigenvalues
(fmin / fmax in the Gershgorin bounds drop NaN); k_stebz now propagates it.
The workspace is handed over full of NaN: nothing may be read from it before
it is written."""
import numpy as np
import pytest

import oila_ref as R

pytestmark = pytest.mark.gpu


class Prob:
    def __init__(self, A, pad=0, with_info=True):
        import torch
        self.A0 = A
        self.M = M = A.shape[0]
        self.A = R.DevMat(A, pad)
        self.w = R.DevMat(np.zeros(M), 0, fill=R.SENT)
        n = R.lib().oila_test_eigh_workspace_doubles(M)
        self.work = torch.full((n + 8,), float('nan'), dtype=torch.float64, device='cuda')
        self.info = R.dev_ints([0, -7]) if with_info else None

    def desc(self):
        return R.Eigh(self.A.ptr(), self.w.ptr(), self.work.data_ptr(), self.M, self.A.ld,
                      self.info.data_ptr() if self.info is not None else None)

    def fetch(self):
        self.U = self.A.result()
        self.wv = self.w.result()[:, 0]
        if self.info is not None:
            i = self.info.cpu().numpy()
            assert i[1] == -7
            self.info_v = int(i[0])
        return self


def solve(probs):
    R.run_eigh([p.desc() for p in probs])
    return [p.fetch() for p in probs]


_cache = {}


def per_size(M):
    """Every family at size M in one launch (computed once per size)."""
    if M not in _cache:
        _cache[M] = dict(zip(R.EIGH_FAMILIES, solve([Prob(R.eigh_matrix(f, M)) for f in R.EIGH_FAMILIES])))
    return _cache[M]


@pytest.mark.parametrize('M', R.EIGH_SIZES)
def test_families(M):
    worst = np.zeros(3)
    fails = []
    for f, p in per_size(M).items():
        try:
            r = R.check_eigh(p.A0, p.wv, p.U, what=f"{f} M={M}")
            assert p.info_v == 0, f"{f} M={M}: info {p.info_v}"
        except AssertionError as e:
            fails.append(str(e))
            try:
                r = R.eigh_ratios(p.A0, p.wv, p.U)
            except AssertionError:
                continue
        if np.any(p.A0):
            worst = np.maximum(worst, r)
        print(f"EIGH M={M} {f}: eigenvalues {r[0]:.3g} orthogonality {r[1]:.3g} residual {r[2]:.3g}")
    print(f"EIGH M={M} WORST: eigenvalues {worst[0]:.3g} orthogonality {worst[1]:.3g} residual {worst[2]:.3g}")
    assert not fails, fails


def test_mixed_sizes_pads_and_null_info():
    probs = []
    for i, M in enumerate((3, 33, 64, 130)):
        for pad in (0, 3):
            f = R.EIGH_FAMILIES[(3 * i + pad) % len(R.EIGH_FAMILIES)]
            probs.append(Prob(R.eigh_matrix(f, M), pad, with_info=not (M == 33 and pad == 3)))
        probs.append(Prob(R.eigh_matrix('triples', M), 3))
    for p in solve(probs):
        R.check_eigh(p.A0, p.wv, p.U, what=f"mixed M={p.M}")
        assert p.info is None or p.info_v == 0


def test_nan_input_propagates():
    A = R.eigh_matrix('goe', 33)
    A[20, 4] = A[4, 20] = np.nan
    good = R.eigh_matrix('goe', 33)
    pn, pg = Prob(A), Prob(good)
    R.run_eigh([pn.desc(), pg.desc()])       # the launch returns
    pn.info_v = int(pn.info.cpu().numpy()[0])
    w, U = pn.w.result(), pn.A.result()
    assert np.isnan(w).any() and np.isnan(U).any()
    assert pn.info_v == 0, "info is left untouched by NaN input"
    pg.fetch()
    R.check_eigh(good, pg.wv, pg.U, what="neighbour of the NaN matrix")


@pytest.mark.parametrize('M', (33, 130))
def test_batch_independence(M):
    for f in ('goe', 'triples', 'matern_dup'):
        alone = solve([Prob(R.eigh_matrix(f, M))])[0]
        inb = per_size(M)[f]
        assert np.array_equal(alone.wv.view(np.uint64), inb.wv.view(np.uint64)), (f, M)
        assert np.array_equal(alone.U.view(np.uint64), inb.U.view(np.uint64)), (f, M)
