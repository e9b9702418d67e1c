"""oila::gemm / oila::gemv (csrc/oi_linalg.hip: k_gemm, k_gemm128, k_gemv_t,
k_gemv_n) against a longdouble product on the host, at the edges of the 64-
and 128-tiles, the 16-deep chunk and the element pairs.

The bound is derived, not measured: elementwise
    |C - C_ref| <= (k + 4) 2^-52 (|alpha| |op A| |op B| + |beta| |C0|)
(oila_ref.gemm_ref).  Every operand sits in a larger buffer whose pad rows and
guard band hold a NaN sentinel: the tests assert the sentinels bitwise (no
write outside the operand) and that every result is finite (no read outside).

Measured on an MI355X (printed as WORST with -s): the worst ratio
error / bound was 0.152 over the 58 gemm products and 0.119 / 0.114 over the
48 gemv products of each form (the worst are the shortest sums, where the
bound is a few roundings)."""
import os

import numpy as np
import pytest

import oila_ref as R

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 63, 64, 65, 127, 128, 129, 130)
KS = (1, 3, 15, 16, 17, 63, 64, 65, 130)
COEF = ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0))
FORMS = ((0, 0), (0, 1), (1, 0), (1, 1))


class Prod:
    """One product's operands on the device and its host reference."""

    def __init__(self, rng, m, n, k, ta, tb, pad=0, alpha=1.0, beta=0.0, tri=0, spread=False, c0=None):
        self.m, self.n, self.k, self.ta, self.tb, self.alpha, self.beta, self.tri = m, n, k, ta, tb, alpha, beta, tri
        opA, opB = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (k, n))
        if spread:   # entries over 1e+-8: the bound is relative to |A||B|, not to |C|
            opA = opA * 10.0 ** rng.uniform(-8, 8, opA.shape)
            opB = opB * 10.0 ** rng.uniform(-8, 8, opB.shape)
        self.opA, self.opB = opA, opB
        self.refB = opB            # what the reference multiplies by (tri == 2 differs)
        if c0 is None:             # beta == 0: C0 full of NaN must not reach the result
            c0 = np.full((m, n), np.nan) if beta == 0.0 else rng.uniform(-1, 1, (m, n))
        self.C0 = c0
        self.pad = pad
        self.A = self.B = self.C = None

    def upload(self):
        self.A = R.DevMat(self.opA.T if self.ta else self.opA, self.pad)
        self.B = R.DevMat(self.opB.T if self.tb else self.opB, self.pad)
        self.C = R.DevMat(self.C0, self.pad)
        return self

    def desc(self):
        return R.Gemm(self.A.ptr(), self.B.ptr(), self.C.ptr(), self.m, self.n, self.k, self.A.ld, self.B.ld,
                      self.C.ld, self.alpha, self.beta, self.tri)

    def ratio(self):
        """error / bound of the result (sentinels and finiteness asserted)."""
        return R.check_gemm(self.C.result(), self.opA, self.refB, self.C0, self.alpha, self.beta)


def run(prods):
    """One launch per transpose form over all products of that form."""
    for ta, tb in FORMS:
        batch = [p for p in prods if (p.ta, p.tb) == (ta, tb)]
        if batch:
            R.run_gemm([p.desc() for p in batch], ta, tb)


def selection():
    """54 (m, n, k) triples: every value of each dimension six times, every
    pair (m, n), (m, k), (n, k) of six cyclic offsets; the four forms, both
    pads and the three coefficient pairs cycle with coprime periods."""
    out = []
    for s in range(6):
        for i in range(9):
            idx = len(out)
            out.append((DIMS[i], DIMS[(i + s) % 9], KS[(i + 2 * s + 1) % 9], FORMS[idx % 4], 3 * ((idx // 4) % 2),
                        COEF[idx % 3]))
    return out


def test_selection_covers_the_issue():
    sel = selection()
    assert len(sel) <= 60
    assert {c[0] for c in sel} == set(DIMS) and {c[1] for c in sel} == set(DIMS) and {c[2] for c in sel} == set(KS)
    assert {c[3] for c in sel} == set(FORMS) and {c[4] for c in sel} == {0, 3} and {c[5] for c in sel} == set(COEF)
    assert {(c[3], c[5]) for c in sel} == {(f, c) for f in FORMS for c in COEF}
    assert {(c[3], c[4]) for c in sel} == {(f, q) for f in FORMS for q in (0, 3)}


def test_sizes_forms_coefficients():
    rng = np.random.default_rng(11)
    prods = [Prod(rng, m, n, k, ta, tb, pad, a, b).upload() for m, n, k, (ta, tb), pad, (a, b) in selection()]
    # entries spread over 1e+-8, one per form
    prods += [Prod(rng, 129, 63, 130, ta, tb, 3, 0.5, -2.0, spread=True).upload() for ta, tb in FORMS]
    run(prods)
    worst = 0.0
    for p in prods:
        r = p.ratio()
        worst = max(worst, r)
        assert r <= 1.0, (p.m, p.n, p.k, p.ta, p.tb, p.pad, p.alpha, p.beta, r)
    print(f"WORST gemm error / bound {worst:.3g} over {len(prods)} products")


def test_k0_and_empty_products():
    rng = np.random.default_rng(12)
    for ta, tb in FORMS:
        a = Prod(rng, 65, 33, 17, ta, tb, 3, -1.0, 1.0).upload()
        k0 = Prod(rng, 65, 33, 0, ta, tb, 3, 0.5, -2.0).upload()          # C = beta C0
        k0n = Prod(rng, 64, 2, 0, ta, tb, 0, 1.0, 0.0).upload()           # C = 0 over NaN
        m0 = Prod(rng, 0, 33, 17, ta, tb, 3, 1.0, 1.0).upload()
        n0 = Prod(rng, 65, 0, 17, ta, tb, 0, 1.0, 1.0).upload()
        b = Prod(rng, 130, 129, 65, ta, tb, 0, 0.5, -2.0).upload()
        run([a, k0, m0, k0n, n0, b])
        assert a.ratio() <= 1.0 and b.ratio() <= 1.0
        assert np.array_equal(k0.C.result(), -2.0 * k0.C0)
        assert np.array_equal(k0n.C.result(), np.zeros((64, 2)))
        for e in (m0, n0):
            assert (e.C.fetch()[1].view(np.uint64) == R.SENT_BITS).all()
    R.run_gemm([], 0, 0)   # an empty batch is a no-op


@pytest.mark.parametrize('tri', (1, 3))
def test_tri1_tri3_lower_only(tri):
    """tri == 1: the 64-tiles with row tile < column tile are not written, the
    others meet the bound.  tri == 3 (cholesky's update): nor are the entries
    above the diagonal inside the diagonal tiles."""
    rng = np.random.default_rng(13)
    for (m, n), (ta, tb) in zip(((130, 130), (129, 65), (65, 130), (64, 64)), FORMS):
        c0 = rng.uniform(-1, 1, (m, n))
        gm, gn = np.arange(m)[:, None], np.arange(n)[None, :]
        keep = (gm // 64 < gn // 64) | ((gm < gn) if tri == 3 else False)
        c0[keep] = R.SENT
        p = Prod(rng, m, n, 17, ta, tb, 3, -1.0, 1.0, tri=tri, c0=c0).upload()
        run([p])
        C = p.C.result()
        assert (C.view(np.uint64)[keep] == R.SENT_BITS).all(), "an entry outside the lower part was written"
        low = ~keep
        ref, bound = R.gemm_ref(p.opA, p.opB, np.where(low, c0, 0.0), -1.0, 1.0)
        assert np.isfinite(C[low]).all()
        assert (np.abs(C[low].astype(R.LD) - ref[low]) <= bound[low]).all()


def test_tri2_upper_triangular_B_is_not_read_below():
    rng = np.random.default_rng(14)
    for ta, tb in FORMS:
        p = Prod(rng, 65, 130, 130, ta, tb, 3, 1.0, 0.0, tri=2)
        kk, jt = np.arange(130)[:, None], np.arange(130)[None, :] // 64
        dead = kk >= 64 * (jt + 1)
        assert dead.any()
        p.refB = np.where(dead, 0.0, p.opB)
        p.opB = np.where(dead, np.nan, p.opB)     # uploaded with NaN where the kernel must not read
        p.upload()
        run([p])
        p.opB = p.refB
        assert p.ratio() <= 1.0, (ta, tb)


def test_routing_128_and_64_tiles_bitwise_equal():
    shapes = ((128, 128, 64), (129, 257, 65), (255, 130, 130))
    old = os.environ.get('OI_GEMM128')
    try:
        for ta, tb in FORMS:
            def batch(extra=False):
                r2 = np.random.default_rng(150)
                ps = [Prod(r2, m, n, k, ta, tb, 3 * (i % 2), -1.0, 1.0).upload() for i, (m, n, k) in enumerate(shapes)]
                if extra:   # one small product keeps the whole batch on the 64-tiles
                    ps.append(Prod(r2, 65, 64, 64, ta, tb, 0, 1.0, 0.0).upload())
                return ps
            os.environ.pop('OI_GEMM128', None)
            wide = batch()
            run(wide)
            os.environ['OI_GEMM128'] = '0'
            narrow = batch()
            run(narrow)
            os.environ.pop('OI_GEMM128', None)
            mixed = batch(extra=True)
            run(mixed)
            for a, b, c in zip(wide, narrow, mixed):
                Ca, Cb, Cc = a.C.result(), b.C.result(), c.C.result()
                assert a.ratio() <= 1.0
                assert np.array_equal(Ca.view(np.uint64), Cb.view(np.uint64)), (ta, tb, a.m, a.n, a.k)
                assert np.array_equal(Ca.view(np.uint64), Cc.view(np.uint64)), (ta, tb, a.m, a.n, a.k)
            assert mixed[-1].ratio() <= 1.0
    finally:
        if old is None:
            os.environ.pop('OI_GEMM128', None)
        else:
            os.environ['OI_GEMM128'] = old


def test_batch_independence():
    shapes = ((129, 65, 17), (1, 1, 1), (64, 64, 16), (130, 2, 63), (63, 127, 15), (128, 128, 64), (2, 130, 3),
              (65, 129, 130))
    for ta, tb in FORMS:
        def make():
            r2 = np.random.default_rng(16)
            return [Prod(r2, m, n, k, ta, tb, 3 * (i % 2), *COEF[i % 3]).upload() for i, (m, n, k) in enumerate(shapes)]
        together = make()
        run(together)
        alone = make()
        for p in alone:
            run([p])
        for a, b in zip(together, alone):
            assert np.array_equal(a.C.result().view(np.uint64), b.C.result().view(np.uint64)), (ta, tb, a.m, a.n, a.k)
            assert a.ratio() <= 1.0


def test_in_place_panel_product():
    """C aliasing A with one column tile and B transposed, as cholesky's panel
    step and trsm_right_lt's scaling use it."""
    rng = np.random.default_rng(17)
    descs, cases = [], []
    for m in (65, 130):
        for n in (64, 33):
            X = rng.uniform(-1, 1, (m, n))
            Bt = rng.uniform(-1, 1, (n, n))        # stored n x k: op(B) = Bt'
            x = R.DevMat(X, 3)
            b = R.DevMat(Bt, 0)
            descs.append(R.Gemm(x.ptr(), b.ptr(), x.ptr(), m, n, n, x.ld, b.ld, x.ld, 1.0, 0.0, 0))
            cases.append((x, X, Bt, b))     # b stays alive until the launch has run
    R.run_gemm(descs, 0, 1)
    for x, X, Bt, _ in cases:
        assert R.check_gemm(x.result(), X, Bt.T, None, 1.0, 0.0) <= 1.0


GV_M = (1, 63, 64, 65, 130, 257)
GV_N = (1, 3, 4, 5, 15, 16, 17, 65)


@pytest.mark.parametrize('trans', (0, 1))
def test_gemv(trans):
    """n < 16 leaves waves of k_gemv_n without columns; n not a multiple of 4
    leaves waves of k_gemv_t without an output."""
    rng = np.random.default_rng(18 + trans)
    descs, cases = [], []
    for i, (m, n) in enumerate((m, n) for m in GV_M for n in GV_N):
        alpha, beta = COEF[i % 3]
        A = rng.uniform(-1, 1, (m, n))
        nx, ny = (m, n) if trans else (n, m)
        x = rng.uniform(-1, 1, nx)
        y0 = np.full(ny, np.nan) if beta == 0.0 else rng.uniform(-1, 1, ny)
        dA, dx, dy = R.DevMat(A, 3 * ((i // 3) % 2)), R.DevMat(x), R.DevMat(y0, 3 * (i % 2))
        descs.append(R.Gemv(dA.ptr(), dx.ptr(), dy.ptr(), m, n, dA.ld, alpha, beta))
        cases.append((dy, A.T if trans else A, x, y0, alpha, beta, (dA, dx)))   # operands stay alive
    # empty operands in the batch are skipped
    e = R.DevMat(np.zeros((0, 4)), 3)
    ey = R.DevMat(np.zeros(4 if trans else 0), 3, fill=R.SENT)
    descs.insert(5, R.Gemv(e.ptr(), e.ptr(), ey.ptr(), 0, 4, e.ld, 1.0, 1.0))
    R.run_gemv(descs, trans)
    worst = 0.0
    for dy, opA, x, y0, alpha, beta, _ in cases:
        r = R.check_gemm(dy.result(), opA, x[:, None], y0[:, None], alpha, beta)
        worst = max(worst, r)
        assert r <= 1.0, (trans, opA.shape, alpha, beta, r)
    assert (ey.fetch()[1].view(np.uint64) == R.SENT_BITS).all()
    print(f"WORST gemv(trans={trans}) error / bound {worst:.3g} over {len(cases)} products")
