"""The float64 Nystrom oracle (oracle/nystrom_oracle.py) against a 60-digit
mpmath restatement of the same quantities at edge shapes (M = 1, M = n,
M = 32 | 33, n = 65) and three hyper sets, one of them with K_mm = sf2 I
exactly (an M-fold eigenvalue cluster).

The restatement shares no step with the oracle beyond the kernel's formula:
no eigendecomposition, no clamp, no Woodbury chain through u / s --
  G  = sn2 Kmm + Kmn Knm
  Ki = (I - Knm G^-1 Kmn) / sn2
  slogdet(H) / 2 = (log det G - log det Kmm) / 2
  nlZ = y' Ki y / 2 + slogdet(H) / 2 + n log(2 pi) / 2
  Q = Ki - A A',  A = Ki y;  dnlZ_d = sum(Q dK_d) / 2, dnlZ_3 = sum(Q 2K) / 2, dnlZ_4 = sn2 tr Q
  fs = mean + k*' A;  sd = sqrt(sf2 - k*' Ki k*)
on the oracle's own float64 inputs (sites, y, exp(h)).  The oracle must be
within 1e-13 of it on the scales of tests/nystrom_cases.assert_cell: three
orders inside the 1e-10 bars the GPU path is held to, so those bars measure
the GPU code and not the reference.  Measured: nlZ <= 2.6e-15, gradient
<= 2.9e-15, fs <= 2.9e-16, sd <= 5.3e-15.
"""
import numpy as np
import pytest

import nystrom_cases as C

mp = pytest.importorskip('mpmath')

SHAPES = ((1, 1), (3, 2), (33, 32), (65, 1), (65, 65), (70, 33))
TOL = 1e-13
_worst = C.Worst()


def _kernel(xa, xb, ell, sf2, want_dk=False):
    """sf2 (1 + Q) exp(-Q), Q = sqrt(3) |(a - b) / ell|, and with want_dk the
    three sf2 q_d^2 exp(-Q), q_d = sqrt(3) |a_d - b_d| / ell_d."""
    K = mp.matrix(len(xa), len(xb))
    dK = [mp.matrix(len(xa), len(xb)) for _ in range(3)] if want_dk else None
    for i, a in enumerate(xa):
        for j, b in enumerate(xb):
            q2 = [3 * ((a[d] - b[d]) / ell[d]) ** 2 for d in range(3)]
            Q = mp.sqrt(q2[0] + q2[1] + q2[2])
            e = mp.exp(-Q)
            K[i, j] = sf2 * (1 + Q) * e
            if want_dk:
                for d in range(3):
                    dK[d][i, j] = sf2 * q2[d] * e
    return (K, dK) if want_dk else K


def _logdet(A):
    L = mp.cholesky(A)
    return 2 * sum(mp.log(L[i, i]) for i in range(A.rows))


def _restated(h, x, y, M):
    n = len(y)
    hyp = [mp.mpf(float(v)) for v in np.exp(h)]          # the oracle's own float64 hypers
    ell, sf2, sn2 = hyp[:3], hyp[3], hyp[4]
    X = [[mp.mpf(float(v)) for v in row] for row in x]
    yv = mp.matrix([mp.mpf(float(v)) for v in y])
    sel = [int(i) for i in C.N.inducing_indices(n, M)]
    Xm = [X[i] for i in sel]
    K, dK = _kernel(X, X, ell, sf2, want_dk=True)
    Kmm = _kernel(Xm, Xm, ell, sf2)
    Knm = _kernel(X, Xm, ell, sf2)
    G = sn2 * Kmm + Knm.T * Knm
    Ki = (mp.eye(n) - Knm * mp.inverse(G) * Knm.T) / sn2
    A = Ki * yv
    nlz = (yv.T * A)[0] / 2 + (_logdet(G) - _logdet(Kmm)) / 2 + n * mp.log(2 * mp.pi) / 2
    Q = Ki - A * A.T
    dot = lambda P, R: sum(P[i, j] * R[i, j] for i in range(n) for j in range(n))
    grad = [dot(Q, dK[d]) / 2 for d in range(3)] + [dot(Q, 2 * K) / 2, sn2 * sum(Q[i, i] for i in range(n))]
    ks = _kernel(X, [[mp.mpf(float(v)) for v in C.XS[0]]], ell, sf2)
    fs = mp.mpf(C.MEAN) + (ks.T * A)[0]
    arg = sf2 - (ks.T * Ki * ks)[0]
    sd = mp.sqrt(arg) if arg >= 0 else mp.nan
    return nlz, grad, fs, sd, mp.sqrt(sf2), arg / sf2


def _err(got, ref):
    """|got - ref| / max(1, |ref|) formed in mpmath."""
    return float(abs(mp.mpf(float(got)) - ref) / max(mp.mpf(1), abs(ref)))


@pytest.mark.parametrize('hname', sorted(C.HYPERS))
@pytest.mark.parametrize('n,M', SHAPES)
def test_oracle_matches_mpmath(n, M, hname):
    mp.mp.dps = 60
    h = C.HYPERS[hname]
    x, y = C.cell(n, C.cell_seed(n, M))
    nlz, grad, fs, sd, sp = C.oracle_cell(h, x, y, M)
    rn, rg, rfs, rsd, rsp, margin = _restated(h, x, y, M)
    assert abs(margin) >= 1e-6, "sd's argument is at rounding level: choose another seed"
    gscale = max(mp.mpf(1), max(abs(v) for v in rg))
    err = {'nlz': _err(nlz, rn),
           'grad': float(max(abs(mp.mpf(float(g)) - r) for g, r in zip(grad, rg)) / gscale),
           'fs': _err(fs, rfs), 'sprior': _err(sp, rsp)}
    assert np.isnan(sd) == mp.isnan(rsd), (sd, rsd, float(margin))
    err['sd'] = 0.0 if np.isnan(sd) else _err(sd, rsd)
    print(f"n={n} M={M} {hname}: " + ' '.join(f"{q} {e:.2e}" for q, e in err.items())
          + f" | sd {'NaN' if np.isnan(sd) else 'finite'}, (sf2 - err)/sf2 = {float(margin):.3g}")
    _worst.add({q: e / TOL for q, e in err.items()}, f"({n},{M}) {hname}")
    for q, e in err.items():
        assert e <= TOL, (q, e)


def test_every_gpu_case_is_decidable():
    """The screen of the GPU tests, run here on every case they use: none has
    sd's argument sf2 - err within 1e-6 sf2 of zero, so no case is dropped and
    sd is NaN in the oracle exactly where that argument is negative -- by
    arithmetic, not by rounding."""
    cases = [c for h in C.HYPERS.values() for c in C.edge_cases(h)] + C.chunk_cases() + C.fit_cases()
    C.screen(cases)
    nans = []
    for c in cases:
        m = C.sd_margin(c.h, c.x, c.y, c.M)
        assert np.isnan(C.reference(c)[3]) == (m < 0), (c, m)
        if m < 0:
            nans.append((c.n, c.M, round(m, 3)))
    print(f"{len(cases)} cases, sd NaN (n, M, (sf2 - err)/sf2):", nans)
    assert nans and len(nans) < len(cases)


def test_worst_ratios_report():
    """Prints the worst oracle error / 1e-13 per quantity over the cases above."""
    if _worst.w:
        _worst.report("oracle vs mpmath, worst error / 1e-13")
        assert all(r <= 1.0 for r, _ in _worst.w.values())
