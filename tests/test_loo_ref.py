"""The leave-one-out reference against itself, without a GPU: the closed form
(tests/loo_ref.py ``loo_closed``, one factorisation) against what it stands for
(``loo_brute``, n fits of n - 1 observations) on the cells of gpr3d.npz.

Bounds: mu within 1e-11 max(1, |mu|), sd within 1e-11 sd.  Measured: <= 2.7e-15
and <= 1.1e-14 relative, the cells' condition numbers reaching 2e3.
"""
import numpy as np
import pytest

from conftest import load_golden, ragged_cell
import loo_ref as R

TOL = 1e-11


def test_closed_form_equals_n_refits():
    d = load_golden('gpr3d.npz')
    mean = float(d['mean'])
    seen = 0
    for c in range(len(d['offs']) - 1):
        x, z = ragged_cell(d, c)
        if not 2 <= len(z) <= 200:
            continue
        seen += 1
        mu, sd, lpl = R.loo_closed(x, z, mean, d['hyp2'][c])
        bmu, bsd, blpl = R.loo_brute(x, z, mean, d['hyp2'][c])
        emu = np.max(np.abs(mu - bmu) / np.maximum(1.0, np.abs(bmu)))
        esd = np.max(np.abs(sd - bsd) / bsd)
        print(f"cell {c}: n {len(z)} |dmu| {emu:.2e} |dsd|/sd {esd:.2e} |dlpl| {abs(lpl - blpl):.2e}")
        assert np.all(np.abs(mu - bmu) <= TOL * np.maximum(1.0, np.abs(bmu))), c
        assert np.all(np.abs(sd - bsd) <= TOL * bsd), c
    assert seen >= 3   # (lpl is the same function of z, mu and sd in both: printed, not bounded)


def test_one_observation_is_the_prior():
    hyp = np.array([2e5, 2e5, 6.0, 5e-3, 1e-3])
    for f in (R.loo_closed, R.loo_brute):
        mu, sd, lpl = f(np.array([[1e5, 2e5, 3.0]]), np.array([0.7]), 0.3, hyp)
        assert abs(mu[0] - 0.3) <= 1e-15 and abs(sd[0] - np.sqrt(6e-3)) <= 1e-16
        want = -0.5 * np.log(2 * np.pi) - np.log(np.sqrt(6e-3)) - 0.4 ** 2 / (2 * 6e-3)
        assert abs(lpl - want) <= 1e-12 * abs(want)


def test_no_observation():
    mu, sd, lpl = R.loo_closed(np.zeros((0, 3)), np.zeros(0), 0.3, np.ones(5))
    assert mu.shape == (0,) and sd.shape == (0,) and lpl == 0.0


def test_non_pd_cell_raises():
    d = load_golden('gpr3d.npz')
    c = int(np.argmax(np.diff(d['offs']) >= 2))
    x, z = ragged_cell(d, c)
    hyp = d['hyp2'][c].copy()
    hyp[4] = -2.0 * hyp[3]  # first pivot sf2 + sn2 <= 0
    for f in (R.loo_closed, R.loo_brute):
        with pytest.raises(np.linalg.LinAlgError):
            f(x, z, float(d['mean']), hyp)
