"""The numpy reference of ``oi_gpr_sample`` (tests/sample_ref.py) on its own:
the generator's known answers and counter layout, the moments of the normals
it maps to, and the draw's covariance.  No GPU needed."""
import numpy as np
import pytest

from optimalinterpolation_amd import synthetic
import sample_ref as R

HYP = np.array([2e5, 2e5, 6.0, 5e-3, 1e-3])   # the hypers of scripts/loo_timing.py


def _hex(words):
    return ' '.join(f'{int(w):08x}' for w in words)


@pytest.mark.parametrize('counter, key, words', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_known_answers(counter, key, words):
    assert _hex(R.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))) == words


def test_block_index_carries_into_counter_word_1():
    """Elements 2^33 - 3 .. 2^33 + 2 are blocks 2^32 - 2 .. 2^32 + 1: the last
    two have counter word 0 = 0, 1 and word 1 = 1."""
    seed, stream, first = 7, 9, 2 ** 33 - 3
    w = R.block_words(seed, stream, (np.arange(6, dtype=np.uint64) + np.uint64(first)) >> np.uint64(1))
    key = np.array([7, 0], dtype=np.uint64)
    for row, ctr in zip(w[[0, 1, 3, 5]], [(0xFFFFFFFE, 0, 9, 0), (0xFFFFFFFF, 0, 9, 0), (0, 1, 9, 0), (1, 1, 9, 0)]):
        assert np.array_equal(row, R.philox4x32_10(np.array(ctr, dtype=np.uint64), key))
    assert np.array_equal(w[1], w[2]) and np.array_equal(w[3], w[4])      # two elements per block
    z, _ = R.normals(seed, stream, first, 6)
    lo, _ = R.normals(seed, stream, first - 2 ** 32, 6)                    # the same word 0, word 1 = 0
    assert np.isfinite(z).all() and not np.any(z == lo)


def test_stream_and_seed_reach_their_words():
    b = np.arange(64, dtype=np.uint64)
    seed, stream = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    w = R.block_words(seed, stream, b)
    ctr = np.stack([b, np.zeros_like(b), np.full_like(b, 0x76543210), np.full_like(b, 0xFEDCBA98)], axis=-1)
    assert np.array_equal(w, R.philox4x32_10(ctr, np.array([0x89ABCDEF, 0x01234567], dtype=np.uint64)))
    # one bit of either, low word or high word, changes every block
    for bit in (0, 31, 32, 63):
        for other in (R.block_words(seed ^ (1 << bit), stream, b), R.block_words(seed, stream ^ (1 << bit), b)):
            assert np.all(np.any(other != w, axis=-1))


def test_moments_of_the_reference_normals():
    """Conditions on the mapping, not measurements: at seed 20181205, stream 3,
    nt = 121, nsamp = 256 every standardised moment is below 4, the KS
    distance x sqrt(N) below 1.63 (the 1 % point) and the largest off-diagonal
    entry of Xi Xi' / S x sqrt(S) below 6."""
    from math import erf
    nt, S = 121, 256
    xi = R.cell_xi(20181205, 3, nt, S)
    z = xi.ravel()
    N = z.size
    m = z.mean()
    c = z - m
    var = (c ** 2).mean()
    skew = (c ** 3).mean() / var ** 1.5
    kurt = (c ** 4).mean() / var ** 2 - 3.0
    std = np.array([m * np.sqrt(N), (var - 1.0) * np.sqrt(N / 2.0), skew * np.sqrt(N / 6.0), kurt * np.sqrt(N / 24.0)])
    zs = np.sort(z)
    cdf = np.array([0.5 * (1.0 + erf(v / np.sqrt(2.0))) for v in zs])
    ks = max(np.max(np.arange(1, N + 1) / N - cdf), np.max(cdf - np.arange(N) / N)) * np.sqrt(N)
    G = xi @ xi.T / S
    off = np.max(np.abs(G - np.diag(G.diagonal()))) * np.sqrt(S)
    print(f"standardised mean / var / skew / kurt {std}, KS sqrt(N) {ks:.3f}, max off-diagonal {off:.3f}")
    assert np.all(np.abs(std) < 4.0)
    assert ks < 1.63
    assert off < 6.0


def test_longdouble_normals_are_the_same_mapping():
    z, r = R.normals(5, 6, 2 ** 33 - 3, 300)
    zl, rl = R.normals(5, 6, 2 ** 33 - 3, 300, np.longdouble)
    assert zl.dtype == np.longdouble
    assert np.max(np.abs(z - zl) / np.maximum(1.0, rl)) < 16 * 2.0 ** -52


@pytest.mark.parametrize('noise, jitter', [(False, 0.0), (True, 0.0), (False, 2e-4)])
def test_draws_have_the_reference_covariance(noise, jitter):
    """Exactly, through the factor: samples - fs = Lc Xi with Lc Lc' = C, and C
    is cov plus the diagonal terms."""
    cells = synthetic.make_cells([65], seed=3)
    x, y, centre = cells.cell(0)
    g = (np.arange(4) - 1.5) * 25e3
    gx, gy = np.meshgrid(g, g, indexing='ij')
    xs = np.stack([centre[0, 0] + gx.ravel(), centre[0, 1] + gy.ravel(), np.full(16, centre[0, 2])], axis=1)
    xi = R.cell_xi(1, 2, 16, 8)
    samples, fs, sd, C, Lc = R.sample_cell(x, y, xs, cells.mean, HYP, xi, noise, jitter)
    _, cov = R.posterior(x, y, xs, cells.mean, HYP)
    want = cov + np.eye(16) * ((HYP[4] if noise else 0.0) + jitter)
    assert np.max(np.abs(C - want)) <= 4 * np.finfo(float).eps * HYP[3]
    assert np.array_equal(np.triu(Lc, 1), np.zeros((16, 16)))
    assert np.max(np.abs(Lc @ Lc.T - C)) <= 16 * np.finfo(float).eps * np.max(C)
    assert np.max(np.abs((samples - fs[:, None]) - Lc @ xi)) <= 4 * np.finfo(float).eps * np.max(np.abs(samples))
    assert np.array_equal(sd, np.sqrt(cov.diagonal()))
    # the linear map's covariance for unit-covariance normals is Lc I Lc' = C: nothing statistical
    assert np.allclose(np.linalg.solve(Lc, samples - fs[:, None]), xi, rtol=0, atol=1e-9)
