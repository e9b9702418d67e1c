"""CPU checks of tests/day_ref.py, the cases of the day kernels' per-edge GPU
tests (tests/test_gpu_day_kernels.py), and the pin of the kernel that
oi_smooth_fields(kern = NULL, std) builds.  No GPU.

A case that cannot tell a right kernel from a wrong one proves nothing, so the
generators are checked here against the oracle alone: the constructed hit
patterns have the lane and chunk positions they claim, the asymmetric kernels
are asymmetric (and the oracle's result changes when the flip or the transpose
is dropped), and every summation case changes bits under another summation
order."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import day_ref as R
from oracle import day_oracle as D
from optimalinterpolation_amd import _lib


# ------------------------------------------------- the built-in Gaussian kernel
def test_hook_is_exported_and_not_in_oi_h():
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\b[TW] oi_test_gaussian_kernel\b', out)
    assert 'oi_test_gaussian_kernel' not in _lib.SIGNATURES


@pytest.mark.parametrize('std', [0.5, 1, 1.5, 2, 3, 8, 0.3, 2.7])
def test_builtin_kernel_within_4ulp_of_numpy(std):
    """gaussian_kernel (csrc/oi_day.cpp) against D.gaussian2d_kernel: the same
    size and every entry within 4 ulp.  The bound is derived: the two exp
    implementations are each within 1 ulp of the truth, so they differ by at
    most 2; the normalising sum (taken in numpy's order on both sides) of such
    terms moves by at most 1; the division adds 1.  With the sum taken left to
    right instead, entries are 5-22 ulp off at std 1, 2, 3 and 8."""
    k, ref = R.builtin_kernel(std), D.gaussian2d_kernel(std)
    assert k.shape == ref.shape
    d = R.ulp_distance(k, ref)
    print(f"std {std}: ks {k.shape[0]}, max {d.max()} ulp, {np.count_nonzero(d)} of {d.size} entries differ")
    assert d.max() <= 4


@pytest.mark.parametrize('std', [1, 1.5])
def test_builtin_kernel_bit_equal(std):
    """At these widths libm's exp and numpy's agree on every entry, so the
    kernel is numpy's bit for bit once the sum is taken in numpy's order
    (std = 1 is a production width).  This depends on both exp builds; the
    4-ulp pin above does not."""
    assert R.same_bits(R.builtin_kernel(std), D.gaussian2d_kernel(std))


def test_builtin_kernel_refused_widths():
    for std in (0.0, -1.0, float('nan'), 8.0 + 1e-9, float('inf')):
        assert R.lib().oi_test_gaussian_kernel(std, None, 0) == -1, std
    assert R.lib().oi_test_gaussian_kernel(8.0, None, 0) == 65
    # too small a cap writes nothing and still returns the size
    out = np.full(81, R.SENT)
    assert R.lib().oi_test_gaussian_kernel(1.0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 80) == 9
    assert np.all(out == R.SENT)


def test_normalising_sum_order_shows_in_the_bits():
    """The pin bites: normalised by a left-to-right sum, the oracle's own
    kernel moves (so a builder that adds left to right cannot be bit-equal)."""
    for std in (1, 2):
        k = D.gaussian2d_kernel(std)
        raw = k * 3.0       # any unnormalised multiple
        assert raw.sum() == D.numpy_pairwise_sum(raw.ravel())
        assert raw.sum() != np.cumsum(raw.ravel())[-1]


# ------------------------------------------------- smoothing cases
def test_smooth_kernels_are_what_they_claim():
    for ks in R.KSIZES:
        g, a, s = (R.smooth_kernel(kind, ks) for kind in R.KINDS)
        assert g.shape == a.shape == s.shape == (ks, ks)
        assert np.all(a > 0) and len(np.unique(a)) == a.size and a.sum() != 1.0
        if ks > 1:      # a 1 x 1 kernel is its own transpose
            assert not np.array_equal(a, a.T) and not np.array_equal(a, a[::-1, ::-1])
            assert not np.array_equal(a, a[::-1]) and not np.array_equal(a, a[:, ::-1])
            assert (s == 0).any() and (s < 0).any() and (s > 0).any()
        else:
            assert s[0, 0] < 0 and np.array_equal(g, [[1.0]])


@pytest.mark.parametrize('ks', [3, 9, 17, 65])
def test_asymmetric_kernel_shows_a_missing_flip(ks):
    """With the asymmetric kernel the oracle's own result changes when the
    kernel is not flipped, or transposed: a kernel that indexed it wrongly
    cannot pass.  With the Gaussian it does not change."""
    fields, vmax, mask, kern = R.smooth_case((33, 31), ks, 'asymmetric')
    f = np.where(np.isinf(fields[0]), np.nan, fields[0])
    ref = D.convolve_interpolate(f, kern)
    for wrong in (kern[::-1, ::-1], kern.T, kern[::-1], kern[:, ::-1]):
        assert not np.array_equal(D.convolve_interpolate(f, np.ascontiguousarray(wrong)), ref, equal_nan=True)
    g = R.smooth_kernel('gaussian', ks)
    assert np.array_equal(D.convolve_interpolate(f, np.ascontiguousarray(g[::-1, ::-1].T)),
                          D.convolve_interpolate(f, g), equal_nan=True)


def test_smooth_cases_cover_what_they_claim():
    nfs, masks, vm1 = set(), set(), set()
    nan_window = bot_negative = bot_cancels = zero_replaced = False
    for shape in R.SHAPES:
        for ks in R.KSIZES:
            for kind in R.KINDS:
                fields, vmax, mask, kern, ref = R.smooth_case_with_ref(shape, ks, kind)
                assert fields.shape == (len(vmax),) + shape and ref.shape == fields.shape
                nfs.add(len(fields))
                masks.add('all' if np.isnan(mask).all() else 'none' if not np.isnan(mask).any() else 'some')
                if len(fields) == 1:
                    vm1.add(repr(float(vmax[0])))
                if len(fields) >= 5:
                    assert np.isnan(fields[2]).all()
                    if ks == 1:     # no padding in the window: an all-NaN field stays NaN
                        assert np.isnan(ref[2]).all()
                    assert not fields[3].any() and not np.isnan(fields[4]).any()
                if len(fields) == 7 and fields[5].size >= 15:
                    assert (fields[5] == 0).any() and np.signbit(fields[5][fields[5] == 0]).any()
                if shape == (33, 31) and len(fields) >= 5:
                    f1 = fields[1]
                    conv = D.convolve_interpolate(f1, kern)
                    if ks <= 9 and kind != 'signed':
                        assert np.isnan(conv[16, 15])          # a whole window of NaN
                        nan_window = True
                    if kind == 'signed':
                        bot = _bot(~(np.isnan(fields[0]) | np.isinf(fields[0])), kern)
                        bot_negative |= bool((bot < 0).any())
                        bot_cancels |= bool((bot == 0).any())
                    if len(fields) == 7 and kind != 'signed':
                        c6 = D.convolve_interpolate(fields[6], kern)
                        zero_replaced |= bool((c6 == 0).any() and np.isfinite(np.nanmean(c6)))
    assert nfs == {1, 5, 7} and masks == {'all', 'none', 'some'}
    assert vm1 == {repr(0.5), repr(np.inf), repr(np.nan), repr(-0.25)}
    assert nan_window and bot_negative and bot_cancels and zero_replaced
    # the mixed field: +-inf on pixels 0, 15, 16 and the last row and column, ~45 % NaN
    f0 = R.smooth_case((33, 31), 9, 'gaussian')[0][0]
    assert np.isinf(f0[0, [0, 15, 16]]).all() and np.isinf(f0[32, [0, 15, 16, 30]]).all()
    assert np.isinf(f0[[0, 15, 16], 30]).all()
    assert 0.35 < np.isnan(f0).mean() < 0.55 and (f0 == 50.0).any()


def _bot(valid, kern):
    """The convolution's ``bot``: the flipped kernel summed over the valid
    entries of each pixel's window, padding included (exact for the signed
    kernels, whose entries are multiples of 1/4)."""
    return ndimage.correlate(valid.astype(float), kern[::-1, ::-1], mode='constant', cval=1.0)


@pytest.mark.parametrize('npix', R.FIX_NPIX)
def test_fix_cases_show_the_summation_order(npix):
    """Each k_smooth_fix case: np.nanmean is the reference, the oracle's
    restatement agrees with it (up to 16389 pixels here; the largest size is in
    tests/test_day_oracle.py), and the mean changes bits when the terms are
    added in another order -- otherwise the case could not tell numpy's order
    from any other.  Below 8 terms numpy itself adds left to right, so there the
    other order is right to left; one pixel has no order."""
    v = R.fix_case(npix)
    ok = ~np.isnan(v)
    assert ok.any() and np.array_equal(R.fix_ref(v)[v == 0], np.full((v == 0).sum(), np.nanmean(v)))
    if npix >= 7:
        assert (v == 0).any()
    if npix >= 127:
        assert 0.3 < np.isnan(v).mean() < 0.5
    if npix <= R.FIX_ORACLE_MAX:
        assert D.numpy_pairwise_sum(np.where(ok, v, 0.0)) / ok.sum() == np.nanmean(v)
    if npix >= 8:
        assert R.sum_left_to_right(v) / ok.sum() != np.nanmean(v)
    elif npix == 7:
        assert R.sum_left_to_right(v[::-1]) / ok.sum() != np.nanmean(v)
    if npix == R.FIX_NPIX[-1]:
        assert (npix + 8191) // 8192 > 256      # a second trip of the block-sum loop


# ------------------------------------------------- radius-query cases
@pytest.mark.parametrize('M', R.QUERY_M)
def test_query_layouts_against_ckdtree(M):
    q = R.query_targets(M)
    for layout in R.LAYOUTS:
        pts = R.query_points(M, layout)
        assert pts.shape == (M, 2)
        offs, idx = R.ball_ref(pts, q, 5 * R.S)
        for c in range(len(q)):
            assert np.array_equal(idx[offs[c]:offs[c + 1]], D.ball_query(pts, q[c], 5 * R.S))
        if M:
            o2, i2 = R.ckdtree_ref(pts, q, 5 * R.S)
            assert np.array_equal(offs, o2) and np.array_equal(idx, i2)
        assert offs[-1] - offs[-2] == 0                     # the last target hits nothing
        if layout == 'clump' and M >= 512:
            assert offs[4] - offs[3] == 30
    if M >= 1024:
        # the first target's ball ends exactly on the first row of a chunk: that
        # chunk holds a hit and its box is at distance r exactly
        pts = R.query_points(M, 'lattice')
        hits = D.ball_query(pts, q[0], 5 * R.S)
        top = 12 * R.WIDTH + 20
        assert top in hits and top % R.CHUNK == 20 and pts[top, 1] - q[0, 1] == 5 * R.S
        assert pts[(top // R.CHUNK) * R.CHUNK:(top // R.CHUNK + 1) * R.CHUNK, 1].min() - q[0, 1] == 5 * R.S


def test_hit_patterns_are_where_they_claim():
    pts, q, r, expected = R.hit_patterns()
    M = len(pts)
    assert M == R.PATTERN_M and (M + R.CHUNK - 1) // R.CHUNK == 259 and M % R.CHUNK == R.PATTERN_TAIL
    offs, idx = R.ball_ref(pts, q, r)
    for k, want in enumerate(expected):
        assert np.array_equal(idx[offs[k]:offs[k + 1]], want), k
    o2, i2 = R.ckdtree_ref(pts, q, r)
    assert np.array_equal(offs, o2) and np.array_equal(idx, i2)
    nfull = M // R.CHUNK
    for k, c in enumerate([0, nfull // 2, nfull - 1, nfull]):
        assert np.all(expected[k] // R.CHUNK == c)
        local = list(expected[k] % R.CHUNK)
        assert local == [p for p in R.LANES if c * R.CHUNK + p < M]
        # lanes 0 and 63 of a wave, lane 0 of the next, threads 0 and 255 of a chunk
        assert {0, 63, 64} <= set(local) and (255 in local) == (c < nfull)
    assert 0 < nfull // 2 < 255 and nfull - 1 > 256         # first batch, and the second
    assert len(expected[4]) == 256 and np.all(expected[4] // R.CHUNK == R.FULL_CHUNK)
    assert len(expected[5]) == 0
    assert set(expected[6] // R.CHUNK) == {255, 256}        # either side of the batch boundary
    # one radius for all: a huge one hits all M for every target
    offs, idx = R.ball_ref(pts, q[:2], 1e9)
    assert list(offs) == [0, M, 2 * M] and np.array_equal(idx[:M], np.arange(M))


def test_exact_radius_case():
    pts, q, r, expected = R.exact_radius_case()
    assert np.array_equal(D.ball_query(pts, q[0], r), expected) and len(expected) == 12
    assert np.array_equal(R.ckdtree_ref(pts, q, r)[1], expected)
    d = pts - q[0]
    assert np.all(d[0::2, 0] ** 2 + d[0::2, 1] ** 2 == r * r)      # exactly on the circle
    assert np.all(d[1::2, 0] ** 2 + d[1::2, 1] ** 2 > r * r)       # one ulp beyond
    # r = 0 on a point stored three times
    p3 = np.array([[R.S, 2 * R.S], [0.0, 0.0], [R.S, 2 * R.S], [R.S, 2 * R.S]])
    assert list(D.ball_query(p3, p3[0], 0.0)) == [0, 2, 3]


def test_nonfinite_points_and_boxes():
    pts = R.nonfinite_points()
    assert np.isnan(pts[R.CHUNK:2 * R.CHUNK]).all()
    rest = np.delete(pts, np.s_[R.CHUNK:2 * R.CHUNK], axis=0)
    assert np.isnan(rest).any() and np.isposinf(rest).any() and np.isneginf(rest).any()
    bb = R.bbox_ref(pts)
    assert bb.shape == (4, 4) and np.isnan(bb[1]).all() and not np.isnan(bb[[0, 2, 3]]).any()
    assert len(pts) % R.CHUNK == 40                          # a partial tail
    q = np.array([[20 * R.S, 7 * R.S], [np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0]])
    for r in (5 * R.S, np.inf, 1e200):
        offs, idx = R.ball_ref(pts, q, r)
        with np.errstate(invalid='ignore'):
            for c in range(len(q)):
                assert np.array_equal(idx[offs[c]:offs[c + 1]], D.ball_query(pts, q[c], r))
        assert offs[2] - offs[1] == 0 and offs[3] - offs[2] == 0     # a NaN target hits nothing
    # r*r = +inf: every point without a NaN coordinate is a hit, infinite ones included
    offs, idx = R.ball_ref(pts, q[:1], 1e200)
    assert np.array_equal(idx, np.nonzero(~np.isnan(pts).any(axis=1))[0])
    assert np.isinf(pts[idx]).any()


def test_many_targets_reference():
    rng = np.random.default_rng(11)
    pts = R.lattice(300)
    q = rng.uniform(-2 * R.S, 66 * R.S, (70000, 2)) * [1.0, 0.1]
    offs, idx = R.ball_ref(pts, q, 5 * R.S)
    assert len(offs) == 70001 and offs[-1] == len(idx) > 70000
    for c in (0, 1, 65535, 65536, 69999):
        assert np.array_equal(idx[offs[c]:offs[c + 1]], D.ball_query(pts, q[c], 5 * R.S))


# ------------------------------------------------- gather cases
@pytest.mark.parametrize('M', R.GATHER_M)
@pytest.mark.parametrize('N', R.GATHER_N)
def test_gather_cases(N, M):
    cols, idx = R.gather_case(N, M)
    assert len(idx) == N and idx.min() >= 0 and idx.max() < M
    if N >= 4:
        assert len(np.unique(idx)) < N                      # repeated
    if M > 1 and N > 1:
        assert idx[0] > idx[1]                              # descending
    if M == 300:
        allv = np.concatenate(cols)
        assert np.isnan(allv).any() and np.isposinf(allv).any() and np.isneginf(allv).any()
    xyt, z = R.gather_ref(cols, idx)
    assert R.same_bits(xyt[:, 1], cols[1][idx]) and R.same_bits(z, cols[3][idx])
    bad, pos = R.gather_bad(idx, M)
    assert set(pos) >= {0, N - 1, N // 2}
    assert all(b < 0 or b >= M for b in bad[pos]) and np.array_equal(np.delete(bad, pos), np.delete(idx, pos))
    if N >= 4:
        assert set(bad[pos]) == {-1, M, 2 ** 40, R.INT64_MIN}
    xb, zb = R.gather_ref(cols, bad, pos)
    assert np.isnan(xb[pos]).all() and np.isnan(zb[pos]).all()
    keep = np.setdiff1d(np.arange(N), pos)
    assert R.same_bits(xb[keep], xyt[keep]) and R.same_bits(zb[keep], z[keep])
    if M == 300:
        got = np.concatenate([c[idx] for c in cols]).view(np.int64)
        if N >= 255:    # the two NaN bit patterns and -0.0 are among the gathered payloads
            assert {int(v) for v in R.NAN_PAYLOAD.view(np.int64)} <= set(got.tolist())
            assert int(np.array([-0.0]).view(np.int64)[0]) in set(got.tolist())
