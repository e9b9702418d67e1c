"""The day kernels (csrc/oi_day.hip) edge by edge against the CPU oracle:
every smoothing tile and window size, numpy's summation boundaries as
k_smooth_fix sees them, the radius query's chunk, wave and batch boundaries,
non-finite inputs, the ABI's cap contract, the chunk boxes themselves and the
gather's NaN rows.  Cases and references: tests/day_ref.py (checked on the CPU
by tests/test_day_ref.py).

All comparisons are bitwise.  Device-mode calls run on views into larger
buffers filled with a guard value that must still be there afterwards, so a
stray write shows without faulting anything."""
import ctypes

import numpy as np
import pytest

import day_ref as R
from oracle import day_oracle as D
from optimalinterpolation_amd import _lib

pytestmark = pytest.mark.gpu


def same(a, b, what=''):
    """Bitwise equal, signed zeros included; NaN equals NaN whatever its payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    ok = a.shape == b.shape and np.array_equal(na, nb) and R.same_bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))
    if not ok and a.shape == b.shape:  # diagnostics for the failure message
        bad = ~(((a == b) & (np.signbit(a) == np.signbit(b))) | (na & nb))
        print(f"{what}: {bad.sum()} of {bad.size} entries differ, first at {np.argwhere(bad)[0]}, "
              f"nan-pattern equal {np.array_equal(na, nb)}")
    return ok


# ------------------------------------------------------------- smoothing
@pytest.mark.parametrize('ks', R.KSIZES)
@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: '%dx%d' % s)
def test_smooth_tiles_windows_and_kernels(shape, ks):
    """Images narrower than a tile or than the window, every kernel size up to
    the ABI's 65, a Gaussian, an asymmetric kernel (a transposed or un-flipped
    read fails here) and one with zero and negative entries; NaN / inf / zero
    fields, vmax that clips, is +inf, NaN or negative."""
    for kind in R.KINDS:
        fields, vmax, mask, kern, ref = R.smooth_case_with_ref(shape, ks, kind)
        got, intact = R.smooth_device(fields, vmax, mask, kern)
        assert intact, kind
        for f in range(len(fields)):
            assert same(got[f], ref[f], f'{kind} field {f}'), (kind, f)
    # host mode: the same result through the library's own copies
    got = _lib.smooth_fields(fields, vmax, mask, kern)
    assert same(got, ref, 'host mode')


@pytest.mark.parametrize('npix', R.FIX_NPIX)
def test_smooth_fix_summation_order(npix):
    """k_smooth_fix alone (a 1 x 1 kernel [[1.0]] makes the convolution the
    identity): zeros become np.nanmean itself, bit for bit, at every boundary
    of numpy's pairwise summation and where the kernel's block-sum loop takes
    a second trip (more than 256 buffers of 8192)."""
    v = R.fix_case(npix)
    mask = np.ones((1, npix))
    got, intact = R.smooth_device(v.reshape(1, 1, npix), np.array([np.inf]), mask, np.array([[1.0]]))
    assert intact
    ref = R.fix_ref(v)
    assert same(got[0, 0], ref, f'npix {npix}')
    if npix <= R.FIX_ORACLE_MAX:
        ok = ~np.isnan(v)
        mean = D.numpy_pairwise_sum(np.where(ok, v, 0.0)) / ok.sum()
        assert np.all(got[0, 0][v == 0] == mean)


@pytest.mark.parametrize('std', [1, 2])
def test_smooth_builtin_kernel(std):
    """kern = NULL: the library builds the kernel itself.  The result equals,
    bitwise, the call with the array the hook returns, and the oracle's
    convolution with that array."""
    fields, vmax, mask, _ = R.smooth_case((33, 31), 9, 'gaussian' if std == 1 else 'asymmetric')
    fields = np.ascontiguousarray(fields)
    nf, ny, nx = fields.shape
    out = np.full(fields.size + 1, R.SENT)
    rc = _lib.load().oi_smooth_fields(_lib._ptr(fields), nf, ny, nx, _lib._ptr(vmax), _lib._ptr(mask), float(std),
                                      None, 0, _lib._ptr(out), ctypes.byref(_lib.options()))
    assert rc == 0 and out[-1] == R.SENT
    got = out[:-1].reshape(fields.shape)
    kern = R.builtin_kernel(std)
    assert same(got, _lib.smooth_fields(fields, vmax, mask, kern), 'kern = hook array')
    for f in range(nf):
        assert same(got[f], R.smooth_ref(fields[f], vmax[f], mask, kern), f'oracle, field {f}')


def test_smooth_refuses_bad_kernel_arguments():
    f, m, vm, out = np.ones((1, 4, 4)), np.ones((4, 4)), np.ones(1), np.full((1, 4, 4), R.SENT)
    k = np.ones((4, 4))
    fn, o = _lib.load().oi_smooth_fields, ctypes.byref(_lib.options())
    for std in (float('nan'), 0.0, -1.0, 8.5):
        assert fn(_lib._ptr(f), 1, 4, 4, _lib._ptr(vm), _lib._ptr(m), std, None, 0, _lib._ptr(out), o) == R.OI_E_ARG
    for ks in (4, 2, 0, 67):        # even, zero, above the ABI's 65
        assert fn(_lib._ptr(f), 1, 4, 4, _lib._ptr(vm), _lib._ptr(m), 1.0, _lib._ptr(k), ks, _lib._ptr(out), o) \
            == R.OI_E_ARG
    assert np.all(out == R.SENT)
    assert same(_lib.smooth_fields(f, vm, m, np.array([[1.0]])), f)      # and a good call still works


# ------------------------------------------------------------- radius query
def _check_query(pts, q, r, ckdtree=True, extra=5):
    offs, idx, intact = R.ball_query_device(pts, q, r, extra=extra)
    ref_offs, ref_idx = R.ball_ref(pts, q, r)
    assert intact
    assert np.array_equal(offs, ref_offs), np.nonzero(np.diff(offs) != np.diff(ref_offs))[0][:5]
    assert np.array_equal(idx, ref_idx)
    if ckdtree and len(pts):
        o2, i2 = R.ckdtree_ref(pts, q, r)
        assert np.array_equal(offs, o2) and np.array_equal(idx, i2)
    return offs, idx


@pytest.mark.parametrize('layout', R.LAYOUTS)
@pytest.mark.parametrize('M', R.QUERY_M)
def test_query_sizes_and_layouts(M, layout):
    """M on the 256-point chunk boundaries and on the 256-chunk batch
    boundaries; compact chunks, chunks whose boxes span everything, and a chunk
    with a far clump.  r = 5 lattice steps: 3-4-5 points sit exactly on the
    radius, and the first target's ball ends on the first row of a chunk."""
    _check_query(R.query_points(M, layout), R.query_targets(M), 5 * R.S)


def test_query_constructed_hit_patterns():
    pts, q, r, expected = R.hit_patterns()
    offs, idx = _check_query(pts, q, r)
    for k, want in enumerate(expected):
        assert np.array_equal(idx[offs[k]:offs[k + 1]], want), k
    # every target hits all M
    M = len(pts)
    offs, idx = _check_query(pts, q[:2], 1e9, ckdtree=False)
    assert list(offs) == [0, M, 2 * M] and np.array_equal(idx[M:], np.arange(M))


def test_query_exact_radius():
    pts, q, r, expected = R.exact_radius_case()
    offs, idx = _check_query(pts, q, r)
    assert np.array_equal(idx, expected)
    p3 = np.array([[R.S, 2 * R.S], [0.0, 0.0], [R.S, 2 * R.S], [R.S, 2 * R.S]])
    offs, idx = _check_query(p3, p3[:1], 0.0)
    assert list(idx) == [0, 2, 3]


@pytest.mark.parametrize('r', [5 * R.S, float('inf'), 1e200], ids=['r5S', 'rinf', 'r1e200'])
def test_query_nonfinite(r):
    """NaN and +-inf rows scattered through pts, one chunk all NaN, NaN and
    infinite targets, r*r = +inf."""
    pts = R.nonfinite_points()
    q = np.array([[20 * R.S, 7 * R.S], [np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0], [3 * R.S, 9 * R.S]])
    offs, idx = _check_query(pts, q, r, ckdtree=False)
    assert offs[2] == offs[1] and offs[3] == offs[2]
    if r > 5 * R.S:
        assert np.array_equal(idx[:offs[1]], np.nonzero(~np.isnan(pts).any(axis=1))[0])


@pytest.mark.parametrize('Q', [1, 3, 257, 70000])
def test_query_target_counts(Q):
    rng = np.random.default_rng(11)
    q = (rng.uniform(-2 * R.S, 66 * R.S, (70000, 2)) * [1.0, 0.1])[:Q]
    _check_query(R.lattice(300), q, 5 * R.S, ckdtree=Q <= 257)


@pytest.mark.parametrize('case', ['lattice', 'nonfinite', 'patterns'])
def test_chunk_bounding_boxes(case):
    """k_chunk_bbox through oi_launch_ball_count: every chunk's box is the
    NaN-ignoring min / max of its points, bitwise, partial tail and all-NaN
    chunk included; counts equal the oracle's."""
    if case == 'lattice':
        pts, q, r = R.query_points(1000, 'clump'), R.query_targets(1000), 5 * R.S
    elif case == 'nonfinite':
        pts, q, r = R.nonfinite_points(), R.query_targets(800), 5 * R.S
    else:
        pts, q, r, _ = R.hit_patterns()
    bbox, counts, intact = R.ball_count_launch(pts, q, r * r)
    assert intact
    ref = R.bbox_ref(pts)
    assert np.array_equal(np.isnan(bbox), np.isnan(ref))
    assert R.same_bits(np.where(np.isnan(bbox), 0.0, bbox), np.where(np.isnan(ref), 0.0, ref))
    assert np.array_equal(counts, np.diff(R.ball_ref(pts, q, r)[0]))


def test_query_cap_contract():
    """idx = NULL writes offs only; cap = total - 1 returns 0 with correct offs
    and idx untouched; cap = total fills; cap > total leaves the tail
    untouched; host and device mode agree."""
    import torch
    pts, q, r = R.query_points(1000, 'lattice'), R.query_targets(1000), 5 * R.S
    ref_offs, ref_idx = R.ball_ref(pts, q, r)
    total = int(ref_offs[-1])
    assert total > 10
    rc, offs = R.ball_query_raw(pts, q, r)                               # host, idx = NULL
    assert rc == 0 and np.array_equal(offs, ref_offs)
    for cap, filled in ((total - 1, False), (total, True), (total + 7, True)):
        idx = np.full(total + 9, R.SENT_I, dtype=np.int64)
        rc, offs = R.ball_query_raw(pts, q, r, idx=idx, cap=cap)
        assert rc == 0 and np.array_equal(offs, ref_offs), cap
        if filled:
            assert np.array_equal(idx[:total], ref_idx) and np.all(idx[total:] == R.SENT_I), cap
        else:
            assert np.all(idx == R.SENT_I), cap
    # device mode, the same three caps
    tp, tq = torch.from_numpy(pts).cuda(), torch.from_numpy(q).cuda()
    rc, offs = R.ball_query_raw(tp, tq, r, device=True)
    assert rc == 0 and np.array_equal(offs, ref_offs)
    for cap, filled in ((total - 1, False), (total, True), (total + 7, True)):
        g = R.Guarded((total + 9,), dtype='int64')
        g.t.fill_(R.SENT_I)
        rc, offs = R.ball_query_raw(tp, tq, r, idx=g.t, cap=cap, device=True)
        assert rc == 0 and np.array_equal(offs, ref_offs) and g.intact(), cap
        idx = g.numpy()
        if filled:
            assert np.array_equal(idx[:total], ref_idx) and np.all(idx[total:] == R.SENT_I), cap
        else:
            assert np.all(idx == R.SENT_I), cap
    # a negative radius or cap is refused
    assert R.ball_query_raw(pts, q, -1.0)[0] == R.OI_E_ARG
    assert R.ball_query_raw(pts, q, float('nan'))[0] == R.OI_E_ARG
    assert R.ball_query_raw(pts, q, r, cap=-1)[0] == R.OI_E_ARG


# ------------------------------------------------------------- gather
@pytest.mark.parametrize('M', R.GATHER_M)
@pytest.mark.parametrize('N', R.GATHER_N)
def test_gather_device_rows_and_bad_indices(N, M):
    """Repeated and descending indices, NaN / inf / -0.0 payloads compared as
    bits; in device mode exactly the rows of a bad index are NaN."""
    cols, idx = R.gather_case(N, M)
    xyt, z, intact = R.gather_device(cols, idx)
    ref_xyt, ref_z = R.gather_ref(cols, idx)
    assert intact and R.same_bits(xyt, ref_xyt) and R.same_bits(z, ref_z)
    hx, hz = _lib.gather_rows(*cols, idx)                               # host mode
    assert R.same_bits(hx, ref_xyt) and R.same_bits(hz, ref_z)
    bad, pos = R.gather_bad(idx, M)
    xyt, z, intact = R.gather_device(cols, bad)
    assert intact
    assert np.isnan(xyt[pos]).all() and np.isnan(z[pos]).all()
    keep = np.setdiff1d(np.arange(N), pos)
    assert R.same_bits(xyt[keep], ref_xyt[keep]) and R.same_bits(z[keep], ref_z[keep])
    # host mode refuses each bad index, and a good call succeeds afterwards
    for p in pos:
        one = idx.copy()
        one[p] = bad[p]
        with pytest.raises(_lib.OiError, match='liboi error -1'):
            _lib.gather_rows(*cols, one)
    hx, hz = _lib.gather_rows(*cols, idx)
    assert R.same_bits(hx, ref_xyt) and R.same_bits(hz, ref_z)
