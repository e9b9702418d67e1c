"""Cases and references for the per-edge tests of the day kernels
(csrc/oi_day.hip: smoothing, radius query, gather).

Holds the ctypes signatures of the day launchers and of the kernel-builder hook,
the guarded device buffers, the case generators and the constructed hit
patterns with their expected index lists.  tests/test_day_ref.py runs all of it
against the oracle alone (no GPU); tests/test_gpu_day_kernels.py runs the same
cases through the kernels.

Sizes the kernels care about: smoothing tiles are 16 x 16 pixels (SM_TILE);
np.nanmean sums 8192-element buffers pairwise with 128-element leaves and
k_smooth_fix takes 256 buffers per trip of its block-sum loop; the radius query
scans chunks of 256 points (BQ_CHUNK), one wave per 64, and prunes chunk boxes
256 chunks at a time."""
import ctypes
import functools
import warnings

import numpy as np

from oracle import day_oracle as D

CHUNK = 256                 # BQ_CHUNK
BATCH = CHUNK * CHUNK       # points per batch of 256 chunk boxes
SENT = -6.0221e23           # guard value of fp64 buffers (finite, so == finds it)
SENT_I = -0x5A5A5A5A5A5A5A5A  # and of int64 buffers (never a valid index or count)
PAD = 64                    # guard elements on each side of a view
OI_E_ARG = -1

_lib = None


def lib():
    """liboi.so with the day launchers of csrc/oi_day.hip and the hook bound."""
    global _lib
    if _lib is None:
        from optimalinterpolation_amd import _lib as L
        h = L.load()
        P, l, V = ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p
        sig = {'oi_launch_smooth': [P, P, ctypes.c_int, l, l, P, P, ctypes.c_int, P, V],
               'oi_launch_ball_count': [P, l, P, P, l, ctypes.c_double, P, V],
               'oi_launch_ball_fill': [P, l, P, P, l, ctypes.c_double, P, P, V],
               'oi_launch_gather_rows': [P, P, P, P, P, l, l, P, P, V]}
        for name, args in sig.items():
            f = getattr(h, name)
            f.argtypes, f.restype = args, ctypes.c_int
        h.oi_test_gaussian_kernel.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.c_int32]
        h.oi_test_gaussian_kernel.restype = ctypes.c_int32
        _lib = h
    return _lib


def builtin_kernel(std):
    """The kernel oi_smooth_fields(kern = NULL, std) builds, or None when it
    refuses ``std``.  No GPU needed."""
    fn = lib().oi_test_gaussian_kernel
    ks = fn(float(std), None, 0)
    if ks < 0:
        return None
    out = np.full(ks * ks + 1, SENT)
    assert fn(float(std), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ks * ks) == ks
    assert out[-1] == SENT
    return out[:-1].reshape(ks, ks).copy()


def ulp_distance(a, b):
    """Distance in units in the last place between finite doubles of one sign."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


# ------------------------------------------------------------ guarded buffers
class Guarded:
    """A device tensor that is a view into a larger buffer filled with a guard
    value: ``t`` is what the kernel gets, ``intact()`` says whether everything
    around it still holds the guard."""

    def __init__(self, shape, dtype='float64', init=None, pad=PAD):
        import torch
        n = int(np.prod(shape))
        self.sent = SENT if dtype == 'float64' else SENT_I
        self.buf = torch.full((n + 2 * pad,), self.sent, dtype=getattr(torch, dtype), device='cuda')
        self.n, self.pad = n, pad
        self.t = self.buf[pad:pad + n].view(*shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.array(init, copy=True)).view(*shape))

    def intact(self):
        lo, hi = self.buf[:self.pad], self.buf[self.pad + self.n:]
        return bool((lo == self.sent).all().item()) and bool((hi == self.sent).all().item())

    def numpy(self):
        return self.t.cpu().numpy()


def same_bits(a, b):
    """Bitwise equality of two fp64 arrays (signed zeros and NaN payloads count)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------ smoothing
SHAPES = [(1, 1), (1, 17), (17, 1), (3, 5), (15, 16), (16, 16), (16, 17), (33, 31)]
KSIZES = [1, 3, 9, 17, 65]
KINDS = ['gaussian', 'asymmetric', 'signed']
KS_STD = {1: 0.1, 3: 0.3, 9: 1, 17: 2, 65: 8}     # the Gaussian width with that kernel size
FIELD_KINDS = ['mixed', 'nanblock', 'allnan', 'allzero', 'nonan', 'zeros', 'sparse']
# per field kind: a value that clips, NaN (no clip), +inf, a value that clips an
# all-zero field to itself, a negative value, +inf, a value that clips
FIELD_VMAX = [0.5, np.nan, np.inf, 0.0, -0.25, np.inf, 0.5]
VMAX_ONE = [0.5, np.inf, np.nan, -0.25]            # rotated through by the one-field cases


def smooth_kernel(kind, ks):
    """The ks x ks kernel of one kind: the oracle's Gaussian of that size; random
    positive entries, all distinct, sum != 1, equal to neither its transpose
    nor its flip; or one with zero and negative entries (``bot`` can be
    negative, or cancel to zero exactly)."""
    if kind == 'gaussian':
        k = D.gaussian2d_kernel(KS_STD[ks])
        assert k.shape == (ks, ks)
        return k
    rng = np.random.default_rng(1000 + ks)
    if kind == 'asymmetric':
        return rng.permutation(np.arange(1, ks * ks + 1) / 8.0).reshape(ks, ks) + rng.random((ks, ks)) / 32.0
    # signed: small integers / 4, so that sums cancel exactly; about a third zero
    k = rng.integers(-3, 4, size=(ks, ks)).astype(np.float64) / 4.0
    k[rng.random((ks, ks)) < 0.3] = 0.0
    if ks == 1:
        k[0, 0] = -0.75
    return k


def smooth_field(kind, shape, rng):
    ny, nx = shape
    v = rng.normal(size=shape)
    if kind == 'allnan':
        return np.full(shape, np.nan)
    if kind == 'allzero':
        return np.zeros(shape)
    if kind == 'nonan':
        return v
    if kind == 'nanblock':     # whole windows are NaN inside the block (for windows smaller than it)
        v[ny // 8:ny - ny // 8, nx // 8:nx - nx // 8] = np.nan
        return v
    if kind == 'zeros':        # exact zeros of both signs among the values, few NaN
        u = rng.random(shape)
        v[u < 0.3] = 0.0
        v[(u >= 0.3) & (u < 0.6)] = -0.0
        v[u > 0.9] = np.nan
        return v
    if kind == 'sparse':       # mostly NaN: windows of padding only give exact zeros
        v[rng.random(shape) < 0.9] = np.nan
        return v
    # mixed: ~45 % NaN, zeros of both signs, values above the clip, +-inf on
    # pixels 0, 15, 16 and on the last row and column
    u = rng.random(shape)
    v[u < 0.45] = np.nan
    v[(u > 0.45) & (u < 0.50)] = 0.0
    v[(u > 0.50) & (u < 0.55)] = -0.0
    v[(u > 0.55) & (u < 0.62)] = 50.0
    flat = v.reshape(-1)
    for n, p in enumerate((0, 15, 16)):
        if p < flat.size:
            flat[p] = np.inf if n % 2 == 0 else -np.inf
        if p < ny:
            v[p, nx - 1] = -np.inf if n % 2 == 0 else np.inf
        if p < nx:
            v[ny - 1, p] = np.inf if n % 2 == 0 else -np.inf
    v[ny - 1, nx - 1] = np.inf
    return v


def smooth_case(shape, ks, kind):
    """(fields [nf, ny, nx], vmax [nf], mask [ny, nx], kern) of one case; nf, the
    one-field vmax and the mask's kind rotate with the case's number."""
    si, ki, ti = SHAPES.index(shape), KSIZES.index(ks), KINDS.index(kind)
    n = (si * len(KSIZES) + ki) * len(KINDS) + ti
    rng = np.random.default_rng(7000 + n)
    nf = (1, 5, 7)[(si + ki + ti) % 3]
    kinds = FIELD_KINDS[:nf]
    fields = np.stack([smooth_field(k, shape, rng) for k in kinds])
    vmax = np.array(FIELD_VMAX[:nf] if nf > 1 else [VMAX_ONE[(si + 2 * ki + ti) % 4]])
    mask = np.where(rng.random(shape) < 0.8, 0.9, np.nan)
    if n % 10 == 4:
        mask[:] = np.nan        # all NaN
    elif n % 10 == 7:
        mask[:] = 0.9           # none
    return fields, vmax, mask, smooth_kernel(kind, ks)


def smooth_ref(field, vmax, mask, kern):
    """D.smooth (GPR:65-76) with the given kernel instead of the Gaussian."""
    d = np.copy(field)
    d[np.isinf(d)] = np.nan
    with np.errstate(invalid='ignore'):
        d[d > vmax] = vmax
    d = D.convolve_interpolate(d, kern)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)     # nanmean of an all-NaN field
        d[d == 0] = np.nanmean(d)
    d[np.isnan(mask)] = np.nan
    return d


@functools.lru_cache(maxsize=None)
def smooth_case_with_ref(shape, ks, kind):
    fields, vmax, mask, kern = smooth_case(shape, ks, kind)
    ref = np.stack([smooth_ref(fields[f], vmax[f], mask, kern) for f in range(len(fields))])
    for a in (fields, vmax, mask, kern, ref):
        a.setflags(write=False)
    return fields, vmax, mask, kern, ref


# k_smooth_fix alone: ks = 1 with kernel [[1.0]] makes the convolution the identity
FIX_NPIX = [1, 7, 8, 9, 127, 128, 129, 136, 8191, 8192, 8193, 16389, 256 * 8192 + 8192 + 5]
FIX_ORACLE_MAX = 16389      # the pure-Python restatement is run up to here


def _fix_draw(npix, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=npix) * rng.choice([1.0, 1e8, 1e-8], size=npix)
    v[rng.random(npix) < 0.4] = np.nan
    if npix >= 7:
        v[:3] = rng.normal(size=3) * [1.0, 1e8, 1e-8]       # never all-NaN at the small sizes
        v[rng.choice(np.arange(3, npix), size=max(1, npix // 50), replace=False)] = 0.0
    else:
        v[:] = 1.5
    return v


@functools.lru_cache(maxsize=None)
def fix_case(npix):
    """A (1, npix) field whose mean shows the summation order in its bits:
    normal x {1, 1e8, 1e-8}, ~40 % NaN, a few exact zeros.  The first draw
    whose np.nanmean differs from the terms added left to right is taken
    (right to left at 7 pixels, where numpy itself adds left to right): a draw
    on which two orders agree could not tell them apart."""
    for seed in range(npix, npix + 50):
        v = _fix_draw(npix, seed)
        other = sum_left_to_right(v if npix >= 8 else v[::-1]) / (~np.isnan(v)).sum()
        if npix < 7 or other != np.nanmean(v):
            v.setflags(write=False)
            return v
    raise AssertionError(f"no draw of {npix} pixels shows the summation order")


def fix_ref(v):
    """k_smooth_fix's result on ``v`` with a mask that has no NaN: np.nanmean itself."""
    out = np.copy(v)
    out[out == 0] = np.nanmean(v)
    return out


def sum_left_to_right(v):
    """The non-NaN entries of v added one by one onto 0.0 (np.cumsum is sequential)."""
    return np.cumsum(np.where(np.isnan(v), 0.0, v))[-1]


# ------------------------------------------------------------ radius query
S = 25e3                    # lattice spacing: S*S and every product below are exact
WIDTH = 64                  # lattice columns: a chunk of 256 points is 4 full rows
QUERY_M = [0, 1, 255, 256, 257, 512, 65535, 65536, 65537, 131073]
LAYOUTS = ['lattice', 'shuffled', 'clump']
CLUMP_AT = (1e7, 1e7)


def lattice(M):
    i = np.arange(M)
    return np.column_stack([(i % WIDTH) * S, (i // WIDTH) * S]).astype(np.float64)


def query_points(M, layout):
    """M points: the grid-ordered lattice (compact chunks); the same shuffled
    (every chunk's box spans everything); or the lattice with 30 points of a
    middle chunk moved to a far clump (that chunk's box spans both)."""
    p = lattice(M)
    if layout == 'shuffled':
        p = p[np.random.default_rng(M).permutation(M)]
    elif layout == 'clump':
        lo = min(M, ((M + CHUNK - 1) // CHUNK // 2) * CHUNK + 10)
        hi = min(M, lo + 30)
        k = np.arange(hi - lo)
        p[lo:hi] = np.column_stack([CLUMP_AT[0] + (k % 6) * S, CLUMP_AT[1] + (k // 6) * S])
    return p


def query_targets(M):
    """Targets for the layouts above, with r = 5 S: a lattice point whose ball
    ends exactly on the first row of a chunk (row 7 + 5 = 12 = 3 * 4: that
    chunk's box is at distance r exactly, and 3-4-5 lattice points are at r
    exactly), the origin corner, a point between lattice points near the last
    row, the clump, and one that hits nothing."""
    last = max(M - 1, 0) // WIDTH
    return np.array([[20 * S, 7 * S], [0.0, 0.0], [31.5 * S, (last - 2) * S + 0.25 * S],
                     [CLUMP_AT[0] + 2 * S, CLUMP_AT[1] + 2 * S], [-9e6, 4e6]])


def ball_ref(pts, q, r):
    """D.ball_query for every row of q, vectorised with the same arithmetic:
    (offs [Q+1], idx)."""
    pts, q = np.asarray(pts, dtype=np.float64).reshape(-1, 2), np.asarray(q, dtype=np.float64).reshape(-1, 2)
    r2 = r * r
    counts, idx = [], []
    step = max(1, 4_000_000 // max(1, len(pts)))
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, len(q), step):
            dx = pts[None, :, 0] - q[a:a + step, None, 0]
            dy = pts[None, :, 1] - q[a:a + step, None, 1]
            d2 = dx * dx
            d2 = d2 + dy * dy
            hit = d2 <= r2
            counts.append(hit.sum(axis=1))
            idx.append(np.nonzero(hit)[1])
    offs = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64) if counts else np.zeros(1, np.int64)
    return offs, (np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64))


def ckdtree_ref(pts, q, r):
    """scipy's own answer, sorted (only for finite coordinates)."""
    from scipy.spatial import cKDTree
    tree = cKDTree(pts)
    lists = [np.sort(np.asarray(tree.query_ball_point(x=x, r=r), dtype=np.int64)) for x in q]
    offs = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    return offs, (np.concatenate(lists) if lists else np.zeros(0, np.int64))


# Constructed hit patterns: background points on the lattice, the points a
# target is to hit moved next to that target, far from everything else.
LANES = [0, 63, 64, 127, 128, 191, 192, 255]        # first/last lanes of the 4 waves of a chunk
PATTERN_TAIL = 200                                  # points in the partial last chunk
PATTERN_M = BATCH + 2 * CHUNK + PATTERN_TAIL        # 259 chunks: two batches of chunk boxes
PATTERN_R = 5 * S
FULL_CHUNK = 7                                      # the chunk whose 256 points all hit


@functools.lru_cache(maxsize=None)
def hit_patterns():
    """(pts, q, r, expected): ``expected[k]`` is the ascending index list that
    target k hits, known by construction:
      0..3  chunk-local positions LANES of the first chunk, a middle chunk, the
            last full chunk and the partial tail (positions < PATTERN_TAIL)
      4     all 256 points of chunk FULL_CHUNK
      5     nothing
      6     three points either side of the 256-chunk batch boundary"""
    M = PATTERN_M
    pts = lattice(M)
    nfull = M // CHUNK
    chunks = [0, nfull // 2, nfull - 1, nfull]
    expected = []
    for c in chunks:
        expected.append(np.array([c * CHUNK + p for p in LANES if c * CHUNK + p < M], dtype=np.int64))
    expected.append(np.arange(FULL_CHUNK * CHUNK, (FULL_CHUNK + 1) * CHUNK, dtype=np.int64))
    expected.append(np.zeros(0, dtype=np.int64))
    expected.append(np.arange(BATCH - 3, BATCH + 3, dtype=np.int64))
    q = np.array([[-1e7 - 4e5 * k, 3e7 + 4e5 * k] for k in range(len(expected))])
    for k, ids in enumerate(expected):
        j = np.arange(len(ids))
        if k == 4:      # a 16 x 16 patch of spacing S / 8 around the target: all well inside r
            pts[ids] = q[k] + np.column_stack([(j % 16 - 8) * (S / 8), (j // 16 - 8) * (S / 8)])
        else:           # on a circle of radius 3 S around the target
            pts[ids] = q[k] + 3 * S * np.column_stack([np.cos(j), np.sin(j)])
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q, PATTERN_R, expected


def exact_radius_case():
    """Points at distance exactly r = 5 S from the target (3-4-5 triangles and
    the axes: every product is an exact integer) are hits; one np.nextafter
    further out is a miss.  Returns (pts, q, r, expected)."""
    q = np.array([[0.0, 0.0]])     # the bump of one ulp must survive the subtraction
    offs = [(3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3), (-4, 3), (4, -3), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5)]
    on = q[0] + np.array(offs, dtype=np.float64) * S
    beyond = on.copy()
    for k, (a, b) in enumerate(offs):       # push the larger offset one ulp outwards
        ax = 0 if abs(a) > abs(b) else 1
        beyond[k, ax] = np.nextafter(on[k, ax], np.inf if offs[k][ax] > 0 else -np.inf)
    pts = np.empty((2 * len(offs), 2))
    pts[0::2], pts[1::2] = on, beyond
    return pts, q, 5 * S, np.arange(0, 2 * len(offs), 2, dtype=np.int64)


def nonfinite_points(M=3 * CHUNK + 40, seed=3):
    """A lattice with NaN and +-inf rows scattered through it (single
    coordinates and whole rows), and chunk 1 all NaN."""
    p = lattice(M)
    rng = np.random.default_rng(seed)
    ids = rng.choice(M, size=60, replace=False)
    vals = [np.nan, np.inf, -np.inf]
    for n, i in enumerate(ids):
        if n % 3 == 0:
            p[i, 0] = vals[(n // 3) % 3]
        elif n % 3 == 1:
            p[i, 1] = vals[(n // 3) % 3]
        else:
            p[i] = vals[(n // 3) % 3]
    p[CHUNK:2 * CHUNK] = np.nan
    return p


def bbox_ref(pts):
    """Per chunk of 256 points: (min x, max x, min y, max y) ignoring NaN, NaN
    where every coordinate of the chunk is NaN.  [nchunk, 4]."""
    M = len(pts)
    nchunk = (M + CHUNK - 1) // CHUNK
    out = np.empty((nchunk, 4))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)     # all-NaN slice
        for c in range(nchunk):
            p = pts[c * CHUNK:(c + 1) * CHUNK]
            out[c] = [np.nanmin(p[:, 0]), np.nanmax(p[:, 0]), np.nanmin(p[:, 1]), np.nanmax(p[:, 1])]
    return out


# ------------------------------------------------------------ gather
GATHER_N = [1, 255, 256, 257, 1000]
GATHER_M = [1, 300]
INT64_MIN = -2 ** 63
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000001 | (1 << 51)], dtype=np.uint64).view(np.float64)


def gather_case(N, M):
    """(cols = (x, y, t, z) [M] each, idx [N]): payloads with NaN (two bit
    patterns), +-inf and -0.0; indices descending, then repeated."""
    rng = np.random.default_rng(100 * N + M)
    cols = [rng.normal(size=M) for _ in range(4)]
    special = [NAN_PAYLOAD[0], NAN_PAYLOAD[1], np.inf, -np.inf, -0.0, 0.0]
    for c, col in enumerate(cols):
        for n, v in enumerate(special):
            col[(M - 1 - 7 * n - c) % M] = v     # near the end: the descending indices reach them
    desc = np.arange(M - 1, -1, -1, dtype=np.int64)
    idx = np.concatenate([desc, rng.integers(0, M, size=N, dtype=np.int64)])[:N]
    if N >= 4:
        idx[N // 2] = idx[N // 2 - 1]           # a repeat next to itself
    return cols, idx


def gather_bad(idx, M):
    """idx with the bad indices {-1, M, 2^40, INT64_MIN} placed first, last and
    in the middle: (idx, sorted positions of the bad ones)."""
    N = len(idx)
    bad = [-1, M, 2 ** 40, INT64_MIN]
    pos = sorted({0, N - 1, N // 2, min(N - 1, N // 2 + 1)})
    out = idx.copy()
    for n, p in enumerate(pos):
        out[p] = bad[n % 4]
    return out, np.array(pos, dtype=np.int64)


def gather_ref(cols, idx, bad=()):
    x, y, t, z = cols
    ok = np.ones(len(idx), dtype=bool)
    ok[np.asarray(bad, dtype=np.int64)] = False
    safe = np.where(ok, idx, 0)
    xyt = np.stack([x[safe], y[safe], t[safe]], axis=1)
    zo = z[safe].copy()
    xyt[~ok] = np.nan
    zo[~ok] = np.nan
    return xyt, zo


# ------------------------------------------------------------ device-mode calls
def _dp(t, ctype=ctypes.c_double):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctype))


def _hp(a, ctype=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def smooth_device(fields, vmax, mask, kern):
    """oi_smooth_fields in device mode on guarded buffers: (out, guards intact)."""
    from optimalinterpolation_amd import _lib as L
    nf, ny, nx = fields.shape
    f, m, out = Guarded(fields.shape, init=fields), Guarded(mask.shape, init=mask), Guarded(fields.shape)
    vm, k = np.ascontiguousarray(vmax, dtype=np.float64), np.ascontiguousarray(kern, dtype=np.float64)
    rc = lib().oi_smooth_fields(_dp(f.t), nf, ny, nx, _hp(vm), _dp(m.t), 0.0, _hp(k), k.shape[0], _dp(out.t),
                                ctypes.byref(L.options(device_inputs=True)))
    assert rc == 0, L.load().oi_last_error()
    ok = f.intact() and m.intact() and out.intact() and same_bits(f.numpy(), fields) and same_bits(m.numpy(), mask)
    return out.numpy(), ok


def ball_query_raw(pts, q, r, idx=None, cap=0, device=False):
    """One oi_ball_query call: (rc, offs).  ``pts`` / ``q`` / ``idx`` are numpy
    arrays (host mode) or torch device tensors (device mode); idx may be None."""
    from optimalinterpolation_amd import _lib as L
    M, Q = int(pts.shape[0]), int(q.shape[0])
    offs = np.full(Q + 2, SENT_I, dtype=np.int64)           # one guard element behind offs[Q]
    p = (_dp if device else _hp)
    rc = lib().oi_ball_query(p(pts) if M else None, M, p(q), Q, float(r), _hp(offs, ctypes.c_int64),
                             p(idx, ctypes.c_int64) if idx is not None else None, int(cap),
                             ctypes.byref(L.options(device_inputs=device)))
    assert offs[-1] == SENT_I
    return rc, offs[:-1]


def ball_query_device(pts, q, r, extra=0):
    """Both calls of the radius query in device mode, on guarded buffers: the
    sizing call (idx = NULL), then the fill with cap = total + extra.  Returns
    (offs, idx [total], guards intact)."""
    gp = Guarded(pts.shape if len(pts) else (1, 2), init=pts if len(pts) else None)
    gq = Guarded(q.shape, init=q)
    pt = gp.t[:len(pts)]
    rc, offs = ball_query_raw(pt, gq.t, r, device=True)
    assert rc == 0
    total = int(offs[-1])
    gi = Guarded((total + extra,), dtype='int64', pad=PAD)
    gi.t.fill_(SENT_I)
    rc, offs2 = ball_query_raw(pt, gq.t, r, idx=gi.t, cap=total + extra, device=True)
    assert rc == 0 and np.array_equal(offs, offs2)
    got = gi.numpy()
    ok = gp.intact() and gq.intact() and gi.intact() and bool(np.all(got[total:] == SENT_I))
    ok = ok and same_bits(gq.numpy(), q) and (not len(pts) or same_bits(gp.numpy(), pts))
    return offs, got[:total], ok


def ball_count_launch(pts, q, r2):
    """oi_launch_ball_count on guarded torch tensors: (bbox [nchunk, 4], counts
    [Q], guards intact).  bbox is guarded beyond 4 * nchunk doubles, counts
    beyond Q."""
    import torch
    M, Q = len(pts), len(q)
    nchunk = (M + CHUNK - 1) // CHUNK
    gp, gq = Guarded(pts.shape, init=pts), Guarded(q.shape, init=q)
    gb, gc = Guarded((nchunk, 4)), Guarded((Q,), dtype='int64')
    st = torch.cuda.current_stream().cuda_stream or None
    rc = lib().oi_launch_ball_count(gp.t.data_ptr(), M, gb.t.data_ptr(), gq.t.data_ptr(), Q, float(r2),
                                    gc.t.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0
    return gb.numpy(), gc.numpy(), gp.intact() and gq.intact() and gb.intact() and gc.intact()


def gather_device(cols, idx):
    """oi_gather_rows in device mode on guarded buffers: (xyt [N, 3], z [N],
    guards intact).  xyt is guarded beyond 3 N doubles, zout beyond N."""
    from optimalinterpolation_amd import _lib as L
    M, N = len(cols[0]), len(idx)
    gc = [Guarded((M,), init=c) for c in cols]
    gi = Guarded((N,), dtype='int64', init=idx)
    gx, gz = Guarded((N, 3)), Guarded((N,))
    rc = lib().oi_gather_rows(*[_dp(g.t) for g in gc], M, _dp(gi.t, ctypes.c_int64), N, _dp(gx.t), _dp(gz.t),
                              ctypes.byref(L.options(device_inputs=True)))
    assert rc == 0, L.load().oi_last_error()
    ok = all(g.intact() and same_bits(g.numpy(), c) for g, c in zip(gc, cols))
    return gx.numpy(), gz.numpy(), ok and gi.intact() and gx.intact() and gz.intact()
