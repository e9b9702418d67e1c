"""Joint posterior draws of one cell in plain numpy: the reference of
``oi_gpr_sample`` (include/oi.h; tests/test_gpu_sample.py).

``philox4x32_10`` restates the counter-based generator (Salmon et al., SC'11),
``normals`` the header's mapping from (seed, stream, element) to a standard
normal -- in float64, or in longdouble from the same bits -- and ``sample_cell``
the draw itself on ``oracle.gp_oracle.matern32`` and ``np.linalg.cholesky``:
    C = cov + (noise ? sn2 : 0) I + jitter I = Lc Lc'
    samples[t, s] = fs[t] + sum_u Lc[t, u] Xi[u, s]
with fs and cov as ``_ref_cell`` of tests/test_gpu_predict_multi.py forms them.
"""
import numpy as np

from oracle import gp_oracle as O

M0, M1 = 0xD2511F53, 0xCD9E8D57        # the round's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85        # the key schedule's Weyl constants
MASK = 0xFFFFFFFF
U64 = 0xFFFFFFFFFFFFFFFF
TWO_PI = 2 * np.pi


def philox4x32_10(counter, key):
    """Ten rounds on arrays of counters [.. x 4] and keys [.. x 2] (uint32
    values; broadcast against each other): the output words [.. x 4] as uint64
    arrays holding 32-bit values."""
    c = [np.asarray(counter, dtype=np.uint64)[..., q] & np.uint64(MASK) for q in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., q] & np.uint64(MASK) for q in range(2)]
    m32 = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]       # 32 x 32 -> 64 bits, no overflow
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def block_words(seed, stream, blocks):
    """The four words of blocks ``blocks`` (uint64 array) of (seed, stream)."""
    b = np.asarray(blocks, dtype=np.uint64)
    seed, stream = int(seed) & U64, int(stream) & U64
    ctr = np.stack([b & np.uint64(MASK), b >> np.uint64(32), np.full_like(b, stream & MASK),
                    np.full_like(b, stream >> 32)], axis=-1)
    return philox4x32_10(ctr, np.array([seed & MASK, seed >> 32], dtype=np.uint64))


def normals(seed, stream, first, count, dtype=np.float64):
    """Elements first .. first + count - 1 of the stream's standard normals,
    evaluated in ``dtype`` (float64: numpy's own evaluation of the mapping;
    longdouble: the yardstick, from the same bits).  Also returns r."""
    e = (np.arange(count, dtype=np.uint64) + np.uint64(int(first) & U64))
    w = block_words(seed, stream, e >> np.uint64(1))
    k1 = (w[..., 0] << np.uint64(21)) | (w[..., 1] >> np.uint64(11))
    k2 = (w[..., 2] << np.uint64(21)) | (w[..., 3] >> np.uint64(11))
    scale = dtype(2.0) ** -53
    u1 = (k1 + np.uint64(1)).astype(dtype) * scale
    u2 = k2.astype(dtype) * scale
    r = np.sqrt(-2 * np.log(u1))
    if dtype is np.float64:
        th = TWO_PI * u2                 # the double 2 * np.pi, one rounding
    else:
        th = dtype(TWO_PI) * u2          # the same constant, the product exact to the wider format
    odd = (e & np.uint64(1)).astype(bool)
    return np.where(odd, r * np.sin(th), r * np.cos(th)), r


def cell_xi(seed, stream, nt, nsamp, dtype=np.float64):
    """Xi [nt x nsamp] of one cell: element e = s nt + t at [t, s]."""
    return normals(seed, stream, 0, nt * nsamp, dtype)[0].reshape(nsamp, nt).T


def posterior(x, y, xs, mean, hyp):
    """(fs [nt], cov [nt x nt]) of one cell; LinAlgError propagates."""
    ell, sf2, sn2 = list(hyp[:3]), hyp[3], hyp[4]
    n, nt = len(y), len(xs)
    Kxs = O.matern32(xs, ell, sf2) if nt else np.zeros((0, 0))
    if n == 0:
        return np.full(nt, mean), Kxs
    Kx = O.matern32(x, ell, sf2)
    L = np.linalg.cholesky(Kx + np.eye(n) * sn2)
    if nt == 0:
        return np.zeros(0), Kxs
    resid = y - np.ones(n) * mean
    A = np.linalg.solve(L.T, np.linalg.solve(L, resid))
    Kxsx = O.matern32(x, ell, sf2, xs=xs)
    v = np.linalg.solve(L, Kxsx)
    return mean + np.dot(Kxsx.T, A), Kxs - np.dot(v.T, v)


def draw_cov(cov, sn2, noise, jitter):
    """C, the matrix that is factored."""
    nt = len(cov)
    return cov + np.eye(nt) * (sn2 if noise else 0.0) + np.eye(nt) * jitter


def sample_cell(x, y, xs, mean, hyp, xi, noise=False, jitter=0.0):
    """(samples [nt x nsamp], fs [nt], sd [nt], C, Lc) of one cell for the
    normals ``xi`` [nt x nsamp]."""
    fs, cov = posterior(x, y, xs, mean, hyp)
    nt = len(fs)
    C = draw_cov(cov, hyp[4], noise, jitter)
    Lc = np.linalg.cholesky(C) if nt else np.zeros((0, 0))
    xi = np.asarray(xi, dtype=np.float64)
    assert xi.ndim == 2 and xi.shape[0] == nt
    return fs[:, None] + np.dot(Lc, xi), fs, np.sqrt(cov.diagonal()), C, Lc
