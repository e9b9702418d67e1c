"""Leave-group-out cross-validation of one cell in plain numpy: the references
of ``oi_gpr_lgo`` (tests/test_gpu_lgo.py), on ``oracle.gp_oracle.matern32``,
and the inputs that both test files share.

``lgo_closed`` evaluates the block form of GPML 5.4.2
    r = z - mean, K~ = K + sn2 I, alpha = K~^-1 r, Q = K~^-1
    per group G:  Sigma_G = Q_GG^-1, mu_G = z_G - Q_GG^-1 alpha_G,
    sd_i = sqrt([Q_GG^-1]_ii), d2_G = alpha_G' Q_GG^-1 alpha_G,
    lpd_G = -d2_G / 2 + sum_k log C_kk - g log(2 pi) / 2  (Q_GG = C C')
and ``lgo_brute`` what it stands for: one fit per group on the observations
outside it, the group's observations predicted with their full covariance
(noise included) and scored with the joint normal density.  Both return
(mu [n], sd [n], lpd [n], d2 [n], lpl): lpd and d2 hold the group's value at
every member, lpl adds lpd_G in the order of the groups' first appearance.
``np.linalg.LinAlgError`` propagates.

``plan`` restates the library's host plan (``oi_test_lgo_plan``), ``cell_form``
its workspace count (``oi_test_lgo_cell_doubles``).
"""
import ctypes

import numpy as np

from oracle import gp_oracle as O
import dense_ref

HYP = np.array([2e5, 2e5, 6.0, 5e-3, 1e-3])   # the leave-one-out tests' timing hypers
LOG2PI = np.log(2 * np.pi)


def _split(hyp):
    return list(hyp[:3]), hyp[3], hyp[4]


def groups_of(group):
    """Index arrays of the groups, in the order of first appearance; members
    in observation order."""
    group = np.asarray(group, dtype=np.int64).reshape(-1)
    order, members = {}, []
    for i, g in enumerate(group.tolist()):
        if g not in order:
            order[g] = len(members)
            members.append([])
        members[order[g]].append(i)
    return [np.array(m, dtype=np.int64) for m in members]


def _prep(x, z, hyp):
    ell, sf2, sn2 = _split(hyp)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    n = len(z)
    K = O.matern32(x, ell, sf2) + np.eye(n) * sn2 if n else np.zeros((0, 0))
    return z, n, K


def lgo_closed(x, z, group, mean, hyp):
    z, n, K = _prep(x, z, hyp)
    mu, sd, lpd, d2 = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    if n == 0:
        return mu, sd, lpd, d2, 0.0
    L = np.linalg.cholesky(K)
    W = np.linalg.solve(L, np.eye(n))             # L^-1
    Q = W.T @ W
    alpha = W.T @ (W @ (z - mean))
    lpl = 0.0
    for G in groups_of(group):
        C = np.linalg.cholesky(Q[np.ix_(G, G)])
        X = np.linalg.solve(C, np.column_stack([np.eye(len(G)), alpha[G]])).T    # [I ; alpha'] C^-T
        mu[G] = z[G] - X[:-1] @ X[-1]
        sd[G] = np.sqrt((X[:-1] * X[:-1]).sum(axis=1))
        d2[G] = X[-1] @ X[-1]
        lpd[G] = -0.5 * d2[G[0]] + np.log(np.diag(C)).sum() - 0.5 * len(G) * LOG2PI
        lpl += lpd[G[0]]
    return mu, sd, lpd, d2, float(lpl)


def lgo_brute(x, z, group, mean, hyp):
    z, n, K = _prep(x, z, hyp)
    mu, sd, lpd, d2 = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    if n == 0:
        return mu, sd, lpd, d2, 0.0
    np.linalg.cholesky(K)                         # a non-PD cell fails as a whole, as the closed form does
    lpl = 0.0
    for G in groups_of(group):
        R = np.setdiff1d(np.arange(n), G)
        m, S = np.full(len(G), float(mean)), K[np.ix_(G, G)]
        if len(R):                                # nothing outside the group: the prior
            L = np.linalg.cholesky(K[np.ix_(R, R)])
            v = np.linalg.solve(L, K[np.ix_(R, G)])
            m = mean + v.T @ np.linalg.solve(L, z[R] - mean)
            S = S - v.T @ v
        Ls = np.linalg.cholesky(S)
        u = np.linalg.solve(Ls, z[G] - m)
        mu[G], sd[G], d2[G] = m, np.sqrt(np.diag(S)), u @ u
        lpd[G] = -0.5 * (u @ u) - np.log(np.diag(Ls)).sum() - 0.5 * len(G) * LOG2PI
        lpl += lpd[G[0]]
    return mu, sd, lpd, d2, float(lpl)


def errors(got, ref):
    """The five figures the bounds are on: max |dmu| / max(1, |mu|), |dsd| / sd,
    |dlpd| / max(1, |lpd|), |dd2| / max(1, d2), |dlpl| / max(1, |lpl|)."""
    one = lambda a: np.maximum(1.0, np.abs(a))
    return (np.max(np.abs(got[0] - ref[0]) / one(ref[0]), initial=0.0),
            np.max(np.abs(got[1] - ref[1]) / ref[1], initial=0.0),
            np.max(np.abs(got[2] - ref[2]) / one(ref[2]), initial=0.0),
            np.max(np.abs(got[3] - ref[3]) / one(ref[3]), initial=0.0),
            abs(got[4] - ref[4]) / max(1.0, abs(ref[4])))


# ----------------------------------------------------------- shared inputs --

def interleave(sizes, seed):
    """Group indices 0 .. len(sizes) - 1 for sum(sizes) observations, shuffled so
    that group q still appears first before group q + 1 does: after the
    library's sort the groups lie in this order, with these sizes."""
    rng = np.random.default_rng([int(seed), len(sizes)])
    left = list(sizes)
    opened, out = 0, []
    for _ in range(sum(sizes)):
        cand = [q for q in range(min(opened + 1, len(sizes))) if left[q] > 0]
        w = np.array([left[q] for q in cand], dtype=np.float64)
        q = cand[rng.choice(len(cand), p=w / w.sum())]
        opened = max(opened, q + 1)
        left[q] -= 1
        out.append(q)
    return np.array(out, dtype=np.int64)


def odd_labels(gid, seed):
    """Distinct labels for the group indices, in no order: negative ones and
    ones near 2^62."""
    rng = np.random.default_rng([int(seed), 77])
    k = int(gid.max()) + 1 if len(gid) else 0
    pool = np.concatenate([(1 << 62) - np.arange(k), -(1 << 62) + np.arange(k), np.arange(k) - k // 2])
    return rng.permutation(pool)[:k][gid]


# group sizes in sorted order; the starts c0 (mod 64) they produce are in the comments
SIZES_333 = [1, 129, 2, 59, 65, 64, 13]                         # 129 at 1, 65 at 63, 64 at 0
SIZES_700 = [63, 130, 64, 65, 1, 61, 128, 2, 61, 2, 1, 122]     # 63 at 0, 130 at 63 (three boundaries), 64 and
                                                                # 65 at 1, 128 and 2 at 0, 2 at 63, 1 at 1
SIZES_65 = [13, 1, 25, 24, 2]

# name -> (distinct sites m, observations n, group sizes in sorted order or a word)
SPECS = [('one', 1, 1, [1]),
         ('two', 2, 2, [1, 1]),
         ('n63-singletons', 55, 63, [1] * 63),
         ('n64-whole', 60, 64, [64]),
         ('n65-five', 60, 65, SIZES_65),                 # the last block has one row
         ('n130-singletons', 110, 130, [1] * 130),       # g = 1 at every offset
         ('n130-sites', 90, 130, 'sites'),
         ('n333', 300, 333, SIZES_333),
         ('n700', 600, 700, SIZES_700)]


def site_labels(x):
    """gpr.site_groups for one cell, restated: the row of the first bitwise-equal (x, y, t)."""
    first, out = {}, np.empty(len(x), dtype=np.int64)
    for i, row in enumerate(np.ascontiguousarray(x, dtype=np.float64)):
        out[i] = first.setdefault(row.tobytes(), i)
    return out


_cases = None


def cases():
    """[(name, x, z, labels, sizes after the sort)], and the cells' common mean."""
    global _cases
    if _cases is None:
        out, mean = [], None
        for q, (name, m, n, sizes) in enumerate(SPECS):
            cell = dense_ref.exact_cell(m, n, seed=100 + q)
            x, z, _ = cell.cell(0)
            mean = cell.mean
            if isinstance(sizes, str):
                lab = site_labels(x)
                sizes = [len(g) for g in groups_of(lab)]
            else:
                lab = odd_labels(interleave(sizes, q), q)
            out.append((name, x, z, lab, list(sizes)))
        _cases = (out, mean)
    return _cases


_refs = {}


def refs(name):
    """(closed, brute) of a case, computed once."""
    if name not in _refs:
        cs, mean = cases()
        _, x, z, lab, _ = next(c for c in cs if c[0] == name)
        _refs[name] = (lgo_closed(x, z, lab, mean, HYP), lgo_brute(x, z, lab, mean, HYP))
    return _refs[name]


def batch():
    """The cases as one ragged batch: (xyt, z, offs, labels, mean, hyp)."""
    cs, mean = cases()
    offs = np.concatenate([[0], np.cumsum([len(c[2]) for c in cs])])
    return (np.concatenate([c[1] for c in cs]), np.concatenate([c[2] for c in cs]), offs,
            np.concatenate([c[3] for c in cs]), mean, np.tile(HYP, (len(cs), 1)))


# ------------------------------------------------- the host plan, restated --

def up(v, q):
    return (v + q - 1) // q * q


def plan(group):
    """(perm, group starts, group sizes, tiles): sorted row k holds observation
    perm[k]; the aligned 64 x 64 tiles (A, B), A >= B, of K~^-1 that some group
    touches, each once, in lexicographic order."""
    gs = groups_of(group)
    perm = np.concatenate(gs) if gs else np.zeros(0, dtype=np.int64)
    size = np.array([len(g) for g in gs], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(size)])[:-1].astype(np.int64)
    tiles = set()
    for c0, g in zip(start, size):
        bA, bE = c0 // 64, (c0 + g - 1) // 64
        tiles |= {(A, B) for A in range(bA, bE + 1) for B in range(bA, A + 1)}
    return perm, start, size, sorted(tiles)


def cell_form(n, sizes, host):
    """The planner's count for one cell: leave-one-out's (workspace_ref.loo_form)
    plus alpha, lpd and d2 per row, lpd_G and info per group, the gathered inputs
    (device inputs) and per group the padded block, its diagonal-block inverses
    and X."""
    Np = up(n, 64)
    loo = (up(3 * n, 32) + Np * Np + 2 * Np * 64 + up(n, 32) + up(Np // 64, 32) + 2 * n
           + (4 * n if host else 0) + 2)
    per = sum(up(g, 64) ** 2 + 64 * up(g, 64) + up((g + 1) * g, 32) for g in sizes)
    return loo + up(Np, 32) + per + 2 * n + 2 * len(sizes) + (0 if host else 4 * n)


def lib_plan(group):
    from optimalinterpolation_amd import _lib
    fn = _lib.load().oi_test_lgo_plan
    P = ctypes.POINTER(ctypes.c_int64)
    fn.restype, fn.argtypes = ctypes.c_int64, [P, ctypes.c_int64, P, P, P, P, P, ctypes.c_int64]
    group = np.ascontiguousarray(group, dtype=np.int64)
    n = len(group)
    T = (n + 63) // 64
    cap = T * (T + 1) // 2 + 1
    perm, start, size = (np.full(max(n, 1), -1, dtype=np.int64) for _ in range(3))
    ng, tiles = np.zeros(1, dtype=np.int64), np.full(2 * cap, -1, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(P)
    nt = fn(p(group), n, p(perm), p(start), p(size), p(ng), p(tiles), cap)
    assert nt < cap
    k = int(ng[0])
    return perm[:n], start[:k], size[:k], [tuple(t) for t in tiles[:2 * nt].reshape(-1, 2).tolist()]


def lib_cell_doubles(n, sizes, host):
    from optimalinterpolation_amd import _lib
    fn = _lib.load().oi_test_lgo_cell_doubles
    fn.restype = ctypes.c_int64
    fn.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int32]
    s = np.ascontiguousarray(sizes, dtype=np.int64)
    return fn(n, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(s), 2 if host else 0)
