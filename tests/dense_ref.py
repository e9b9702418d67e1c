"""Harness for the per-tile tests of the dense-GP kernels (csrc/oi_kernels.hip):
cells with an exact number of distinct sites, a ctypes mirror of OiCell with
poisoned, guarded device workspaces, a replay of the engine's launch sequence
(oi_engine.cpp launch_round) through the exported launchers, readers of the
tiled device state, a reference of every quantity in np.longdouble -- built
from the same fp64 inputs, never with the code under test -- and a checker
that names the worst tile.  A plain module (tests import it), not a conftest.

Shapes: the kernels tile the m distinct SITES of a cell, T = ceil(m / 64)
block rows with rT = m - 64 (T - 1) rows in the last one; synthetic.make_cells
snaps observations to a lattice, so its sizes are observation counts, not m.
"""
import ctypes
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from optimalinterpolation_amd import synthetic  # noqa: E402

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
NB = 64
TILE = NB * NB
GUARD_TILES = 2      # after L, W, Dinv
GUARD_WORDS = 64     # after vec, part
MODE_EVAL, MODE_PREDICT = 0, 1
OUT_N, OUT_STATUS = 8, 7
DUP_NONPD_TAU = 1e-18          # OI_DUP_NONPD_TAU
SQRT3_64 = 1.7320508075688772  # SQRT3 of oi_kernels.hip
# unwritten workspace and guards: a quiet NaN with a payload (tests/oila_ref.py)
SENT_BITS = np.uint64(0x7FF85EED0BADC0DE)
SENT = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]

# tolerance factors of compare(): err <= K_Q[q] * err64 ("Per-tile
# tests"): the worst err / err64 measured on the MI355X over the grid of
# tests/test_gpu_dense_kernels.py (profiles/dense_kernels/ratios.json) times
# the spread max / median of err64 over the grid's cells, rounded up to a
# power of two
K_Q = {'L': 32.0, 'W': 4.0, 'Dinv': 4.0, 'z': 16.0, 'alpha': 8.0, 'v': 8.0, 'logdet': 8.0, 'pred': 2048.0,
       'grad': 64.0}
QUANTITIES = tuple(K_Q)


def tiles_of(m):
    return (m + NB - 1) // NB


def tri(i):
    return i * (i + 1) // 2


def part_size(T):
    return 5 * tri(T) + 5 * T


def part_logdet(T):
    return 5 * tri(T) + T


def part_pred(T):
    return 5 * tri(T) + 2 * T


# ------------------------------------------------------------------ cells --
def _field(x, y, t):
    return 0.25 + 0.05 * np.sin(x / 2e5) * np.cos(y / 3e5) + 0.01 * t


def exact_cell(m, n_obs=None, seed=0, lattice=True, centre=None):
    """One synthetic cell (a RaggedCells of one cell) with exactly ``m``
    bitwise-distinct sites: ``m`` triples drawn without replacement from the
    25 km lattice x 9 days inside the 300 km disc (``lattice=False``: continuous
    positions, for m beyond the ~4070 lattice triples), ``n_obs - m`` further
    observations that repeat sites, observation order shuffled.  Coordinates
    are positive (no -0.0)."""
    n_obs = m if n_obs is None else int(n_obs)
    assert n_obs >= m >= 1
    rng = np.random.default_rng([int(seed), int(m), int(n_obs), 4242])
    if centre is None:
        cen = synthetic.day_centres()
        centre = cen[rng.integers(0, len(cen))]
    cx, cy = float(centre[0]), float(centre[1])
    if lattice:
        k = int(synthetic.RADIUS_M // synthetic.GRID_M)
        g = np.arange(-k, k + 1) * synthetic.GRID_M
        gx, gy = np.meshgrid(g, g, indexing='ij')
        inside = gx ** 2 + gy ** 2 <= synthetic.RADIUS_M ** 2
        px, py = cx + gx[inside], cy + gy[inside]
        nt = len(px) * synthetic.T_DAYS
        assert m <= nt, f"only {nt} lattice triples in the disc"
        pick = rng.choice(nt, m, replace=False)
        sites = np.stack([px[pick // synthetic.T_DAYS], py[pick // synthetic.T_DAYS],
                          (pick % synthetic.T_DAYS).astype(np.float64)], axis=1)
    else:
        r = synthetic.RADIUS_M * np.sqrt(rng.random(m))
        th = 2 * np.pi * rng.random(m)
        sites = np.stack([cx + r * np.cos(th), cy + r * np.sin(th),
                          rng.integers(0, synthetic.T_DAYS, m).astype(np.float64)], axis=1)
    idx = np.concatenate([np.arange(m), rng.integers(0, m, n_obs - m)])
    idx = idx[rng.permutation(n_obs)]
    xyt = np.ascontiguousarray(sites[idx])
    z = _field(xyt[:, 0], xyt[:, 1], xyt[:, 2]) + rng.normal(0.0, 0.02, n_obs)
    assert (xyt[:, :2] > 0).all() and not np.signbit(xyt).any()
    assert len(np.unique(xyt, axis=0)) == m
    xs = np.array([[cx, cy, float(synthetic.T_MID)]])
    return synthetic.RaggedCells(xyt, z, np.array([0, n_obs]), xs, synthetic.PRIOR_MEAN)


def concat_cells(parts):
    xyt = np.concatenate([p.xyt for p in parts])
    z = np.concatenate([p.z for p in parts])
    offs = np.concatenate([[0], np.cumsum([len(p.z) for p in parts])])
    xs = np.concatenate([p.xs for p in parts])
    return synthetic.RaggedCells(xyt, z, offs, xs, parts[0].mean)


def exact_cells(specs, seed=0, lattice=True):
    """A ragged batch: one exact_cell per entry of ``specs``, each an int m
    (duplicate-free) or a pair (m, n_obs)."""
    parts = []
    for q, s in enumerate(specs):
        m, n_obs = (s, s) if np.ndim(s) == 0 else s
        parts.append(exact_cell(int(m), int(n_obs), seed=(int(seed) * 1000 + q), lattice=lattice))
    return concat_cells(parts)


def site_counts(cells):
    """(n_obs, m, T, rT) of every cell of a ragged batch, counted on the CPU."""
    out = []
    for c in range(cells.ncell):
        x, _, _ = cells.cell(c)
        m = len(np.unique(x, axis=0)) if len(x) else 0
        T = tiles_of(m)
        out.append((len(x), m, T, m - NB * (T - 1) if m else 0))
    return out


def shape_cell(T, rT, extra=0, seed=0):
    return exact_cell(NB * (T - 1) + rT, NB * (T - 1) + rT + extra, seed=seed)


def dedup_np(xyt, r):
    """k_dedup restated: sites in first-occurrence order, per site the count c
    and the sum of r in observation order; v = sum / sqrt(c), d = sqrt(c), and
    SSW = sum (r - site mean)^2 (summed site by site here)."""
    xyt = np.ascontiguousarray(xyt, dtype=np.float64).reshape(-1, 3)
    n = len(xyt)
    first, sid = {}, np.empty(n, dtype=np.int64)
    keys = xyt.view(np.uint64) if n else np.zeros((0, 3), np.uint64)
    for a in range(n):
        # the kernel compares doubles with ==; the cells here hold no -0.0 / NaN
        sid[a] = first.setdefault((int(keys[a, 0]), int(keys[a, 1]), int(keys[a, 2])), len(first))
    m = len(first)
    rs, cnt = np.zeros(m), np.zeros(m)
    for a in range(n):           # observation order
        rs[sid[a]] += r[a]
        cnt[sid[a]] += 1.0
    fo = np.full(m, -1, dtype=np.int64)
    for a in range(n - 1, -1, -1):
        fo[sid[a]] = a
    sites = xyt[fo] if m else np.zeros((0, 3))
    d = np.sqrt(cnt)
    rbar = rs / np.maximum(cnt, 1.0)
    e = np.asarray(r, dtype=np.float64) - rbar[sid]
    terms = e * e
    return sites, rs / d, d, float(np.sum(terms)), float(np.sum(np.abs(terms))), sid, fo


class Cell:
    """One cell of the harness: observations, the sites the kernels run on
    (dedup_np), hypers (lx, ly, lt, sf2, sn2), mode."""

    def __init__(self, rc, hyp, mode=MODE_EVAL, c=0):
        x, z, xs = rc.cell(c)
        self.xyt_obs, self.y, self.xs, self.mean = x.copy(), z.copy(), xs[0].copy(), rc.mean
        self.n_obs = len(z)
        self.r_obs = self.y - self.mean
        self.sites, self.v, self.dw, self.ssw = dedup_np(x, self.r_obs)[:4]
        self.m = len(self.v)
        self.T = tiles_of(self.m)
        self.rT = self.m - NB * (self.T - 1)
        self.hyp = np.array(hyp, dtype=np.float64)
        self.mode = mode

    def with_(self, hyp=None, mode=None):
        import copy
        c = copy.copy(self)
        if hyp is not None:
            c.hyp = np.array(hyp, dtype=np.float64)
        if mode is not None:
            c.mode = mode
        return c


def hyp_of_h(h):
    """exp(h[:5]) as the engine forms it (std::exp = libm's, which math.exp calls)."""
    return np.array([math.exp(float(v)) for v in np.asarray(h)[:5]])


# the T1 comparison of tests/test_gpu_parity.py, for tests that
# hold the C ABI against the oracle
def grad_scale(h, x, y, mX):
    """S_j = 1/2 sum |Q o dK_j| (j < 4) and sn2 sum |diag Q| at h, oracle-side."""
    from oracle import gp_oracle as O
    n = len(y)
    sf2, sn2 = np.exp(h[3]), np.exp(h[4])
    K, dK = O.matern32(x, np.exp(h[:3]), sf2, grad=True)
    Kinv = np.linalg.inv(K + np.eye(n) * sn2)
    a = Kinv @ (y - mX)
    Q = Kinv - np.outer(a, a)
    return np.array([np.abs(Q * dK[0]).sum() / 2, np.abs(Q * dK[1]).sum() / 2, np.abs(Q * dK[2]).sum() / 2,
                     np.abs(Q * 2 * K).sum() / 2, sn2 * np.abs(np.diag(Q)).sum(), 0.0])


def t1_close(a, b, scale=None, rtol=1e-10):
    """(all |a - b| <= rtol scale, worst ratio); scale defaults to max(1, |b|)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if scale is None:
        scale = np.maximum(1.0, np.abs(b))
    err = np.abs(a - b) / scale
    return bool(np.all(err <= rtol)), float(np.max(err))


# ----------------------------------------------------------- device mirror --
c_dp = ctypes.c_void_p


class OiCell(ctypes.Structure):   # csrc/oi_device.h
    _fields_ = [('L', c_dp), ('W', c_dp), ('Dinv', c_dp), ('vec', c_dp), ('part', c_dp), ('xyt', c_dp),
                ('r', c_dp), ('dw', c_dp), ('out', c_dp), ('status', c_dp),
                ('n', ctypes.c_int32), ('T', ctypes.c_int32), ('mode', ctypes.c_int32), ('n_obs', ctypes.c_int32),
                ('hyp', ctypes.c_double * 5), ('xs', ctypes.c_double * 3), ('mean', ctypes.c_double),
                ('ssw', ctypes.c_double), ('pad2_', ctypes.c_double)]


_lib = None


def lib():
    """liboi.so with the kernel launchers of oi_device.h bound."""
    global _lib
    if _lib is None:
        from optimalinterpolation_amd import _lib as L
        h = L.load()
        P, I, V = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
        sig = {'oi_launch_diag_factor': [P, P, I, I, V],
               'oi_launch_chol_panel': [P, P, I, I, I, I, I, V],
               'oi_launch_panel4': [P, P, I, I, I, I, I, V],
               'oi_launch_panel_even': [P, P, I, I, I, I, I, V],
               'oi_launch_lauum_grad': [P, P, I, I, V],
               'oi_launch_finalize': [P, P, I, P, P, ctypes.c_ulonglong, V],
               'oi_launch_dedup': [P, P, P, I, I, I, P, P, P, P, P, V],
               'oi_launch_residual': [P, P, ctypes.c_double, P, ctypes.c_int64, V],
               'oi_test_sizeof_cell': []}
        for name, args in sig.items():
            f = getattr(h, name)
            f.argtypes, f.restype = args, ctypes.c_int
        _lib = h
    return _lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream or None


def _poison(n):
    import torch
    return torch.from_numpy(np.full(n, SENT)).cuda()


class DevCell:
    """A cell's device workspace, as the engine's admit() lays it out but one
    tensor per array: all SENT, two guard tiles after L / W / Dinv, GUARD_WORDS
    after vec and part; W null for a predicting cell."""

    def __init__(self, cell):
        import torch
        self.cell = cell
        T, nt = cell.T, tri(cell.T)
        self.L = _poison((nt + GUARD_TILES) * TILE)
        self.W = _poison((nt + GUARD_TILES) * TILE) if cell.mode == MODE_EVAL else None
        self.Dinv = _poison((T + GUARD_TILES) * TILE)
        self.vec = _poison(4 * T * NB + GUARD_WORDS)
        self.part = _poison(part_size(T) + GUARD_WORDS)
        self.out = _poison(OUT_N + GUARD_WORDS)
        self.status = torch.zeros(4, dtype=torch.int32, device='cuda')
        self.xyt = torch.from_numpy(np.ascontiguousarray(cell.sites)).cuda()
        self.r = torch.from_numpy(np.ascontiguousarray(cell.v)).cuda()
        self.dw = torch.from_numpy(np.ascontiguousarray(cell.dw)).cuda()

    def record(self):
        c = self.cell
        d = OiCell()
        d.L, d.Dinv, d.vec, d.part = (self.L.data_ptr(), self.Dinv.data_ptr(), self.vec.data_ptr(),
                                      self.part.data_ptr())
        d.W = self.W.data_ptr() if self.W is not None else None
        d.xyt, d.r, d.dw = self.xyt.data_ptr(), self.r.data_ptr(), self.dw.data_ptr()
        d.out, d.status = self.out.data_ptr(), self.status.data_ptr()
        d.n, d.T, d.mode, d.n_obs = c.m, c.T, c.mode, c.n_obs
        for k in range(5):
            d.hyp[k] = float(c.hyp[k])
        for k in range(3):
            d.xs[k] = float(c.xs[k])
        d.mean, d.ssw, d.pad2_ = float(c.mean), float(c.ssw), 0.0
        return d

    def fetch(self):
        """The workspace as on the device now (call after run_round): a State."""
        c = self.cell
        g = lambda t: t.cpu().numpy()
        return State(c.m, c.mode, g(self.L), g(self.W) if self.W is not None else None, g(self.Dinv),
                     g(self.vec), g(self.part), g(self.out), int(self.status[0].item()))


def round_order(cells):
    """The engine's lists: fitting and predicting cells each sorted by T
    descending (stable), merged by T with the fitting cell first on a tie.
    Returns (all, eval) as indices into ``cells``."""
    ev = sorted([k for k, c in enumerate(cells) if c.mode == MODE_EVAL], key=lambda k: -cells[k].T)
    pr = sorted([k for k, c in enumerate(cells) if c.mode != MODE_EVAL], key=lambda k: -cells[k].T)
    al, a, b = [], 0, 0
    while a < len(ev) or b < len(pr):
        if b >= len(pr) or (a < len(ev) and not cells[pr[b]].T > cells[ev[a]].T):
            al.append(ev[a])
            a += 1
        else:
            al.append(pr[b])
            b += 1
    return al, ev


def run_round(dcells, panel='even', fuse=True, upto=None):
    """One round of the engine over ``dcells`` (DevCell list), launch for
    launch as oi_engine.cpp launch_round issues it, on torch's current stream:
    k_diag_factor4w(0); per block column j the even panel (``panel``: 'even' =
    k_panel_even, '4' = k_panel4) or k_chol_panel, over the cnt cells with
    T > j, and without ``fuse`` k_diag_factor4w(j) before it; the last column
    skipped when no cell is fitting; then k_lauum_grad1 over the fitting cells
    and k_finalize.  ``upto``: stop after column ``upto``'s panel (and, without
    ``fuse``, the factor of diagonal tile upto + 1) -- no k_lauum_grad1, no
    k_finalize.  Returns the launch log."""
    import torch
    assert panel in ('even', '4')
    h = lib()
    assert ctypes.sizeof(OiCell) == h.oi_test_sizeof_cell()
    cells = [d.cell for d in dcells]
    al, ev = round_order(cells)
    na, ne = len(al), len(ev)
    recs = (OiCell * len(dcells))(*[d.record() for d in dcells])
    dc = torch.from_numpy(np.frombuffer(bytes(recs), dtype=np.uint8).copy()).cuda()
    l_all = torch.tensor(al, dtype=torch.int32).cuda()
    l_ev = torch.tensor(ev if ev else [0], dtype=torch.int32).cuda()
    done = torch.zeros(16, dtype=torch.int32, device='cuda')
    for d in dcells:
        d.status.zero_()
    maxT = cells[al[0]].T if na else 0
    maxTe = cells[ev[0]].T if ne else 0
    st, log, rc = _stream(), [], 0
    fuse_i, trtri = (1 if fuse else 0), (1 if ne > 0 else 0)

    def launch(name, *args):
        nonlocal rc
        log.append((name,) + args)
        rc |= getattr(h, 'oi_launch_' + name)(dc.data_ptr(), *args, st)

    stopped = False
    for j in range(maxT):
        cnt = sum(1 for k in al if cells[k].T > j)
        if j == 0 or not fuse:
            launch('diag_factor', l_all.data_ptr(), cnt, j)
        if not (j == maxT - 1 and ne == 0):
            kind = 'chol_panel' if j % 2 else ('panel4' if panel == '4' else 'panel_even')
            launch(kind, l_all.data_ptr(), cnt, maxT, j, trtri, fuse_i)
        if upto is not None and j == upto:
            if not fuse and j + 1 < maxT:
                launch('diag_factor', l_all.data_ptr(), sum(1 for k in al if cells[k].T > j + 1), j + 1)
            stopped = True
            break
    if not stopped:
        if ne > 0:
            launch('lauum_grad', l_ev.data_ptr(), ne, maxTe)
        log.append(('finalize', na))
        rc |= h.oi_launch_finalize(dc.data_ptr(), l_all.data_ptr(), na, done.data_ptr(), None, 1, st)
    torch.cuda.synchronize()
    assert rc == 0, "a kernel launch failed"
    del recs
    return log


# ----------------------------------------------------------------- readers --
class State:
    """A cell's workspace as dense arrays.  L[x], W[x], Dinv[j]: tile x =
    i (i + 1) / 2 + j as a 64 x 64 array indexed (row, column) (L and Dinv are
    stored column-major, W row-major), guard tiles at the end; vec
    z | alpha | kstar | v and part (OI_PART_*) with their guard words."""

    def __init__(self, m, mode, L, W, Dinv, vec, part, out, status):
        self.m, self.mode, self.T = m, mode, tiles_of(m)
        self.L = np.ascontiguousarray(np.asarray(L).reshape(-1, NB, NB).transpose(0, 2, 1))
        self.W = np.asarray(W).reshape(-1, NB, NB).copy() if W is not None else None
        self.Dinv = np.ascontiguousarray(np.asarray(Dinv).reshape(-1, NB, NB).transpose(0, 2, 1))
        self.vec, self.part, self.out, self.status = (np.array(vec), np.array(part), np.array(out), status)

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def arrays(self):
        return [a for a in (self.L, self.W, self.Dinv, self.vec, self.part, self.out) if a is not None]

    def same_bits(self, other):
        a, b = self.arrays(), other.arrays()
        return (len(a) == len(b) and self.status == other.status
                and all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b)))

    def poisoned(self):
        """Nothing but status and out written."""
        return all((a.view(np.uint64) == SENT_BITS).all() for a in self.arrays()[:-1])


# --------------------------------------------------------------- reference --
def chol_ld(A):
    """Lower Cholesky factor in longdouble, blocked by 64 columns (left-looking:
    the block column's update is one product, then its 64 columns one by one)."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j0 in range(0, n, NB):
        j1 = min(n, j0 + NB)
        P = A[j0:, j0:j1] - L[j0:, :j0] @ L[j0:j1, :j0].T
        for j in range(j1 - j0):
            c = P[j:, j] - P[j:, :j] @ P[j, :j]
            d = np.sqrt(c[0])
            P[j, j] = d
            P[j + 1:, j] = c[1:] / d
        for j in range(j1 - j0):
            P[:j, j] = 0
        L[j0:, j0:j1] = P
    return L


def trinv_ld(L):
    """Inverse of a lower-triangular matrix, row by row."""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    W = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(L[i, :i] @ W[:i, :i]) if i else np.zeros(0, dtype=LD)
        W[i, :i] = row / L[i, i]
        W[i, i] = LD(1) / L[i, i]
    return W


def gram_lower_ld(W):
    """W^T W of a lower-triangular W, block columns' lower parts only, mirrored."""
    n = W.shape[0]
    G = np.zeros((n, n), dtype=W.dtype)
    for j0 in range(0, n, NB):
        j1 = min(n, j0 + NB)
        G[j0:, j0:j1] = W[j0:, j0:].T @ W[j0:, j0:j1]
    return np.tril(G) + np.tril(G, -1).T


def _kernel_terms(sites, dw, hyp, dt):
    """Scaled coordinates u = sqrt(3) x / ell (stage_sites / amat), Q, e^-Q, Kd,
    the lauum coordinates sqrt(3) (x / ell), in dtype ``dt``."""
    x = np.asarray(sites, dtype=dt)
    ell = np.asarray(hyp[:3], dtype=dt)
    s3 = np.sqrt(dt(3)) if dt is LD else dt(SQRT3_64)
    u = (s3 * x) / ell
    d = u[:, None, :] - u[None, :, :]
    Q = np.sqrt((d * d).sum(-1))
    e = np.exp(-Q)
    Kd = dt(hyp[3]) * ((1 + Q) * e)
    uq = s3 * (x / ell)
    return u, Q, e, Kd, uq


class _Q:
    """The quantities of one cell in one precision (dt = longdouble: the
    reference; float64 with LAPACK: the yardstick err64)."""

    def __init__(self, cell, dt):
        import scipy.linalg as sl
        m, T = cell.m, cell.T
        N = NB * T
        hyp = cell.hyp
        sf2, sn2 = dt(hyp[3]), dt(hyp[4])
        dw = np.asarray(cell.dw, dtype=dt)
        v = np.asarray(cell.v, dtype=dt)
        u, Q, e, Kd, uq = _kernel_terms(cell.sites, dw, hyp, dt)
        M = (dw[:, None] * dw[None, :]) * Kd + sn2 * np.eye(m, dtype=dt)
        self.M = M
        if dt is LD:
            Lm = chol_ld(M)
            Wm = trinv_ld(Lm)
            Minv = gram_lower_ld(Wm)
        else:
            Lm = np.linalg.cholesky(M)
            Wm = sl.solve_triangular(Lm, np.eye(m), lower=True)
            Wm = np.tril(Wm)
            Minv = Wm.T @ Wm
        pad = lambda A: np.block([[A, np.zeros((m, N - m), dtype=dt)],
                                  [np.zeros((N - m, m), dtype=dt), np.eye(N - m, dtype=dt)]])
        self.L, self.W = pad(Lm), pad(Wm)
        if dt is LD:
            self.Dinv = np.stack([trinv_ld(self.L[k * NB:(k + 1) * NB, k * NB:(k + 1) * NB]) for k in range(T)])
        else:
            self.Dinv = np.stack([np.tril(sl.solve_triangular(self.L[k * NB:(k + 1) * NB, k * NB:(k + 1) * NB],
                                                              np.eye(NB), lower=True)) for k in range(T)])
        padv = lambda a: np.concatenate([a, np.zeros(N - m, dtype=dt)])
        z = Wm @ v if dt is LD else sl.solve_triangular(Lm, v, lower=True)
        al = Wm.T @ z if dt is LD else sl.solve_triangular(Lm.T, z, lower=False)
        # k* = D kd* (k_diag_factor4w(0)); v* = L^-1 k*
        xs = (np.sqrt(dt(3)) if dt is LD else dt(SQRT3_64)) * np.asarray(cell.xs, dtype=dt) / np.asarray(hyp[:3], dtype=dt)
        dq = u - xs[None, :]
        Qs = np.sqrt((dq * dq).sum(-1))
        ks = dw * (sf2 * ((1 + Qs) * np.exp(-Qs)))
        vs = Wm @ ks if dt is LD else sl.solve_triangular(Lm, ks, lower=True)
        self.z, self.alpha, self.kstar, self.vstar = padv(z), padv(al), padv(ks), padv(vs)
        # per-block partials and their scales (sums of absolute terms)
        lg = np.log(np.diag(Lm))
        blk = lambda a: np.array([a[k * NB:(k + 1) * NB].sum() for k in range(T)], dtype=dt)
        self.logdet, self.logdet_s = blk(padv(lg)), blk(padv(np.abs(lg)))
        zz, zv, vv = self.z * self.z, self.z * self.vstar, self.vstar * self.vstar
        self.pred = np.stack([blk(zz), blk(zv), blk(vv)], axis=1)
        self.pred_s = np.stack([blk(np.abs(zz)), blk(np.abs(zv)), blk(np.abs(vv))], axis=1)
        # lauum_tile's five partials per lower tile
        w0 = Minv - al[:, None] * al[None, :]
        w = (dw[:, None] * dw[None, :]) * w0
        dq3 = uq[:, None, :] - uq[None, :, :]
        terms = [w * (sf2 * ((dq3[:, :, k] * dq3[:, :, k]) * e)) for k in range(3)] + [w * (2 * Kd)]
        nt = tri(T)
        self.grad, self.grad_s = np.zeros((nt, 5), dtype=dt), np.zeros((nt, 5), dtype=dt)
        for i in range(T):
            for j in range(i + 1):
                a0, a1, b0, b1 = i * NB, min(m, (i + 1) * NB), j * NB, min(m, (j + 1) * NB)
                x = tri(i) + j
                for k in range(4):
                    t = terms[k][a0:a1, b0:b1]
                    t = 2 * t if i != j else 2 * np.tril(t, -1) + np.diag(np.diag(t))
                    self.grad[x, k], self.grad_s[x, k] = t.sum(), np.abs(t).sum()
                if i == j:
                    t = np.diag(w0)[a0:a1]
                    self.grad[x, 4], self.grad_s[x, 4] = t.sum(), np.abs(t).sum()


class Ref:
    """Reference of one cell at its hypers: every quantity in longdouble
    (``q``), the plain fp64 numpy / LAPACK computation of the same (``q64``)
    and, per quantity, scale and err64 = max |q64 - q| / scale floored at eps."""

    def __init__(self, cell):
        self.cell = cell
        self.q, self.q64 = _Q(cell, LD), _Q(cell, np.float64)
        q, q64 = self.q, self.q64
        T = cell.T
        self.scale, self.err64 = {}, {}

        def put(name, a, b, scale):
            scale = np.asarray(scale, dtype=LD)
            self.scale[name] = scale
            with np.errstate(invalid='ignore', divide='ignore'):
                r = np.abs(np.asarray(b, dtype=LD) - a) / scale
            r = np.where(scale == 0, 0, r)
            self.err64[name] = max(float(np.max(r)), EPS)
        for name, a, b in (('L', q.L, q64.L), ('W', q.W, q64.W), ('Dinv', q.Dinv, q64.Dinv), ('z', q.z, q64.z),
                           ('alpha', q.alpha, q64.alpha), ('v', q.vstar, q64.vstar)):
            put(name, a, b, np.max(np.abs(a)))
        put('logdet', q.logdet, q64.logdet, q.logdet_s)
        put('pred', q.pred, q64.pred, q.pred_s)
        put('grad', q.grad, q64.grad, q.grad_s)
        assert T == tiles_of(cell.m)

    # the results k_finalize forms from the partials (site form, oi_device.h)
    def out_eval(self):
        c, q = self.cell, self.q
        sn2, nm = LD(c.hyp[4]), LD(c.n_obs - c.m)
        quad, logdet = q.pred[:, 0].sum(), q.logdet.sum()
        g = q.grad.sum(0)
        ssw = LD(c.ssw)
        log2pi = np.log(LD(2) * np.arctan(LD(1)) * 4)
        nlz = (quad + ssw / sn2) / 2 + (logdet + nm / 2 * np.log(sn2)) + c.n_obs * log2pi / 2
        g4 = sn2 * ((g[4] + nm / sn2) - ssw / (sn2 * sn2))
        return nlz, np.array([g[0] / 2, g[1] / 2, g[2] / 2, g[3] / 2, g4, LD(0)], dtype=LD)

    def out_predict(self):
        c, q = self.cell, self.q
        sf2, sn2, nm = LD(c.hyp[3]), LD(c.hyp[4]), LD(c.n_obs - c.m)
        p = q.pred.sum(0)
        log2pi = np.log(LD(2) * np.arctan(LD(1)) * 4)
        lz = -(p[0] + LD(c.ssw) / sn2) / 2 - (q.logdet.sum() + nm / 2 * np.log(sn2)) - c.n_obs * log2pi / 2
        return LD(c.mean) + p[1], np.sqrt(sf2 - p[2]), lz

    def as_state(self, mode=None):
        """The State a faultless run leaves: the reference rounded to fp64 where
        the kernels write, SENT everywhere else (guards included)."""
        c, q = self.cell, self.q
        mode = c.mode if mode is None else mode
        T, nt = c.T, tri(c.T)
        f = lambda a: np.asarray(a, dtype=np.float64)

        def tiles(A):
            out = np.full((nt + GUARD_TILES, NB, NB), SENT)
            for i in range(T):
                for j in range(i + 1):
                    out[tri(i) + j] = f(A[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB])
            return out
        st = State.__new__(State)
        st.m, st.mode, st.T, st.status = c.m, mode, T, 0
        st.L = tiles(q.L)
        st.W = tiles(q.W) if mode == MODE_EVAL else None
        st.Dinv = np.full((T + GUARD_TILES, NB, NB), SENT)
        st.Dinv[:T] = f(q.Dinv)
        N = NB * T
        st.vec = np.full(4 * N + GUARD_WORDS, SENT)
        st.vec[:N] = f(q.z)
        st.part = np.full(part_size(T) + GUARD_WORDS, SENT)
        st.part[part_logdet(T):part_logdet(T) + T] = f(q.logdet)
        st.out = np.full(OUT_N + GUARD_WORDS, SENT)
        pz = f(q.pred)
        if mode == MODE_EVAL:
            st.vec[N:2 * N] = f(q.alpha)
            st.part[:5 * nt] = f(q.grad).ravel()
            pz[:, 1:] = 0.0   # v = 0 for a fitting cell: z.v = v.v = 0
            nlz, g = self.out_eval()
            st.out[0], st.out[1:7], st.out[OUT_STATUS] = float(nlz), f(g), 0.0
        else:
            st.vec[3 * N:4 * N] = f(q.vstar)
            st.out[:3], st.out[OUT_STATUS] = [float(v) for v in self.out_predict()], 0.0
        st.part[part_pred(T):part_pred(T) + 3 * T] = pz.ravel()
        return st


# ----------------------------------------------------------------- checker --
class Finding:
    """One place where a State departs from its reference: quantity (a name of
    QUANTITIES, or name + '.pad' / '.upper' / '.guard' / '.untouched'), tile
    (i, j) (vectors and per-block partials: (i, None)), the 16 x 16 block
    inside it (vectors: (b, None); partials: (component, None)), and
    ratio = error / bound (inf for a value that must be exact)."""

    def __init__(self, quantity, i, j, block, ratio):
        self.quantity, self.i, self.j, self.block, self.ratio = quantity, i, j, block, ratio

    def key(self):
        return (self.quantity, self.i, self.j, self.block)

    def __repr__(self):
        return f"{self.quantity} tile ({self.i}, {self.j}) block {self.block}: {self.ratio:.3g} x bound"


class Report:
    def __init__(self):
        self.findings = []
        self.ratios = {}     # quantity -> worst err / err64 of this cell

    @property
    def worst(self):
        return max(self.findings, key=lambda f: f.ratio) if self.findings else None

    def keys(self):
        return sorted(f.key() for f in self.findings)

    def __repr__(self):
        if not self.findings:
            return "no finding"
        w = self.worst
        return f"{len(self.findings)} findings, worst: {w!r}; first: {self.findings[:6]!r}"


def _sent(a):
    return np.asarray(a).view(np.uint64) == SENT_BITS


def compare(state, ref, kq=None):
    """Every tile of ``state`` against ``ref``:
    value where the kernels compute (err = |gpu - ref| / scale per 16 x 16 block,
    bound K_Q err64; NaN fails), exact identity / zero in the padding rows and
    columns of L, W, Dinv and zero in the padding of the vectors, exact zero
    above the diagonal of diagonal tiles, SENT bits in guards and in what no
    kernel writes (the kstar slot; alpha and the gradient partials of a
    predicting cell, v of a fitting one; the spare part slots)."""
    kq = K_Q if kq is None else kq
    rep = Report()
    q, m, T, mode = ref.q, state.m, state.T, state.mode
    N, nt = NB * T, tri(T)

    def note(name, ratio):
        rep.ratios[name] = max(rep.ratios.get(name, 0.0), float(ratio))

    def tile_check(name, got, want, i, j, lower_only):
        """64 x 64 tile at block (i, j) of the padded matrix"""
        want64 = np.asarray(want, dtype=np.float64)
        rows = np.arange(NB)[:, None] + NB * i
        cols = np.arange(NB)[None, :] + NB * j
        pad = (rows >= m) | (cols >= m)
        upper = (rows < cols) & ~pad if lower_only else np.zeros_like(pad)
        exact = pad | upper
        with np.errstate(invalid='ignore'):
            err = np.abs(np.asarray(got, dtype=LD) - want) / ref.scale[name]
            r = np.asarray(err / LD(ref.err64[name]), dtype=np.float64)
        bad_val = ~(r <= kq[name]) & ~exact
        bad_pad = (got != want64) & pad
        bad_up = (got != want64) & upper
        if (~exact).any():
            rv = r[~exact]
            note(name, np.inf if np.isnan(rv).any() else rv.max())
        for bi in range(4):
            for bj in range(4):
                s = (slice(16 * bi, 16 * bi + 16), slice(16 * bj, 16 * bj + 16))
                if bad_val[s].any():
                    rr = r[s][bad_val[s]]
                    rep.findings.append(Finding(name, i, j, (bi, bj),
                                                np.inf if np.isnan(rr).any() else rr.max() / kq[name]))
                if bad_pad[s].any():
                    rep.findings.append(Finding(name + '.pad', i, j, (bi, bj), np.inf))
                if bad_up[s].any():
                    rep.findings.append(Finding(name + '.upper', i, j, (bi, bj), np.inf))

    def guard_check(name, a):
        ok = _sent(a).reshape(len(a), -1).all(axis=1)
        for w in np.argwhere(~ok).ravel():
            rep.findings.append(Finding(name, int(w), None, None, np.inf))

    for i in range(T):
        for j in range(i + 1):
            sl = (slice(NB * i, NB * i + NB), slice(NB * j, NB * j + NB))
            tile_check('L', state.L[tri(i) + j], q.L[sl], i, j, i == j)
            if mode == MODE_EVAL:
                tile_check('W', state.W[tri(i) + j], q.W[sl], i, j, i == j)
        tile_check('Dinv', state.Dinv[i], q.Dinv[i], i, i, True)
    guard_check('L.guard', state.L[nt:])
    guard_check('Dinv.guard', state.Dinv[T:])
    if mode == MODE_EVAL:
        guard_check('W.guard', state.W[nt:])
    else:
        assert state.W is None

    def vec_check(name, got, want):
        want64 = np.asarray(want, dtype=np.float64)
        idx = np.arange(N)
        pad = idx >= m
        with np.errstate(invalid='ignore'):
            r = np.asarray(np.abs(np.asarray(got, dtype=LD) - want) / ref.scale[name] / LD(ref.err64[name]),
                           dtype=np.float64)
        bad = np.where(pad, got != want64, ~(r <= kq[name]))
        rv = r[~pad]
        note(name, np.inf if np.isnan(rv).any() else rv.max())
        for b in np.unique(idx[bad] // 16):
            s = slice(16 * b, 16 * b + 16)
            isp = pad[s] & bad[s]
            nm = name + '.pad' if isp.any() and not (bad[s] & ~pad[s]).any() else name
            rr = r[s][bad[s] & ~pad[s]]
            ratio = np.inf if isp.any() or np.isnan(rr).any() else rr.max() / kq[name]
            rep.findings.append(Finding(nm, int(b // 4), None, (int(b % 4), None), ratio))

    vec_check('z', state.vec[:N], q.z)
    if mode == MODE_EVAL:
        vec_check('alpha', state.vec[N:2 * N], q.alpha)
        guard_check('vec.untouched', state.vec[2 * N:4 * N].reshape(-1, 16))
    else:
        vec_check('v', state.vec[3 * N:4 * N], q.vstar)
        guard_check('vec.untouched', state.vec[N:3 * N].reshape(-1, 16))
    guard_check('vec.guard', state.vec[4 * N:].reshape(-1, 16))

    def part_check(name, got, want, scale, comps, where):
        """got / want / scale [rows x comps]; where(row) -> (i, j)"""
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.abs(np.asarray(got, dtype=LD) - want) / scale / LD(ref.err64[name])
        r = np.asarray(np.where((scale == 0) & (np.asarray(got, dtype=LD) == want), 0, r), dtype=np.float64)
        note(name, np.inf if np.isnan(r).any() else r.max())
        for x, k in np.argwhere(~(r <= kq[name])):
            i, j = where(int(x))
            rep.findings.append(Finding(name, i, j, (int(k), None),
                                        np.inf if np.isnan(r[x, k]) else r[x, k] / kq[name]))

    p = state.part
    part_check('logdet', p[part_logdet(T):part_logdet(T) + T].reshape(T, 1), q.logdet.reshape(T, 1),
               q.logdet_s.reshape(T, 1), 1, lambda x: (x, None))
    pr = p[part_pred(T):part_pred(T) + 3 * T].reshape(T, 3)
    if mode == MODE_EVAL:
        part_check('pred', pr[:, :1], q.pred[:, :1], q.pred_s[:, :1], 1, lambda x: (x, None))
        if (pr[:, 1:] != 0).any():   # v = 0 for a fitting cell
            rep.findings.append(Finding('pred', int(np.argwhere(pr[:, 1:] != 0)[0, 0]), None, (1, None), np.inf))
        itile = {tri(i) + j: (i, j) for i in range(T) for j in range(i + 1)}
        part_check('grad', p[:5 * nt].reshape(nt, 5), q.grad, q.grad_s, 5, lambda x: itile[x])
    else:
        part_check('pred', pr, q.pred, q.pred_s, 3, lambda x: (x, None))
        guard_check('part.untouched', p[:5 * nt].reshape(-1, 5))
    guard_check('part.untouched', p[5 * nt:5 * nt + T].reshape(-1, 1))
    guard_check('part.guard', p[part_size(T):].reshape(-1, 16))
    guard_check('out.guard', state.out[OUT_N:].reshape(-1, 16))
    return rep
