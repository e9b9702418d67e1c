"""The dense-GP kernels driven directly through their exported launchers
(oi_device.h) and checked tile by tile against the longdouble reference of
tests/dense_ref.py, at exact site counts: every 16-row mask edge of the last
block row (rT next to 16, 32, 48, 64) at T = 1, 2, 5, the ends at T = 3 .. 8,
one T = 13 cell; k_panel_even and k_panel4, fused look-ahead and separate
diagonal launches, fitting / predicting / mixed rounds.  DESIGN §2 "Per-tile
tests" has the shapes, the tolerance rule and the measured ratios."""
import fractions

import numpy as np
import pytest

import dense_ref as R
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib

pytestmark = pytest.mark.gpu

HYP = (2e5, 2.5e5, 7.0, 4e-3, 1e-3)          # long length scales: no tile product negligible
HYP_ANISO = (9e4, 3e5, 3.0, 1e-2, 2e-3)
RT_ALL = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
RT_ENDS = (1, 16, 17, 64)
GRID = ([(T, rT) for T in (1, 2, 5) for rT in RT_ALL] + [(T, rT) for T in (3, 4, 6, 7, 8) for rT in RT_ENDS]
        + [(13, 17)])
PANELS, FUSES, MODES = ('even', '4'), (True, False), ('eval', 'predict', 'mixed')
RTOL = 1e-10                                  # T1 (tests/test_gpu_parity.py)


def grid_cells():
    """(Cell, hyper name) of the grid: every shape at HYP, the T = 2, 5 shapes at HYP_ANISO too."""
    out = []
    for q, (T, rT) in enumerate(GRID):
        rc = R.shape_cell(T, rT, seed=100 + q)
        out.append((R.Cell(rc, HYP), 'iso', rc))
        if T in (2, 5):
            out.append((R.Cell(rc, HYP_ANISO), 'aniso', rc))
    return out


@pytest.fixture(scope='module')
def grid():
    """The cells and their longdouble references, computed once for the module."""
    cells = grid_cells()
    return [(c, R.Ref(c), name, rc) for c, name, rc in cells]


def mode_of(modes, k):
    return {'eval': R.MODE_EVAL, 'predict': R.MODE_PREDICT}.get(modes, R.MODE_EVAL if k % 2 == 0 else R.MODE_PREDICT)


_runs = {}


def run_config(grid, panel, fuse, modes):
    """One ragged round of the whole grid in a configuration: [(State, Report)], cached."""
    key = (panel, fuse, modes)
    if key not in _runs:
        dcs = [R.DevCell(c.with_(mode=mode_of(modes, k))) for k, (c, _, _, _) in enumerate(grid)]
        R.run_round(dcs, panel=panel, fuse=fuse)
        out = []
        for d, (c, ref, _, _) in zip(dcs, grid):
            st = d.fetch()
            rep = R.compare(st, ref)
            st.w_null, st.L, st.W, st.Dinv = st.W is None, None, None, None   # keep the small arrays only
            out.append((st, rep))
        _runs[key] = out
    return _runs[key]


def worst_ratios(results):
    w = {}
    for _, rep in results:
        for q, r in rep.ratios.items():
            w[q] = max(w.get(q, 0.0), r)
    return w


# ------------------------------------------------------------ (a) and (c) --
@pytest.mark.parametrize('modes', MODES)
@pytest.mark.parametrize('fuse', FUSES, ids=['fused', 'separate'])
@pytest.mark.parametrize('panel', PANELS)
def test_factor_state_tile_by_tile(grid, panel, fuse, modes):
    """After the round: every lower tile of L and W, every Dinv, z, alpha, v,
    the logdet and pred partials within K_Q err64 of the reference; padding
    exactly identity / zero, upper triangles of diagonal tiles exactly zero,
    guards and unwritten slots bit-intact, no NaN where a value belongs, W
    null in predict mode; k_finalize's row at T1 of the reference's."""
    results = run_config(grid, panel, fuse, modes)
    print('worst err / err64:', {q: round(r, 3) for q, r in worst_ratios(results).items()})
    bad = []
    for k, ((c, ref, name, _), (st, rep)) in enumerate(zip(grid, results)):
        assert st.status == 0 and st.out[R.OUT_STATUS] == 0.0, (c.T, c.rT, name)
        assert st.w_null == (st.mode == R.MODE_PREDICT)
        if rep.findings:
            bad.append(((c.T, c.rT, name), rep))
        if st.mode == R.MODE_EVAL:
            nlz, g = ref.out_eval()
            # T1 scales: |g_j| + 1/2 sum |Q o dK_j|, and sn2 sum |diag Q| for the noise term
            gs = np.asarray(ref.q.grad_s.sum(0), float)
            S = np.abs(np.asarray(g[:5], float)) + np.array([gs[0] / 2, gs[1] / 2, gs[2] / 2, gs[3] / 2, c.hyp[4] * gs[4]])
            assert abs(st.out[0] - float(nlz)) <= RTOL * max(1.0, abs(float(nlz))), (c.T, c.rT, name)
            assert np.all(np.abs(st.out[1:6] - np.asarray(g[:5], float)) <= RTOL * S), (c.T, c.rT, name)
            assert st.out[6] == 0.0
        else:
            for got, want in zip(st.out[:3], ref.out_predict()):
                assert abs(got - float(want)) <= RTOL * max(1.0, abs(float(want))), (c.T, c.rT, name)
    assert not bad, bad[:4]


@pytest.mark.parametrize('panel', PANELS)
def test_lauum_grad_partials(grid, panel):
    """k_lauum_grad1: all T (T + 1) / 2 x 5 partials of every fitting cell,
    each against the reference on the scale of its own sum of absolute terms."""
    results = run_config(grid, panel, True, 'eval')
    n = 0
    for (c, ref, name, _), (st, rep) in zip(grid, results):
        nt = R.tri(c.T)
        got = st.part[:5 * nt].reshape(nt, 5)
        assert np.isfinite(got).all(), (c.T, c.rT, name)
        assert [f for f in rep.findings if f.quantity == 'grad'] == [], (c.T, c.rT, name, rep)
        # the trace partial exists on diagonal tiles only
        off = [R.tri(i) + j for i in range(c.T) for j in range(i)]
        assert (got[off, 4] == 0).all()
        n += got.size
    assert n == sum(5 * R.tri(c.T) for c, _, _, _ in grid)
    assert 'grad' in worst_ratios(results)


# -------------------------------------------------------------------- (b) --
@pytest.mark.parametrize('fuse', FUSES, ids=['fused', 'separate'])
@pytest.mark.parametrize('panel', PANELS)
def test_columns_final_launch_by_launch(panel, fuse):
    """Stopping the replay after column j (T = 7, rT = 17): columns <= j of L,
    rows <= j of W, Dinv and z up to block j already hold the bits of the full
    run -- for even j after the even panel alone, for odd j once
    k_chol_panel(j) has run.  A failure names the launch."""
    T = 7
    cell = R.Cell(R.shape_cell(T, 17, seed=77), HYP)
    full = R.DevCell(cell)
    R.run_round([full], panel=panel, fuse=fuse)
    F = full.fetch()
    assert F.status == 0
    bits = lambda a: np.asarray(a).view(np.uint64)
    for j in range(T):
        d = R.DevCell(cell)
        log = R.run_round([d], panel=panel, fuse=fuse, upto=j)
        S = d.fetch()
        where = f"after {log[-1][0]}(j={j}) [{panel}, fuse={fuse}]"
        for c in range(j + 1):
            for i in range(c, T):
                assert np.array_equal(bits(S.L[R.tri(i) + c]), bits(F.L[R.tri(i) + c])), f"L({i},{c}) {where}"
            for r in range(c, j + 1):
                assert np.array_equal(bits(S.W[R.tri(r) + c]), bits(F.W[R.tri(r) + c])), f"W({r},{c}) {where}"
            assert np.array_equal(bits(S.Dinv[c]), bits(F.Dinv[c])), f"Dinv({c}) {where}"
            assert np.array_equal(bits(S.vec[64 * c:64 * c + 64]), bits(F.vec[64 * c:64 * c + 64])), f"z({c}) {where}"
        # nothing of the rows below W row j + 1 is written yet
        for r in range(j + 2, T):
            for c in range(r + 1):
                assert R._sent(S.W[R.tri(r) + c]).all(), f"W({r},{c}) written {where}"
        assert R._sent(S.out).all()


# -------------------------------------------------------------------- (d) --
@pytest.mark.parametrize('panel', PANELS)
def test_replay_equals_the_engine_bitwise(grid, panel, monkeypatch):
    """The harness's result rows are bitwise the product's (nlml_grad_batch,
    gpr_batch(opt=False)) on the same duplicate-free cells -- k_panel_even as
    the engine picks it by default for rounds this small, k_panel4 under
    OI_PANEL4_MINT=0 + OI_PANEL4_MINWG=0 -- so the replay is the product's
    launch sequence."""
    if panel == '4':
        monkeypatch.setenv('OI_PANEL4_MINT', '0')
        monkeypatch.setenv('OI_PANEL4_MINWG', '0')
    rcs = [rc for c, _, name, rc in grid if name == 'iso']
    batch = R.concat_cells(rcs)
    h = np.tile(np.concatenate([np.log(HYP), [0.0]]), (len(rcs), 1))
    hyp = R.hyp_of_h(h[0])
    nlz, grad, st = _lib.nlml_grad_batch(batch.xyt, batch.z, np.full(len(batch.z), batch.mean), batch.offs, h)
    out, st2, _ = _lib.gpr_batch(batch.xyt, batch.z, batch.offs, batch.xs, batch.mean, opt=False,
                                 hyp=np.tile(hyp, (len(rcs), 1)))
    assert (st == 0).all() and (st2 == 0).all()
    for mode in (R.MODE_EVAL, R.MODE_PREDICT):
        dcs = [R.DevCell(R.Cell(rc, hyp, mode)) for rc in rcs]
        assert all(d.cell.m == d.cell.n_obs for d in dcs)
        R.run_round(dcs, panel=panel, fuse=True)
        for k, d in enumerate(dcs):
            s = d.fetch()
            if mode == R.MODE_EVAL:
                assert s.out[0] == nlz[k] and np.array_equal(s.out[1:7], grad[k]), (GRID[k], s.out, nlz[k], grad[k])
            else:
                assert np.array_equal(s.out[:3], out[k, :3]), (GRID[k], s.out, out[k])


# -------------------------------------------------------------------- (e) --
DEAL_SHAPES = [(5, 17), (1, 1), (13, 17), (2, 64), (7, 16), (3, 1), (8, 17), (1, 64), (4, 16), (2, 1), (6, 64),
               (5, 63), (3, 17), (2, 33), (1, 31), (7, 1), (4, 64)]


@pytest.mark.parametrize('panel', PANELS)
def test_cell_to_workgroup_dealing(panel):
    """xcd_cell_slot / xcd_cell_slot_lead0 and the grid padded to 8 cells:
    rounds of 1, 7, 8, 9 and 17 cells of mixed T (cells with T <= j dropping
    out of the later launches, fitting and predicting cells mixed) leave every
    cell's whole state bitwise as that cell run alone."""
    cells = [R.Cell(R.shape_cell(T, rT, seed=300 + k), HYP, R.MODE_EVAL if k % 3 else R.MODE_PREDICT)
             for k, (T, rT) in enumerate(DEAL_SHAPES)]
    alone = []
    for c in cells:
        d = R.DevCell(c)
        R.run_round([d], panel=panel, fuse=True)
        alone.append(d.fetch())
        assert alone[-1].status == 0 and not R._sent(alone[-1].out[:3]).any()
    for n in (1, 7, 8, 9, 17):
        dcs = [R.DevCell(c) for c in cells[:n]]
        R.run_round(dcs, panel=panel, fuse=True)
        for k, d in enumerate(dcs):
            assert d.fetch().same_bits(alone[k]), (n, k, DEAL_SHAPES[k])


# -------------------------------------------------------------------- (f) --
@pytest.mark.parametrize('panel', PANELS)
def test_failed_cell_leaves_its_workspace_and_mates_alone(panel):
    """A cell with repeated sites and sn2 / sf2 below OI_DUP_NONPD_TAU n_obs is
    flagged not-PD by k_diag_factor4w(0): no later launch writes its workspace,
    its row is inf (fitting) / NaN (predicting), its round-mates' states are
    bitwise those of a round without it."""
    sf2 = 4e-3
    hyp_bad = (2e5, 2.5e5, 7.0, sf2, sf2 * 1e-3 * R.DUP_NONPD_TAU)
    mk = lambda T, rT, extra, hyp, mode, s: R.Cell(R.shape_cell(T, rT, extra=extra, seed=s), hyp, mode)
    good = [mk(3, 17, 0, HYP, R.MODE_EVAL, 1), mk(1, 33, 9, HYP, R.MODE_PREDICT, 2), mk(2, 1, 0, HYP, R.MODE_EVAL, 3)]
    bad = [mk(5, 16, 5, hyp_bad, R.MODE_EVAL, 4), mk(2, 48, 5, hyp_bad, R.MODE_PREDICT, 5)]
    for c in bad:
        assert c.n_obs > c.m and c.hyp[4] < R.DUP_NONPD_TAU * c.n_obs * c.hyp[3]
    ref = [R.DevCell(c) for c in good]
    R.run_round(ref, panel=panel, fuse=True)
    order = [bad[0], good[0], good[1], bad[1], good[2]]
    dcs = [R.DevCell(c) for c in order]
    R.run_round(dcs, panel=panel, fuse=True)
    st = [d.fetch() for d in dcs]
    for k, g in ((1, 0), (2, 1), (4, 2)):
        assert st[k].status == 0 and st[k].same_bits(ref[g].fetch()), k
    for k in (0, 3):
        assert st[k].status == 1 and st[k].poisoned(), k
        assert st[k].out[R.OUT_STATUS] == 1.0 and R._sent(st[k].out[R.OUT_N:]).all()
    assert np.all(st[0].out[:7] == np.inf)
    assert np.isnan(st[3].out[:3]).all() and not R._sent(st[3].out[:3]).any() and R._sent(st[3].out[3:7]).all()


# -------------------------------------------------------------------- (g) --
def _fma(a, b, c):
    F = fractions.Fraction
    return float(F(a) * F(b) + F(c))


def ssw_restated(r, sid, fo, fused):
    """k_dedup's SSW in its own order: thread t owns observations
    [t seg, (t + 1) seg), sums (r - site mean)^2 over the sites first seen
    there, each site's observations in order; 64-lane shuffle trees, then
    ((w0 + w1) + w2) + w3.  fused: part = fma(e, e, part)."""
    n = len(r)
    seg = (n + 255) // 256
    members = {}
    for a in range(n):
        members.setdefault(int(sid[a]), []).append(a)
    part = np.zeros(256)
    for t in range(256):
        p = 0.0
        for a in range(min(n, t * seg), min(n, t * seg + seg)):
            s = int(sid[a])
            if fo[s] != a:
                continue
            rs, cnt = 0.0, 0.0
            for b in members[s]:
                rs += r[b]
                cnt += 1.0
            rbar = rs / cnt
            for b in members[s]:
                e = r[b] - rbar
                p = _fma(e, e, p) if fused else p + e * e
        part[t] = p
    red = []
    for w in range(4):
        x = part[64 * w:64 * w + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            x[:o] = x[:o] + x[o:2 * o]
        red.append(x[0])
    return ((red[0] + red[1]) + red[2]) + red[3]


DEDUP_PATTERNS = {'none': lambda a, n: a, 'one': lambda a, n: 0 * a, 'runs': lambda a, n: a // 100,
                  'stride': lambda a, n: a % 256}


def _dedup_case(n, pattern, rng):
    sid = DEDUP_PATTERNS[pattern](np.arange(n), n)
    sites = np.stack([3e6 + 25e3 * rng.permutation(n), 2e6 + 25e3 * rng.permutation(n),
                      rng.integers(0, 9, n).astype(float)], axis=1)
    return sites[sid], rng.normal(0.0, 0.05, n)


@pytest.mark.parametrize('sizes', [(1, 2, 255, 256, 257), (4096, 4097, 2, 257), (13000, 13001, 1)],
                         ids=['small', 'lds_limit', 'max_n'])
@pytest.mark.parametrize('pattern', list(DEDUP_PATTERNS) + ['nodup'])
def test_dedup_kernel(sizes, pattern):
    """k_dedup through oi_launch_dedup against its numpy restatement: sites in
    first-occurrence order, counts, m exact; v = sum / sqrt(c) bitwise (sums in
    observation order); SSW bitwise in the kernel's own summation order (with
    the square either fused into the sum or not); nothing written past a
    cell's m sites.  Sizes cross the LDS staging limit (4096) and DEDUP_MAX_N
    (13000: beyond it, and with nodup, every observation is its own site)."""
    import torch
    rng = np.random.default_rng([len(sizes), sizes[0], list(DEDUP_PATTERNS).index(pattern) if pattern != 'nodup' else 9])
    nodup = pattern == 'nodup'
    parts = [_dedup_case(n, 'runs' if nodup else pattern, rng) for n in sizes]
    xyt = np.concatenate([p[0] for p in parts])
    r = np.concatenate([p[1] for p in parts])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, nc, G = int(offs[-1]), len(sizes), 64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_x, d_r, d_o = dev(xyt), dev(r), dev(offs)
    d_s, d_v, d_d, d_w = R._poison(3 * N + G), R._poison(N + G), R._poison(N + G), R._poison(nc + G)
    d_m = torch.full((nc + G,), -7, dtype=torch.int32, device='cuda')
    rc = R.lib().oi_launch_dedup(d_x.data_ptr(), d_r.data_ptr(), d_o.data_ptr(), nc, max(sizes), int(nodup),
                                 d_s.data_ptr(), d_v.data_ptr(), d_d.data_ptr(), d_m.data_ptr(), d_w.data_ptr(),
                                 R._stream())
    torch.cuda.synchronize()
    assert rc == 0
    s, v, d, w, mc = (t.cpu().numpy() for t in (d_s, d_v, d_d, d_w, d_m))
    assert R._sent(s[3 * N:]).all() and R._sent(v[N:]).all() and R._sent(d[N:]).all() and R._sent(w[nc:]).all()
    assert (mc[nc:] == -7).all()
    for c, n in enumerate(sizes):
        a0 = int(offs[c])
        x, rr = xyt[a0:a0 + n], r[a0:a0 + n]
        if nodup or n > 13000:
            es, ev, ed, sid, fo = x, rr, np.ones(n), np.arange(n), np.arange(n)
            essw = (0.0,)
        else:
            es, ev, ed, _, _, sid, fo = R.dedup_np(x, rr)
            essw = (ssw_restated(rr, sid, fo, True), ssw_restated(rr, sid, fo, False))
        m = len(ev)
        assert mc[c] == m, (n, pattern)
        assert np.array_equal(s[3 * a0:3 * (a0 + m)].reshape(m, 3), es), (n, pattern)
        assert np.array_equal(d[a0:a0 + m], ed) and np.array_equal(v[a0:a0 + m], ev), (n, pattern)
        assert R._sent(s[3 * (a0 + m):3 * (a0 + n)]).all() and R._sent(v[a0 + m:a0 + n]).all() \
            and R._sent(d[a0 + m:a0 + n]).all(), (n, pattern)
        assert w[c] in essw, (n, pattern, w[c], essw)


# -------------------------------------------------------------------- (h) --
def test_abi_at_exact_edges_with_duplicates():
    """The default path (k_dedup, engine, k_finalize's (n - m) and SSW terms)
    on cells whose SITE count sits on a tile edge, n_obs = m + 37, against the
    oracle's n x n neg_log_ml and predict at T1."""
    close, grad_scale = R.t1_close, R.grad_scale
    shapes = [(1, 1), (1, 63), (1, 64), (2, 1), (2, 16), (2, 17), (3, 64), (4, 1), (5, 48), (6, 49), (8, 64)]
    cells = R.concat_cells([R.shape_cell(T, rT, extra=37, seed=500 + k) for k, (T, rT) in enumerate(shapes)])
    assert [(m, T, rT) for _, m, T, rT in R.site_counts(cells)] == [(64 * (T - 1) + rT, T, rT) for T, rT in shapes]
    nc = len(shapes)
    h = np.tile(np.concatenate([np.log(HYP), [0.0]]), (nc, 1))
    h[1::2] = np.concatenate([np.log(HYP_ANISO), [0.0]])
    mX = np.full(len(cells.z), cells.mean)
    nlz, grad, st = _lib.nlml_grad_batch(cells.xyt, cells.z, mX, cells.offs, h)
    hyp = np.exp(h[:, :5])
    out, st2, _ = _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False, hyp=hyp)
    assert (st == 0).all() and (st2 == 0).all()
    for c in range(nc):
        x, y, xs = cells.cell(c)
        mx = np.full(len(y), cells.mean)
        f, g = O.neg_log_ml(h[c], x, y, mx)
        f = float(np.asarray(f).item())
        ok, err = close(nlz[c], f)
        assert ok, (shapes[c], nlz[c], f, err)
        sc = np.abs(g) + grad_scale(h[c], x, y, mx)
        ok, err = close(grad[c], g, scale=np.maximum(sc, 1e-300))
        assert ok, (shapes[c], grad[c], g, err)
        fs, sd, lZ = O.predict(x, y, xs, cells.mean, hyp[c, :3], hyp[c, 3], hyp[c, 4])
        ok, err = close(out[c, :3], [fs[0], sd[0], lZ])
        assert ok, (shapes[c], out[c, :3], (fs[0], sd[0], lZ), err)
