"""Admission in the continuous-batching engine (csrc/oi_engine.cpp): slots,
stream groups and the device arena under small pools.

Cells wait in a FIFO queue; admit() gives each a slot (``max_pool`` of them,
split over ``OI_GROUPS`` stream groups) and a first-fit block of the arena
(``pool_bytes``); a finished cell hands both to the next.  A cell's arithmetic
never depends on its round mates, so every case here -- few slots, a slot and a
block reused by cells of other sizes, uneven groups, cells waiting for memory,
a pool that holds exactly the largest cell, batches whose input blocks fragment
the arena -- must give the outputs, status words and CG info of ONE
unconstrained call bit for bit.  That reference is computed once per kind
(fit, predict at fixed hypers, objective + gradient) and its predict rows are
anchored to the oracle (GPR:173-182) within 1e-10 * max(1, |ref|), the bound
of tests/test_gpu_config2.py.

Every pool is computed from tests/engine_ref.py (sizes from the library's
hooks, equal to the closed forms there by tests/test_arena.py); the problem
size of a cell is its number of DISTINCT sites, counted here with np.unique.
After every test the device's arena must be wholly free, in one block.  Every
refusal in this file is made by the host before any launch."""
import numpy as np
import pytest

import engine_ref as E
from oracle import gp_oracle as O
from optimalinterpolation_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

X0 = np.array(O.X0_PRODUCTION)
H_EVAL = np.array([np.log(2e5), np.log(2e5), np.log(6.), np.log(5e-3), np.log(1e-3), 0.0])
# tile edges (64), one to six tiles, two empty cells; the generator's duplicate
# sites stay in, so the cells' sizes m are counted below
SIZES = [0, 1, 63, 64, 65, 130, 200, 257, 333, 0, 90, 17, 300, 185]
CELLS = synthetic.make_cells(SIZES, seed=25)
NCELL = CELLS.ncell
M = np.array([len(np.unique(CELLS.cell(c)[0], axis=0)) for c in range(NCELL)])
M_MAX = int(M.max())
N_OBS = int(CELLS.offs[-1])
HYP = np.tile(synthetic.FIXED_HYPERS, (NCELL, 1))
KINDS = ['fit', 'pred', 'eval']
EVAL_MEM = {'fit': True, 'pred': False, 'eval': True}   # whether the kind's cells hold W


def test_cells_cover_the_tile_counts():
    T = (M + 63) // 64
    assert sorted(set(T)) == [0, 1, 2, 3, 4, 5, 6]
    assert {63, 64, 65} <= set(M) and (M == 0).sum() == 2
    assert M_MAX % 64 == 1            # the largest cell's last tile holds one row
    assert (M < np.array(SIZES)).any()  # some sites repeat


def _run(kind, cells=CELLS, idx=None, **kw):
    """One call of `kind` over cells[idx]: a tuple of arrays, one row per cell."""
    if idx is not None:
        cells = cells.subset(idx)
    n = cells.ncell
    if kind == 'fit':
        return _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, x0=X0, opt=True, info=True, **kw)
    if kind == 'pred':
        return _lib.gpr_batch(cells.xyt, cells.z, cells.offs, cells.xs, cells.mean, opt=False,
                              hyp=np.tile(synthetic.FIXED_HYPERS, (n, 1)), info=True, **kw)
    return _lib.nlml_grad_batch(cells.xyt, cells.z, np.full(len(cells.z), cells.mean), cells.offs,
                                np.tile(H_EVAL, (n, 1)), **kw)


def _assert_same(got, ref, idx=None, what=''):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        b = b if idx is None else b[np.asarray(idx)]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), (what, k, a, b)


def _totals():
    p = _lib.profile_json()
    return p['evals'], p['predicts']


@pytest.fixture(scope='module')
def ref():
    """The unconstrained call of each kind (default pool, every cell resident at
    once) with its totals of objective evaluations and predictions."""
    r = {}
    for kind in KINDS:
        _lib.profile_reset()
        out = _run(kind)
        for a in out:
            a.setflags(write=False)
        r[kind] = out
        r[kind + '_totals'] = _totals()
    return r


@pytest.fixture(autouse=True)
def _arena_wholly_free(ref):
    yield
    st = E.arena_state(0)
    assert st is not None
    size, free, largest = st
    assert free == size and largest == size, st


def test_reference_against_the_oracle(ref):
    out, status, _ = ref['pred']
    lx, ly, lt, sf2, sn2 = synthetic.FIXED_HYPERS
    assert np.all(status == 0)
    for c in range(NCELL):
        x, y, xs = CELLS.cell(c)
        if len(y) == 0:   # no observation: the prior
            assert out[c, 0] == CELLS.mean and out[c, 1] == np.sqrt(sf2) and out[c, 2] == 0.0
            continue
        fs, sd, lz = O.predict(x, y, xs, CELLS.mean, (lx, ly, lt), sf2, sn2)
        want = np.array([fs[0], sd[0], lz])
        err = np.abs(out[c, :3] - want) / np.maximum(1.0, np.abs(want))
        assert np.all(err <= 1e-10), (c, out[c, :3], want, err)
        assert np.array_equal(out[c, 3:], synthetic.FIXED_HYPERS)
    fit, fst, info = ref['fit']
    big = M >= 63
    assert np.all(fst[big] == 0) and np.all(np.isfinite(fit[big])) and np.all(info[big, 3] > 1)
    nlz, grad, est = ref['eval']
    assert np.all(est == 0) and np.all(np.isfinite(nlz)) and np.all(np.isfinite(grad))


# --------------------------------------------------------------- slots
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('max_pool', [1, 2, 3, 5, NCELL - 1, NCELL])
def test_max_pool(ref, kind, max_pool):
    _lib.profile_reset()
    got = _run(kind, max_pool=max_pool, profile=True)
    p = _lib.profile_json()
    _assert_same(got, ref[kind], what=(kind, max_pool))
    rows = p['rounds_log']
    assert rows and all(r[0] + r[1] <= max_pool for r in rows), rows
    assert max(r[0] + r[1] for r in rows) == max_pool     # the slots are all used
    assert (p['evals'], p['predicts']) == ref[kind + '_totals']


def _session(kind, batches, wait_order, **kw):
    """Submits cells[idx] for every idx of `batches`, all before the first wait,
    waits in `wait_order`, and returns the rows in cell order of `batches`."""
    res = {}
    with _lib.Session(**kw) as s:
        t = []
        for idx in batches:
            b = CELLS.subset(idx)
            if kind == 'fit':
                t.append(s.submit(b.xyt, b.z, b.offs, b.xs, b.mean, x0=X0))
            else:
                t.append(s.submit(b.xyt, b.z, b.offs, b.xs, b.mean, opt=False, hyp=HYP[:b.ncell]))
        for k in wait_order:
            res[k] = s.wait(t[k])
    return tuple(np.concatenate([res[k][j] for k in range(len(batches))]) for j in range(3))


@pytest.mark.parametrize('poison', [False, True])
@pytest.mark.parametrize('kind', ['fit', 'pred'])
def test_one_slot_reused_across_sizes(ref, kind, poison, monkeypatch):
    """One slot, one cell resident at a time: the slot and its arena block serve
    a smaller and a larger cell in turn, with the last cell's (finite) tiles
    still in the block -- or NaNs under OI_POISON=1."""
    if poison:
        monkeypatch.setenv('OI_POISON', '1')
    order = [SIZES.index(n) for n in (333, 65, 257, 64, 130, 0, 200, 1)]
    got = _session(kind, [[c] for c in order], range(len(order)), max_pool=1)
    _assert_same(got, ref[kind], idx=order, what=(kind, poison))


# --------------------------------------------------------------- stream groups
def _group_shape(groups, cap):
    G = 1 if cap < 2 * groups else groups
    return G, (cap + G - 1) // G


@pytest.mark.parametrize('profile', [False, True])
@pytest.mark.parametrize('kind', ['fit', 'pred'])
@pytest.mark.parametrize('groups, max_pool', [(2, 3), (2, 4), (2, 5), (3, 7), (8, NCELL)])
def test_groups(ref, groups, max_pool, kind, profile, monkeypatch):
    """One group by the cap < 2 * groups rule (2, 3) and (8, ncell), an even
    split (2, 4), an uneven one (2, 5) -> 3 + 2, a group of one slot (3, 7) ->
    3 + 3 + 1.  Unprofiled rounds complete through the host flag, profiled ones
    by a stream synchronise."""
    monkeypatch.setenv('OI_GROUPS', str(groups))
    G, capG = _group_shape(groups, min(max_pool, NCELL))
    assert (G, capG) == {(2, 3): (1, 3), (2, 4): (2, 2), (2, 5): (2, 3), (3, 7): (3, 3), (8, NCELL): (1, NCELL)}[
        (groups, max_pool)]
    _lib.profile_reset()
    got = _run(kind, max_pool=max_pool, profile=profile)
    p = _lib.profile_json()
    _assert_same(got, ref[kind], what=(groups, max_pool, kind, profile))
    assert (p['evals'], p['predicts']) == ref[kind + '_totals']
    if profile:   # a row is one group's round
        assert all(r[0] + r[1] <= capG for r in p['rounds_log']), p['rounds_log']


# --------------------------------------------------------------- memory
def _budget_cells(kind):
    return 2 * E.cell_bytes(M_MAX, EVAL_MEM[kind])


def _memory_bound_pool(kind):
    """The whole batch's inputs and twice the largest cell."""
    return E.input_bytes(N_OBS, NCELL, True) + _budget_cells(kind)


def _first_wave(kind, budget):
    """Cells admitted before the first round: largest first (ties by index),
    until the queue's head does not fit."""
    used = k = 0
    for c in sorted(range(NCELL), key=lambda c: -M[c]):
        b = E.cell_bytes(M[c], EVAL_MEM[kind])
        if used + b > budget:
            break
        used, k = used + b, k + 1
    return k


def _most_cells(kind, budget):
    """How many cells `budget` bytes can hold at most (the smallest ones)."""
    used = k = 0
    for b in sorted(E.cell_bytes(m, EVAL_MEM[kind]) for m in M):
        if used + b > budget:
            break
        used, k = used + b, k + 1
    return k


@pytest.mark.parametrize('kind', KINDS)
def test_memory_bound_admission(ref, kind):
    pool = _memory_bound_pool(kind)
    _lib.profile_reset()
    got = _run(kind, pool_bytes=pool, profile=True)
    p = _lib.profile_json()
    _assert_same(got, ref[kind], what=kind)
    rows = p['rounds_log']
    first = _first_wave(kind, _budget_cells(kind))
    assert 1 <= first < NCELL
    assert rows[0][0] + rows[0][1] == first and rows[0][2] == (M_MAX + 63) // 64, rows[0]
    # the other cells came in later waves, and never more than the pool holds
    most = _most_cells(kind, _budget_cells(kind))
    assert most < NCELL
    assert all(r[0] + r[1] <= most for r in rows), (most, rows)
    assert len(rows) > 1
    assert (p['evals'], p['predicts']) == ref[kind + '_totals']
    assert E.arena_state(0)[0] == pool


@pytest.mark.parametrize('kind', ['fit', 'eval', 'pred'])
def test_exact_pool(ref, kind):
    """A pool of exactly the largest cell passes the submit check, so the batch
    completes (its inputs leave the arena); one granule less is refused at
    submit, before any launch, and leaves the arena whole."""
    pool = E.cell_bytes(M_MAX, EVAL_MEM[kind])
    assert E.input_bytes(N_OBS, NCELL, True) < pool   # the inputs do go to the arena first
    got = _run(kind, pool_bytes=pool)
    _assert_same(got, ref[kind], what=kind)
    assert E.arena_state(0) == (pool, pool, pool)
    with pytest.raises(_lib.OiError, match=r'-3.*a cell needs'):
        _run(kind, pool_bytes=pool - E.GRANULE)
    small = pool - E.GRANULE
    assert E.arena_state(0) == (small, small, small)
    # an ordinary call next: a pool with room for the inputs and every cell at once
    roomy = E.input_bytes(N_OBS, NCELL, True) + sum(E.cell_bytes(m, EVAL_MEM[kind]) for m in M)
    _lib.profile_reset()
    _assert_same(_run(kind, pool_bytes=roomy, profile=True), ref[kind], what=(kind, 'after the refusal'))
    first = _lib.profile_json()['rounds_log'][0]
    assert first[0] + first[1] == NCELL


QUARTERS = [list(range(0, 4)), list(range(4, 8)), list(range(8, 11)), list(range(11, NCELL))]


@pytest.mark.parametrize('max_pool', [0, 2])
@pytest.mark.parametrize('kind', ['fit', 'pred'])
def test_session_under_pressure(ref, kind, max_pool):
    """Four batches queued before the first wait in a pool that holds two large
    cells, waited out of order."""
    got = _session(kind, QUARTERS, (3, 1, 0, 2), pool_bytes=_memory_bound_pool(kind), max_pool=max_pool)
    _assert_same(got, ref[kind], what=(kind, max_pool))


@pytest.mark.parametrize('kind', ['fit', 'pred'])
def test_session_fragmented_by_inputs(ref, kind):
    """Batches A and B queued, A waited first.  A's cells run behind both input
    blocks; when A leaves, the free arena is A's old input block and the gap
    behind B's inputs, and B's largest cell fits the pool but neither of them."""
    A = [SIZES.index(n) for n in (65, 17, 90)]
    B = [SIZES.index(n) for n in (333, 130, 1)]
    ev = EVAL_MEM[kind]
    pool = E.cell_bytes(M_MAX, ev)
    in_a = E.input_bytes(CELLS.sizes[A].sum(), len(A), True)
    in_b = E.input_bytes(CELLS.sizes[B].sum(), len(B), True)
    gap = pool - in_a - in_b
    assert sum(E.cell_bytes(M[c], ev) for c in A) <= gap      # A runs with both blocks in place
    assert in_a < E.cell_bytes(M_MAX, ev) and gap < E.cell_bytes(M_MAX, ev) <= pool
    got = _session(kind, [A, B], (0, 1), pool_bytes=pool)
    _assert_same(got, ref[kind], idx=A + B, what=kind)


@pytest.mark.parametrize('kind', ['fit', 'pred'])
def test_empty_cells_leak_nothing(ref, kind):
    """An n = 0 cell owns no memory: the cell admitted after it gets the same
    offset, the empty cell leaves first, and the neighbour's bytes must still
    come back.  Two batches queued before the first wait, the first one ending
    (in admission order) with the empty cells; explicit pool, so the arena
    outlives the session."""
    first = [SIZES.index(200), 0, 9, SIZES.index(17)]        # cells 0 and 9 are empty
    second = [SIZES.index(n) for n in (257, 64, 130)]
    assert M[0] == 0 and M[9] == 0
    pool = E.input_bytes(N_OBS, NCELL, True) + 4 * E.cell_bytes(M_MAX, EVAL_MEM[kind])
    got = _session(kind, [first, second], (0, 1), pool_bytes=pool)
    _assert_same(got, ref[kind], idx=first + second, what=kind)
    assert E.arena_state(0) == (pool, pool, pool)
    # and the pool still holds what it held at first: the same session again
    got = _session(kind, [first, second], (1, 0), pool_bytes=pool)
    _assert_same(got, ref[kind], idx=first + second, what=(kind, 'again'))
    assert E.arena_state(0) == (pool, pool, pool)
