"""A plain `bench.py` run (no `--full`) and `--dump-outputs DIR`: the run times
exactly `--steps` steps, prints the headline line without the CPU baseline or
the parity check, and writes what its last timed step returned -- which must
be, bit for bit, what one blocking library call on that step's cells returns
(per-cell arithmetic never depends on the batch, tests/test_gpu_session.py)
-- plus the posterior fields of every timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, CELLS = 3, 24


@pytest.fixture(scope='module')
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('bench_outputs')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS),
                        '--warmup', '1', '--day-cells', str(CELLS), '--budget-s', '90',
                        '--dump-outputs', str(d / 'dump'), '--out', str(d / 'line.json')],
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line == json.loads((d / 'line.json').read_text())
    return line, d / 'dump'


@pytest.mark.gpu
def test_plain_line_is_the_headline_only(plain_run):
    line, _ = plain_run
    assert line['steps'] == STEPS and not line.get('truncated')
    assert line['unit'] == 'grid-cells/s' and line['higher_is_better'] is True and line['dtype'] == 'f64'
    assert line['value'] > 0 and line['failed_cells'] == 0 and line['config']['cells_total'] == CELLS
    # ms_per_step is the timed region over the timed steps, value the cells over the same region
    assert line['ms_per_step'] == pytest.approx(line['timed_s'] * 1e3 / STEPS, rel=1e-3, abs=0.2)
    assert line['value'] == pytest.approx(CELLS / line['timed_s'], rel=2e-3)
    # what takes runs of its own is behind --full
    assert line['cpu_baseline'] is None and 'parity' not in line
    assert line['roofline']['kernel']  # day: per-launch events are inside the timed region


@pytest.mark.gpu
def test_dump_outputs_are_the_last_steps_results(plain_run):
    import argparse
    import bench
    from optimalinterpolation_amd import _lib
    _, dump = plain_run
    got = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    assert set(got) == {'out', 'status', 'info', 'fields'}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_OUTPUTS_MAX_BYTES
    # the same slices bench.py times: the day's first CELLS cells in STEPS equal-cost runs
    args = argparse.Namespace(workload='day', steps=STEPS, warmup=0, seed=0, day_cells=CELLS, slices='ordered',
                              day_shares=0, share=-1)
    slices = bench.build_slices(args, 0, 1)[0]
    assert len(slices) == STEPS and got['fields'].shape == (CELLS, 8)
    last = slices[-1]
    out, st, info = _lib.gpr_batch(last.xyt, last.z, last.offs, last.xs, last.mean, x0=bench.X0, opt=True, info=True)
    assert np.all(st == 0) and np.isfinite(out).all()
    assert np.array_equal(got['out'], out)
    assert np.array_equal(got['status'], st.astype(float))
    assert np.array_equal(got['info'], info.astype(float))
    assert np.array_equal(got['fields'][-last.ncell:], out)


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_OUTPUTS_MAX_BYTES', 4096)
    big = np.arange(3000, dtype=np.float64).reshape(60, 50)
    arrays = {'a': big, 'b': np.arange(500, dtype=np.int32), 'c': np.ones(7, dtype=np.float32), 'none': None}
    bench.dump_outputs(str(tmp_path / 'x'), arrays)
    bench.dump_outputs(str(tmp_path / 'y'), arrays)
    x = {f: np.load(tmp_path / 'x' / f) for f in sorted(os.listdir(tmp_path / 'x'))}
    assert set(x) == {'a.npy', 'b.npy', 'c.npy'}
    assert sum(a.nbytes for a in x.values()) <= 4096
    assert x['a.npy'].dtype == np.float64 and x['b.npy'].dtype == np.float64 and x['c.npy'].dtype == np.float32
    assert np.all(np.isin(x['a.npy'], big)) and np.all(np.diff(x['a.npy']) > 0)  # a sorted sample of the array
    for f, a in x.items():
        assert np.array_equal(a, np.load(tmp_path / 'y' / f))


def test_dump_outputs_holds_finite_numbers_only(tmp_path):
    import bench
    a = np.arange(24, dtype=np.float64).reshape(3, 8)
    a[1, :3], a[1, 3:] = np.nan, np.inf  # a cell whose fit ran off to non-finite hypers
    bench.dump_outputs(str(tmp_path), {'out': a, 'status': np.zeros(3, dtype=np.int32)})
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert set(got) == {'out', 'out_nonfinite', 'status'}
    assert all(np.isfinite(v).all() and v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got['out_nonfinite'], np.arange(8, 16))
    assert np.array_equal(got['out'], np.r_[a[0], a[2]])
