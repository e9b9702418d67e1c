"""The engine's device arena without a GPU.

* The first-fit free list (csrc/oi_arena.h) is built on its own with g++
  -fsanitize=address,undefined (`make -C optimalinterpolation_amd arena_check`)
  under tests/host/arena_check.cpp: seeded random alloc / release sequences
  against a granule bitmap, and the literal sequences of the defects found in
  it (a zero-byte block that lost its neighbour's bytes).  No ASan / UBSan
  report, exit code 0.
* The sizes admission works with -- a resident cell's block, a batch's input
  block -- come from the library's hooks and must equal the closed forms of
  tests/engine_ref.py to the byte: the pools of
  tests/test_gpu_engine_admission.py are computed from them."""
import os
import re
import shutil
import subprocess

import pytest

import engine_ref as E
from conftest import ROOT
from optimalinterpolation_amd import _lib

PKG = os.path.join(ROOT, 'optimalinterpolation_amd')
SIZES = [0, 1, 63, 64, 65, 128, 130, 333, 4097]


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_free_list_under_asan_ubsan():
    subprocess.run(['make', '-C', PKG, 'arena_check'], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(PKG, 'build', 'arena_check_san')], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and re.search(r'^OK \d+ cases', r.stdout, re.M), (r.stdout[-2000:], r.stderr[-3000:])
    assert 'FAIL' not in r.stdout
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def test_hooks_are_exported_and_not_in_oi_h():
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in ('oi_test_engine_cell_bytes', 'oi_test_engine_input_bytes', 'oi_test_engine_arena'):
        assert re.search(rf'\b[TW] {name}\b', out), name
        assert name not in _lib.SIGNATURES
        assert name not in open(os.path.join(ROOT, 'include', 'oi.h')).read()


@pytest.mark.parametrize('eval_mem', [False, True])
def test_cell_bytes_is_the_closed_form(eval_mem):
    for n in SIZES:
        assert E.cell_bytes(n, eval_mem) == E.cell_bytes_form(n, eval_mem), n
        assert E.cell_bytes(n, eval_mem) % E.GRANULE == 0
    assert E.cell_bytes(0, eval_mem) == 0                 # an empty cell owns no memory
    # one tile: L (| W) and Dinv 32 KiB each, 4 vectors of 64, 10 partial sums rounded to a granule
    assert E.cell_bytes(1, eval_mem) == (3 if eval_mem else 2) * 32768 + 2048 + 256


@pytest.mark.parametrize('host', [False, True])
def test_input_bytes_is_the_closed_form(host):
    for N in SIZES:
        for ncell in (0, 1, 2, 12, 63, 64, 65):
            assert E.input_bytes(N, ncell, host) == E.input_bytes_form(N, ncell, host), (N, ncell)
    # eight (seven with device inputs) pieces, none empty
    assert E.input_bytes(0, 0, host) == (8 if host else 7) * E.GRANULE
    assert E.input_bytes(32, 1, host) == (256 + 768 + 256 + 256 + 3 * 256) + (768 if host else 0)
