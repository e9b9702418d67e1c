"""Each staged path sizes its workspace by running the layout function that
carves it on a counting Carver.  The counts must stay what the hand-written
formulas gave (tests/workspace_ref.py keeps those as the specification): the
chunk planner's cuts, and with them every ``pool_bytes`` case of the GPU tests,
depend on them to the double.  Exact comparisons, no GPU."""
import itertools
import re
import subprocess

import pytest

import workspace_ref as W
from optimalinterpolation_amd import _lib

SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 128, 130, 333]
BOOL = [False, True]


def test_hook_is_exported_and_not_in_oi_h():
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\b[TW] oi_test_cell_doubles\b', out)
    assert 'oi_test_cell_doubles' not in _lib.SIGNATURES
    assert W.cell_doubles(7, 1) == -1      # an unknown path


@pytest.mark.parametrize('cov, host', itertools.product(BOOL, BOOL))
def test_predict_multi(cov, host):
    for n, nt in itertools.product(SIZES, SIZES):
        assert W.cell_doubles(W.PREDICT, n, nt, cov=cov, host=host) == W.predict_form(n, nt, cov, host), (n, nt)


@pytest.mark.parametrize('host', BOOL)
def test_loo(host):
    for n in SIZES:
        assert W.cell_doubles(W.LOO, n, host=host) == W.loo_form(n, host), n
    # the multi-chunk case of tests/test_gpu_loo.py: its largest cell
    assert W.cell_doubles(W.LOO, 333, host=True) == 200016


@pytest.mark.parametrize('cov, host, elbo', itertools.product(BOOL, BOOL, BOOL))
def test_svgp(cov, host, elbo):
    lib = _lib.load()
    for M in (1, 32, 33, 64):
        assert lib.oi_svgp_param_count(M) == 6 + 4 * M + M * (M + 1) // 2
        for n in SIZES:
            assert W.cell_doubles(W.SVGP, n, M=M, cov=cov, host=host, elbo=elbo) == W.svgp_form(M, n, cov, host, elbo), \
                (M, n)


@pytest.mark.parametrize('cov', BOOL)
def test_nystrom_predict_multi(cov):
    for M, n, nt in itertools.product((1, 32, 33, 64, 65), SIZES, SIZES):
        assert W.cell_doubles(W.NYSTROM, n, nt, M, cov=cov) == W.nystrom_form(n, M, nt, cov), (M, n, nt)


# The Nystrom Runner's two workspaces.  Its chunk size is cut by the one-slot
# count, which must stay the closed form its constructor held; the arrays it
# carves must be the sizes its kernels index (a short array is an out-of-bounds
# write on the GPU, so this is where a mistyped size is caught).
RUNNER_NM = [(n, M) for n in (1, 63, 64, 65, 129, 333, 3000) for M in (1, 31, 32, 33, 64, 65, 128) if M <= n]
RUNNER_CH = [1, 2, 64]


def test_runner_hook_is_exported_and_not_in_oi_h():
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r'\b[TW] oi_test_nystrom_runner_doubles\b', out)
    assert 'oi_test_nystrom_runner_doubles' not in _lib.SIGNATURES
    assert W.runner_doubles(3, 64, 32, 1, 32) == -1      # an unknown `which`


@pytest.mark.parametrize('padq', [0, 32])
def test_nystrom_runner_slots(padq):
    for (n, M), ch in itertools.product(RUNNER_NM, RUNNER_CH):
        one = W.runner_doubles(W.ONE_SLOT, n, M, ch, padq)
        alloc = W.runner_doubles(W.SLOTS, n, M, ch, padq)
        assert one == W.runner_one_slot_form(n, M, padq), (n, M)
        assert alloc == W.runner_slots_form(n, M, ch, padq), (n, M, ch)
        assert alloc >= ch * one, (n, M, ch)


# the flag combinations a Runner is built with: objective fused / unfused, predict only, neither
@pytest.mark.parametrize('flags', [W.OBJ | W.FUSED, W.OBJ, W.PRED | W.FUSED, W.PRED, W.FUSED, 0])
def test_nystrom_runner_fixed(flags):
    for (n, M), cap in itertools.product(RUNNER_NM, RUNNER_CH):
        assert W.runner_doubles(W.FIXED, n, M, cap, 32, flags) == W.runner_fixed_form(n, M, cap, flags), (n, M, cap)
