"""The continuous-batching engine's memory sizes (csrc/oi_engine.cpp): the
library's test hooks and, beside them, the closed forms restated here as the
specification.  A resident cell owns ``cell_bytes`` of the device arena, a
submitted batch ``input_bytes``; admission is first-fit over 256-byte granules
(csrc/oi_arena.h).  Every ``pool_bytes`` of tests/test_gpu_engine_admission.py
is computed from these, so they are compared with the hooks to the byte
(tests/test_arena.py).  No GPU needed."""
import ctypes

import numpy as np

from optimalinterpolation_amd import _lib

NB = 64                 # tile edge (OI_NB)
TILE = NB * NB          # doubles of a tile
GRANULE = 256           # bytes


def up(v, q=GRANULE):
    return (int(v) + q - 1) // q * q


def tiles(n):
    return (int(n) + NB - 1) // NB


def cell_bytes_form(n, eval_mem):
    """L | W (cells that evaluate the objective: fits and eval-only) | Dinv |
    4 vectors | partial sums, each rounded to the granule."""
    T = tiles(n)
    nt = T * (T + 1) // 2
    pieces = [nt * TILE * 8] * (2 if eval_mem else 1) + [T * TILE * 8, 4 * T * NB * 8, (5 * nt + 5 * T) * 8]
    return int(np.sum([up(p) for p in pieces], dtype=np.int64))


def input_bytes_form(N, ncell, host_inputs):
    """residuals | sites | v | d | offs | m | SSW | the rows' copy (host inputs),
    over N observations in ncell cells (an empty array still takes a granule)."""
    N1, C1 = max(int(N), 1), max(int(ncell), 1)
    pieces = [8 * N1, 24 * N1, 8 * N1, 8 * N1, 8 * (C1 + 1), 4 * C1, 8 * C1] + ([24 * N1] if host_inputs else [])
    return int(np.sum([up(p) for p in pieces], dtype=np.int64))


def _hook(name, restype, argtypes):
    fn = getattr(_lib.load(), name)
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def cell_bytes(n, eval_mem):
    """A resident cell's arena block, from the library."""
    return _hook('oi_test_engine_cell_bytes', ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32])(int(n), int(bool(eval_mem)))


def input_bytes(N, ncell, host_inputs=True):
    """A submitted batch's input block, from the library."""
    return _hook('oi_test_engine_input_bytes', ctypes.c_int64,
                 [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32])(int(N), int(ncell), int(bool(host_inputs)))


def arena_state(device=0):
    """(size, free bytes, largest free block) of the device's engine arena, or
    None when no call has built one yet."""
    out = (ctypes.c_int64 * 3)()
    rc = _hook('oi_test_engine_arena', ctypes.c_int32, [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)])(device, out)
    return None if rc else tuple(out)
