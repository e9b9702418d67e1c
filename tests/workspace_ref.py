"""The staged entry points' per-cell workspace counts: the library's test hook
``oi_test_cell_doubles`` (which runs each path's layout function on a counting
Carver) and, beside it, the four closed forms that the sources held before the
layouts replaced them.  The closed forms are the specification: the chunk
planner cuts by these numbers, so every ``pool_bytes`` in the GPU tests depends
on them.  Likewise the Nystrom Runner's two workspaces
(``oi_test_nystrom_runner_doubles``): the one-slot form cuts its chunk size.
No GPU needed."""
import ctypes

from optimalinterpolation_amd import _lib

PREDICT, LOO, SVGP, NYSTROM = 0, 1, 2, 3      # the hook's `path`
COV, HOST, ELBO = 1, 2, 4                     # its `flags`
SLACK = {PREDICT: 8 * 32, LOO: 8 * 32, SVGP: 16 * 32}   # doubles per chunk beside the cells' (CHUNK_SLACK)


def cell_doubles(path, n, nt=0, M=0, cov=False, host=True, elbo=False):
    """What the chunk planner counts for one cell, from the library."""
    fn = _lib.load().oi_test_cell_doubles
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] + [ctypes.c_int64] * 3 + [ctypes.c_int32]
    return fn(path, n, nt, M, COV * bool(cov) + HOST * bool(host) + ELBO * bool(elbo))


def up(v, q):
    return (v + q - 1) // q * q


def predict_form(n, nt, cov, host):
    Np = up(n, 64)
    d = up(3 * n, 32) + up(3 * nt, 32) + Np * Np + Np * 64 + up((nt + 1) * n, 32)
    return d + (nt * nt if cov else 0) + 2 * nt + 3 * nt + (4 * n if host else 0) + 2


def loo_form(n, host):
    Np = up(n, 64)
    return (up(3 * n, 32) + Np * Np + 2 * Np * 64 + up(n, 32) + up(Np // 64, 32) + 2 * n
            + (4 * n if host else 0) + 2)


def svgp_form(M, n, cov, host, elbo):
    rec, params = 8 + 4 * M + M * (M + 1), 6 + 4 * M + M * (M + 1) // 2   # rec_doubles, oi_svgp_param_count
    d = rec + params + 1
    if host:
        d += 3 * n + (n if elbo else 0)
    if elbo:
        return d + (n + 127) // 128 + 1
    return d + 2 * n + (2 * M * n + n * n if cov else 0)


def nystrom_form(n, M, nt, cov):
    Tt = (nt + 63) // 64
    d = up(3 * nt, 32) + up(nt * n, 32) + up(nt * M, 32) + ((n + 63) // 64 + (M + 63) // 64) * Tt * 4096
    return d + (nt * nt if cov else 0)


# ---- the Nystrom Runner's two workspaces (oi_test_nystrom_runner_doubles) ----
FIXED, SLOTS, ONE_SLOT = 0, 1, 2              # the hook's `which`
OBJ, PRED, FUSED = 1, 2, 4                    # its `flags`
NRES, NINFO = 10, 2                           # doubles of results, int32 infos per cell


def runner_doubles(which, nmax, mmax, cap_or_ch, padq, flags=0):
    """A Runner's workspace in doubles, from the library."""
    fn = _lib.load().oi_test_nystrom_runner_doubles
    fn.restype = ctypes.c_int64
    fn.argtypes = [ctypes.c_int32] + [ctypes.c_int64] * 3 + [ctypes.c_int32] * 2
    return fn(which, nmax, mmax, cap_or_ch, padq, flags)


def _padded(mmax, padq):
    """Mp, the eigensolver's workspace for it, its 64-blocks."""
    import oila_ref
    Mp = up(mmax, padq) if padq else mmax
    return Mp, oila_ref.lib().oila_test_eigh_workspace_doubles(Mp), (Mp + 63) // 64


def runner_one_slot_form(nmax, mmax, padq):
    """The constructor's former `per / 8`: what the chunk size is cut by."""
    Mp, ewd, nd64 = _padded(mmax, padq)
    return 6 * nmax + 2 * Mp * Mp + 2 * Mp + 3 * nmax * Mp + ewd + nd64 * 4096


def runner_slots_form(nmax, mmax, ch, padq):
    """ch slots of sc, sq, Kmm, eval, stl, C, B, EW, Dinv, Knm, U1, each array rounded to 32 doubles."""
    Mp, ewd, nd64 = _padded(mmax, padq)
    strides = [3 * nmax, 3 * nmax, Mp * Mp, Mp, Mp, nmax * Mp, Mp * Mp, ewd, nd64 * 4096, nmax * Mp, nmax * Mp]
    return sum(up(ch * s, 32) for s in strides)


def runner_fixed_form(nmax, mmax, cap, flags):
    nt = (nmax + 63) // 64
    arrays = [cap * NRES, (cap * NINFO + 1) // 2, nmax, mmax]
    if flags & OBJ:
        arrays += [(mmax + 63) // 64 * nt * 4096 if flags & FUSED else nmax * nmax, 5 * nt * nt]
    if flags & PRED:
        arrays += [nmax, mmax, 3]
    return sum(up(a, 32) for a in arrays)
