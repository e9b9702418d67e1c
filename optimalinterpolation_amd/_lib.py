"""ctypes binding of liboi.so (include/oi.h).

The shared library is built in-tree by ``make -C optimalinterpolation_amd``
(or ``__graft_entry__.build()``).  It is the product path: there is no CPU
fallback, and every entry point raises if the library or a GPU is missing.

PyTorch is imported first (when present) so that liboi.so binds to the same
HIP runtime instance that torch already loaded (both carry the soname
libamdhip64.so.7); streams handed over from torch are then valid here.
"""
import ctypes
import os
import threading
import types

import numpy as np

try:  # plumbing only: share torch's HIP runtime if torch is in the process
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# OI_LIB: load a differently-built variant (A/B experiments); default the in-tree build
LIB_PATH = os.environ.get('OI_LIB') or os.path.join(_HERE, 'liboi.so')

_lib = None
_lock = threading.Lock()

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_int32_p = ctypes.POINTER(ctypes.c_int32)


class OiOptions(ctypes.Structure):
    _fields_ = [('device', ctypes.c_int32), ('maxiter', ctypes.c_int32), ('gtol', ctypes.c_double),
                ('stream', ctypes.c_void_p), ('pool_bytes', ctypes.c_int64),
                ('max_pool', ctypes.c_int32), ('profile', ctypes.c_int32),
                ('device_inputs', ctypes.c_int32)]


class OiError(RuntimeError):
    pass


def _signatures():
    D, L, I = c_double_p, c_int64_p, c_int32_p
    f, l, i, u, n = ctypes.c_double, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int
    H, S, O, U = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(OiOptions), ctypes.POINTER(ctypes.c_uint64)
    fit = [D, D, L, l, L, L, D, D, f, D, I, I]   # the Nystrom fit's arguments up to info
    gpr = [D, D, L, l, D, f, D, i, D, D, I, I]   # oi_gpr_batch's arguments up to info
    return {
        'oi_options_default': (None, [O]),
        'oi_gpr_batch': (n, gpr + [O]),
        'oi_gpr_predict_multi': (n, [D, D, L, l, D, L, f, D, D, D, D, D, I, O]),
        'oi_gpr_loo': (n, [D, D, L, l, f, D, D, D, D, I, O]),
        'oi_gpr_lgo': (n, [D, D, L, l, L, f, D, D, D, D, D, D, I, O]),
        'oi_gpr_sample': (n, [D, D, L, l, D, L, f, D, l, i, f, u, U, D, D, D, D, I, O]),
        'oi_nlml_grad_batch': (n, [D, D, D, L, l, D, D, D, I, O]),
        'oi_cg_create': (H, [D, f, i]),
        'oi_cg_step': (n, [H, D]),
        'oi_cg_feed': (n, [H, f, D]),
        'oi_cg_result': (n, [H, D, D, I, I, L, L, L]),
        'oi_cg_destroy': (None, [H]),
        'oi_last_error': (S, []),
        'oi_version': (i, []),
        'oi_profile_json': (l, [S, l]),
        'oi_profile_reset': (None, []),
        'oi_smooth_fields': (n, [D, i, l, l, D, D, f, D, i, D, O]),
        'oi_ball_query': (n, [D, l, D, l, f, L, L, l, O]),
        'oi_gather_rows': (n, [D, D, D, D, l, L, l, D, D, O]),
        'oi_nystrom_batch': (n, [D, D, L, l, L, L, D, D, f, D, D, D, I, O]),
        'oi_nystrom_predict_multi': (n, [D, D, L, l, L, L, D, D, L, f, D, D, D, I, O]),
        'oi_nystrom_fit_batch': (n, fit + [O]),
        'oi_svgp_param_count': (i, [i]),
        'oi_svgp_batch': (n, [D, D, L, l, D, i, D, i, i, i, u, f, D, D, D, D, I, O]),
        'oi_svgp_predict': (n, [D, i, l, D, L, i, D, D, D, I, O]),
        'oi_svgp_elbo': (n, [D, i, D, D, L, l, D, I, O]),
        'oi_nystrom_session_create': (H, [O]),
        'oi_nystrom_session_submit': (l, [H] + fit),
        'oi_nystrom_session_wait': (n, [H, l]),
        'oi_nystrom_session_destroy': (None, [H]),
        'oi_session_create': (H, [O]),
        'oi_session_submit': (l, [H] + gpr),
        'oi_session_set_stream': (n, [H, H]),
        'oi_session_wait': (n, [H, l]),
        'oi_session_done': (n, [H, l]),
        'oi_session_destroy': (None, [H]),
    }


# name -> (restype, argtypes) of every symbol include/oi.h declares, the one
# header and the one table; load() applies it and tests/test_abi.py compares it
# with the header's prototypes
SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def _ext_signatures():
    D, L, I, O = c_double_p, c_int64_p, c_int32_p, ctypes.POINTER(OiOptions)
    f, l, n = ctypes.c_double, ctypes.c_int64, ctypes.c_int
    return {
        'oi_gpr_predict_grad': (n, [D, D, L, l, D, L, f, D, D, D, D, D, D, D, I, O]),
    }


# the same for include/oi_ext.h, where the entries after oi.h's are declared
# (tests/test_grad_abi.py compares it with that header)
EXT_SIGNATURES = _ext_signatures()


def load():
    """Load liboi.so (once).  Raises OiError when it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise OiError(f"{LIB_PATH} not built: run `make -C {_HERE}` (or __graft_entry__.build())")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in {**SIGNATURES, **EXT_SIGNATURES}.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def _ptr(a, ctype=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(ctype)) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _check(rc):
    if rc != 0:
        raise OiError(f"liboi error {rc}: {load().oi_last_error().decode(errors='replace')}")


def options(device=0, maxiter=-1, gtol=1e-5, stream=None, pool_bytes=0, max_pool=0, profile=False,
            device_inputs=False):
    o = OiOptions()
    load().oi_options_default(ctypes.byref(o))
    o.device = int(device)
    o.maxiter = int(maxiter)
    o.gtol = float(gtol)
    o.stream = stream
    o.pool_bytes = int(pool_bytes)
    o.max_pool = int(max_pool)
    o.profile = 1 if profile else 0
    o.device_inputs = 1 if device_inputs else 0
    return o


def _check_dev(t, device, dtype='float64', n=None, what='tensor'):
    """A device tensor handed to liboi: right dtype, on cuda:<device> (any
    ordinal when ``device`` is None), contiguous, ``n`` elements (liboi reads
    8 bytes per element)."""
    if str(getattr(t, 'dtype', None)) != f'torch.{dtype}':
        raise ValueError(f"{what} must be torch.{dtype}, got {getattr(t, 'dtype', type(t))}")
    index = t.device.index if t.device.index is not None else 0
    if t.device.type != 'cuda' or (device is not None and index != int(device)):
        raise ValueError(f"{what} must live on cuda{'' if device is None else f':{device}'}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if n is not None and t.numel() != n:
        raise ValueError(f"{what} has {t.numel()} elements, expected {n}")


def _dptr(t, device, ctype=ctypes.c_double, n=None, what='tensor'):
    """Device pointer of a torch tensor that passes _check_dev (fp64 or int64)."""
    _check_dev(t, device, 'int64' if ctype is ctypes.c_int64 else 'float64', n, what)
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctype))


def _obs(xyt, y, offs, device_inputs=False, device=0, what='y'):
    """The observations of a ragged batch, ``xyt`` [N x 3] and ``y`` [N] cut by
    ``offs`` (int64, from _i64): their two pointers and the objects that keep
    them alive.  Host arrays become contiguous fp64 and must agree with
    ``offs``; with ``device_inputs`` both are fp64 contiguous torch tensors on
    cuda:``device`` with 3 N and N elements."""
    if len(offs) == 0 or offs[0] != 0:
        raise ValueError("inconsistent ragged batch")
    N = int(offs[-1])
    if device_inputs:
        return (_dptr(xyt, device, n=3 * N, what='xyt'), _dptr(y, device, n=N, what=what), (xyt, y))
    xyt = _f64(xyt).reshape(-1, 3)
    y = _f64(y).reshape(-1)
    if N != len(y) or xyt.shape[0] != len(y):
        raise ValueError("inconsistent ragged batch")
    return _ptr(xyt), _ptr(y), (xyt, y)


def _sync_producers(device):
    """The Nystrom entry points run on private non-blocking streams and the
    SVGP ones on ``opts.stream`` (the NULL stream unless the caller sets it),
    neither ordered after torch's current stream: wait here until that stream
    has produced their device inputs."""
    import torch
    torch.cuda.current_stream(int(device)).synchronize()


def _caller_stream(device):
    """torch's current stream on ``device`` as a hipStream_t (None = the
    legacy NULL stream, which the library then waits for itself)."""
    import torch
    h = torch.cuda.current_stream(device).cuda_stream
    return h or None


def _gpr_args(xs, ncell, x0, opt, hyp):
    """oi_gpr_batch's host metadata, checked: (xs [ncell x 3], x0 [6] | None, hyp [ncell x 5] | None)."""
    xs = _f64(xs).reshape(-1, 3)
    if xs.shape[0] != ncell:
        raise ValueError("inconsistent ragged batch")
    x0a = _f64(x0) if x0 is not None else None
    hypa = _f64(hyp).reshape(-1, 5) if hyp is not None else None
    if opt and (x0a is None or x0a.shape != (6,)):
        raise ValueError("opt=True needs x0 of length 6")
    if not opt and (hypa is None or hypa.shape[0] != ncell):
        raise ValueError("opt=False needs hyp [ncell x 5]")
    return xs, x0a, hypa


def gpr_batch(xyt, z, offs, xs, mean, x0=None, opt=True, hyp=None, info=False, device_inputs=False,
              **opt_kw):
    """oi_gpr_batch: returns (out [ncell x 8], status [ncell], info [ncell x 4] or None).
    With device_inputs=True ``xyt`` / ``z`` are fp64 contiguous torch tensors on
    cuda:``device`` and the launches are ordered after torch's current stream
    (include/oi.h, stream ordering); the metadata stays on the host."""
    lib = load()
    offs = _i64(offs)
    ncell = len(offs) - 1
    dev = int(opt_kw.get('device', 0))
    xs, x0a, hypa = _gpr_args(xs, ncell, x0, opt, hyp)
    px, pz, _keep = _obs(xyt, z, offs, device_inputs, dev, what='z')
    if device_inputs:
        opt_kw.setdefault('stream', _caller_stream(dev))
    out = np.empty((ncell, 8))
    status = np.zeros(ncell, dtype=np.int32)
    inf = np.zeros((ncell, 4), dtype=np.int32) if info else None
    o = options(device_inputs=device_inputs, **opt_kw)
    _check(lib.oi_gpr_batch(px, pz, _ptr(offs, ctypes.c_int64), ncell, _ptr(xs), float(mean),
                            _ptr(x0a), 1 if opt else 0, _ptr(hypa), _ptr(out),
                            _ptr(status, ctypes.c_int32), _ptr(inf, ctypes.c_int32), ctypes.byref(o)))
    return out, status, inf


def gpr_batch_device(xyt_dev, z_dev, offs, xs, mean, **kw):
    """gpr_batch(..., device_inputs=True)."""
    return gpr_batch(xyt_dev, z_dev, offs, xs, mean, device_inputs=True, **kw)


def _dense_args(xyt, z, offs, hyp, device_inputs, opt_kw, xs=None, toffs=None):
    """What gpr_predict_multi, gpr_loo, gpr_lgo, gpr_sample and gpr_predict_grad share, checked:
    the ragged batch (and, with ``toffs``, its targets ``xs`` [T x 3]), ``hyp``
    [ncell x 5], the observations' pointers, torch's current stream for device
    inputs, the options and a zeroed status.  Returns them as one namespace;
    ``head`` holds the C arguments every one of the four entries begins with."""
    a = types.SimpleNamespace(offs=_i64(offs), xs=None, toffs=None)
    a.ncell = len(a.offs) - 1
    if toffs is not None:
        a.toffs, a.xs = _i64(toffs), _f64(xs).reshape(-1, 3)
        if len(a.toffs) != a.ncell + 1 or a.toffs[0] != 0 or a.toffs[-1] != a.xs.shape[0]:
            raise ValueError("inconsistent ragged batch")
    a.hyp = _f64(hyp).reshape(-1, 5)
    if a.hyp.shape[0] != a.ncell:
        raise ValueError("hyp must be [ncell x 5]")
    dev = int(opt_kw.get('device', 0))
    px, pz, a.keep = _obs(xyt, z, a.offs, device_inputs, dev, what='z')
    if device_inputs:
        opt_kw.setdefault('stream', _caller_stream(dev))
    a.head = (px, pz, _ptr(a.offs, ctypes.c_int64), a.ncell)
    a.opts = options(device_inputs=device_inputs, **opt_kw)
    a.status = np.zeros(a.ncell, dtype=np.int32)
    return a


def gpr_predict_multi(xyt, z, offs, xs, toffs, mean, hyp, cov=False, lz=True, device_inputs=False,
                      **opt_kw):
    """oi_gpr_predict_multi: predict every cell at its own list of targets
    (``xs`` [T x 3], cell c owning rows toffs[c]:toffs[c+1]) at LINEAR hypers
    ``hyp`` [ncell x 5].  Returns (fs [T], sd [T], lz [ncell] | None, cov | None,
    status [ncell]); ``cov`` is the flat array of the cells' nt x nt posterior
    covariances back to back (``split_cov`` cuts it up).  With
    device_inputs=True ``xyt`` / ``z`` are fp64 contiguous torch tensors on
    cuda:``device`` and the call runs on torch's current stream; targets,
    offsets and hypers stay on the host."""
    a = _dense_args(xyt, z, offs, hyp, device_inputs, opt_kw, xs, toffs)
    T = int(a.toffs[-1])
    fs = np.empty(T)
    sd = np.empty(T)
    lza = np.empty(a.ncell) if lz else None
    nt = np.diff(a.toffs)
    cova = np.empty(int((nt * nt).sum())) if cov else None
    _check(load().oi_gpr_predict_multi(*a.head, _ptr(a.xs), _ptr(a.toffs, ctypes.c_int64), float(mean), _ptr(a.hyp),
                                       _ptr(fs), _ptr(sd), _ptr(lza), _ptr(cova), _ptr(a.status, ctypes.c_int32),
                                       ctypes.byref(a.opts)))
    return fs, sd, lza, cova, a.status


def gpr_predict_multi_device(xyt_dev, z_dev, offs, xs, toffs, mean, hyp, **kw):
    """gpr_predict_multi(..., device_inputs=True)."""
    return gpr_predict_multi(xyt_dev, z_dev, offs, xs, toffs, mean, hyp, device_inputs=True, **kw)


def gpr_loo(xyt, z, offs, mean, hyp, lpl=True, device_inputs=False, **opt_kw):
    """oi_gpr_loo: leave-one-out cross-validation of every cell at LINEAR hypers
    ``hyp`` [ncell x 5], from one factorisation per cell.  Returns (mu [N],
    sd [N], lpl [ncell] | None, status [ncell]): ``mu[i]`` / ``sd[i]`` are the
    predictive mean and standard deviation of OBSERVATION i (noise included)
    given the other observations of its cell, in the observations' own order --
    the standardised residual is ``(z - mu) / sd`` -- and ``lpl`` the cells' log
    pseudo-likelihoods.  A cell whose factorisation fails has status 1 and NaN
    results.  With device_inputs=True ``xyt`` / ``z`` are fp64 contiguous torch
    tensors on cuda:``device`` and the call runs on torch's current stream;
    offsets and hypers stay on the host."""
    a = _dense_args(xyt, z, offs, hyp, device_inputs, opt_kw)
    N = int(a.offs[-1])
    mu = np.empty(N)
    sd = np.empty(N)
    lpla = np.empty(a.ncell) if lpl else None
    _check(load().oi_gpr_loo(*a.head, float(mean), _ptr(a.hyp), _ptr(mu), _ptr(sd), _ptr(lpla),
                             _ptr(a.status, ctypes.c_int32), ctypes.byref(a.opts)))
    return mu, sd, lpla, a.status


def gpr_loo_device(xyt_dev, z_dev, offs, mean, hyp, **kw):
    """gpr_loo(..., device_inputs=True)."""
    return gpr_loo(xyt_dev, z_dev, offs, mean, hyp, device_inputs=True, **kw)


def gpr_lgo(xyt, z, offs, group, mean, hyp, lpd=True, d2=True, lpl=True, device_inputs=False, **opt_kw):
    """oi_gpr_lgo: leave-group-out cross-validation of every cell at LINEAR
    hypers ``hyp`` [ncell x 5], from one factorisation per cell.  ``group`` [N]
    labels every observation (any int64; compared only inside a cell, only for
    equality); every group is predicted jointly from the cell's observations
    outside it.  Returns (mu [N], sd [N], lpd [N] | None, d2 [N] | None,
    lpl [ncell] | None, status [ncell]): ``mu[i]`` / ``sd[i]`` are the predictive
    mean and standard deviation of OBSERVATION i (noise included) given the
    observations outside its group, in the observations' own order; ``lpd[i]``
    and ``d2[i]`` are the joint log predictive density and the squared
    Mahalanobis distance of i's group, repeated for every member; ``lpl`` sums
    ``lpd`` over a cell's groups.  Status 1: the cell's factorisation failed
    (all NaN); 2: some group's block failed to factor (those groups' rows and
    ``lpl`` NaN).  With device_inputs=True ``xyt`` / ``z`` are fp64 contiguous
    torch tensors on cuda:``device`` and the call runs on torch's current
    stream; labels, offsets and hypers stay on the host."""
    a = _dense_args(xyt, z, offs, hyp, device_inputs, opt_kw)
    N = int(a.offs[-1])
    group = _i64(group)
    if len(group) != N:
        raise ValueError("group must label every observation")
    mu = np.empty(N)
    sd = np.empty(N)
    lpda = np.empty(N) if lpd else None
    d2a = np.empty(N) if d2 else None
    lpla = np.empty(a.ncell) if lpl else None
    _check(load().oi_gpr_lgo(*a.head, _ptr(group, ctypes.c_int64), float(mean), _ptr(a.hyp), _ptr(mu), _ptr(sd),
                             _ptr(lpda), _ptr(d2a), _ptr(lpla), _ptr(a.status, ctypes.c_int32),
                             ctypes.byref(a.opts)))
    return mu, sd, lpda, d2a, lpla, a.status


def gpr_lgo_device(xyt_dev, z_dev, offs, group, mean, hyp, **kw):
    """gpr_lgo(..., device_inputs=True)."""
    return gpr_lgo(xyt_dev, z_dev, offs, group, mean, hyp, device_inputs=True, **kw)


def gpr_sample(xyt, z, offs, xs, toffs, mean, hyp, nsamp, noise=False, jitter=0.0, seed=0, streams=None, xi=None,
               device_inputs=False, **opt_kw):
    """oi_gpr_sample: ``nsamp`` joint draws from every cell's posterior at its
    own targets (``xs`` [T x 3], cell c owning rows toffs[c]:toffs[c+1]) at
    LINEAR hypers ``hyp`` [ncell x 5].  Returns (samples [T x nsamp], fs [T],
    sd [T], status [ncell]): row ``toffs[c] + t`` of ``samples`` holds the draws
    at target t of cell c, column s is draw s, and the columns of a cell are
    jointly normal with mean ``fs`` and the posterior covariance of
    ``gpr_predict_multi(cov=True)`` (plus sn2 on its diagonal with ``noise``:
    draws of new observations; plus the absolute variance ``jitter``).  With
    ``xi`` [T x nsamp] the standard normals are the caller's; otherwise they are
    generated on the device from ``seed`` and the cells' 64-bit ``streams``
    [ncell] (default: the cell's index in the call), so that a cell's draws
    depend only on (seed, its stream, its number of targets, the columns asked
    for).  Status 1: the cell's factorisation failed (all NaN); 2: the posterior
    covariance did not factor (NaN samples, valid fs and sd; add ``jitter`` or
    ``noise``).  With device_inputs=True ``xyt`` / ``z`` are fp64 contiguous
    torch tensors on cuda:``device`` and the call runs on torch's current
    stream; everything else stays on the host."""
    a = _dense_args(xyt, z, offs, hyp, device_inputs, opt_kw, xs, toffs)
    nsamp = int(nsamp)
    if nsamp < 0:
        raise ValueError("nsamp must be >= 0")
    T = int(a.toffs[-1])
    if streams is not None:
        streams = np.ascontiguousarray(streams, dtype=np.uint64).reshape(-1)
        if len(streams) != a.ncell:
            raise ValueError("streams must be [ncell]")
    if xi is not None:
        xi = _f64(xi)
        if xi.size != T * nsamp:
            raise ValueError("xi must be [T x nsamp]")
    samples = np.empty((T, nsamp))
    fs = np.empty(T)
    sd = np.empty(T)
    _check(load().oi_gpr_sample(*a.head, _ptr(a.xs), _ptr(a.toffs, ctypes.c_int64), float(mean), _ptr(a.hyp), nsamp,
                                1 if noise else 0, float(jitter), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                _ptr(streams, ctypes.c_uint64), _ptr(xi), _ptr(samples), _ptr(fs), _ptr(sd),
                                _ptr(a.status, ctypes.c_int32), ctypes.byref(a.opts)))
    return samples, fs, sd, a.status


def gpr_sample_device(xyt_dev, z_dev, offs, xs, toffs, mean, hyp, nsamp, **kw):
    """gpr_sample(..., device_inputs=True)."""
    return gpr_sample(xyt_dev, z_dev, offs, xs, toffs, mean, hyp, nsamp, device_inputs=True, **kw)


def gpr_predict_grad(xyt, z, offs, xs, toffs, mean, hyp, blk=False, cov=False, device_inputs=False, **opt_kw):
    """oi_gpr_predict_grad (include/oi_ext.h): the posterior of the field and of
    its gradient at every cell's own targets (``xs`` [T x 3], cell c owning rows
    toffs[c]:toffs[c+1]) at LINEAR hypers ``hyp`` [ncell x 5].  Returns (grad
    [T x 3], gsd [T x 3], fs [T], sd [T], blk [T x 4 x 4] | None, cov | None,
    status [ncell]): ``grad`` is the posterior mean of (df/dx, df/dy, df/dt) in
    the inputs' units and ``gsd`` its standard deviation; ``fs`` / ``sd`` are
    ``gpr_predict_multi``'s bit for bit; ``blk[t]`` is the 4 x 4 posterior
    covariance of (f, df/dx, df/dy, df/dt) at target t; ``cov`` is the flat
    array of the cells' (4 nt) x (4 nt) joint covariances back to back, index
    4 t + k (``split_jcov`` cuts it up).  A cell whose factorisation fails has
    status 1 and NaN results.  With device_inputs=True ``xyt`` / ``z`` are fp64
    contiguous torch tensors on cuda:``device`` and the call runs on torch's
    current stream; targets, offsets and hypers stay on the host."""
    a = _dense_args(xyt, z, offs, hyp, device_inputs, opt_kw, xs, toffs)
    T = int(a.toffs[-1])
    grad = np.empty((T, 3))
    gsd = np.empty((T, 3))
    fs = np.empty(T)
    sd = np.empty(T)
    blka = np.empty((T, 4, 4)) if blk else None
    nt = np.diff(a.toffs)
    cova = np.empty(int((16 * nt * nt).sum())) if cov else None
    _check(load().oi_gpr_predict_grad(*a.head, _ptr(a.xs), _ptr(a.toffs, ctypes.c_int64), float(mean), _ptr(a.hyp),
                                      _ptr(grad), _ptr(gsd), _ptr(fs), _ptr(sd), _ptr(blka), _ptr(cova),
                                      _ptr(a.status, ctypes.c_int32), ctypes.byref(a.opts)))
    return grad, gsd, fs, sd, blka, cova, a.status


def gpr_predict_grad_device(xyt_dev, z_dev, offs, xs, toffs, mean, hyp, **kw):
    """gpr_predict_grad(..., device_inputs=True)."""
    return gpr_predict_grad(xyt_dev, z_dev, offs, xs, toffs, mean, hyp, device_inputs=True, **kw)


def split_jcov(cov, toffs):
    """The flat ``cov`` of gpr_predict_grad as a list of 4 nt x 4 nt arrays (views)."""
    m = 4 * np.diff(np.asarray(toffs, dtype=np.int64))
    o = np.concatenate([[0], np.cumsum(m * m)])
    return [cov[o[c]:o[c + 1]].reshape(m[c], m[c]) for c in range(len(m))]


def split_cov(cov, toffs):
    """The flat ``cov`` of gpr_predict_multi as a list of nt x nt arrays (views)."""
    nt = np.diff(np.asarray(toffs, dtype=np.int64))
    o = np.concatenate([[0], np.cumsum(nt * nt)])
    return [cov[o[c]:o[c + 1]].reshape(nt[c], nt[c]) for c in range(len(nt))]


class _SessionBase:
    """What oi_session_* and oi_nystrom_session_* share: the handle, the
    tickets in flight with the arrays they keep alive, wait(ticket), close."""
    _PREFIX = None

    def __init__(self, device=0, device_inputs=False, **opt_kw):
        self._lib = load()
        self.device = int(device)
        self.device_inputs = bool(device_inputs)
        self._opts = options(device=device, device_inputs=device_inputs, **opt_kw)
        self._h = self._fn('create')(ctypes.byref(self._opts))
        if not self._h:
            raise OiError(f"{self._PREFIX}_create: {self._lib.oi_last_error().decode(errors='replace')}")
        self._live = {}    # ticket -> (out, status, info, inputs kept alive), not yet complete

    def _fn(self, verb):
        return getattr(self._lib, f'{self._PREFIX}_{verb}')

    def _ticket(self, t, out, status, info, keep):
        if t < 0:
            _check(int(t))
        # device inputs and the outputs must outlive the ticket
        self._live[int(t)] = (out, status, info, keep)
        return int(t)

    def wait(self, ticket):
        """Block until ``ticket`` completes and return its (out, status, info)."""
        ticket = int(ticket)
        if ticket not in self._live:
            raise KeyError(f"unknown or already collected session ticket {ticket}")
        _check(self._fn('wait')(self._h, ticket))
        return self._live.pop(ticket)[:3]

    def close(self):
        if getattr(self, '_h', None):
            self._fn('destroy')(self._h)
            self._h = None
            self._live.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class Session(_SessionBase):
    """oi_session_*: continuous batching across calls (include/oi.h).

    ``submit`` takes the oi_gpr_batch arguments (host numpy arrays, or fp64
    device tensors with ``device_inputs=True``) and returns a ticket;
    ``wait(ticket)`` returns that batch's (out, status, info) once complete,
    leaving later batches' rounds running on the GPU.  Cells of consecutive
    batches share rounds, so a stream of small batches runs at the rate of one
    big call; per-cell results equal oi_gpr_batch's bit for bit.

    Device inputs are ordered after torch's current stream AT EACH SUBMIT
    (oi_session_set_stream), so a producer running under another
    ``torch.cuda.stream(...)`` context is waited for.  Results of a ticket are
    collected once: by ``wait(ticket)``, or in the dict ``wait()`` returns."""
    _PREFIX = 'oi_session'

    def __init__(self, device=0, device_inputs=False, **opt_kw):
        if device_inputs:
            opt_kw.setdefault('stream', _caller_stream(int(device)))
        super().__init__(device, device_inputs, **opt_kw)
        self._done = {}    # ticket -> results completed by wait(-1), not yet collected

    def submit(self, xyt, z, offs, xs, mean, x0=None, opt=True, hyp=None):
        offs = _i64(offs)
        ncell = len(offs) - 1
        xs, x0a, hypa = _gpr_args(xs, ncell, x0, opt, hyp)
        px, pz, keep = _obs(xyt, z, offs, self.device_inputs, self.device, what='z')
        if self.device_inputs:
            _check(self._lib.oi_session_set_stream(self._h, _caller_stream(self.device)))
        out = np.empty((ncell, 8))
        status = np.zeros(ncell, dtype=np.int32)
        info = np.zeros((ncell, 4), dtype=np.int32)
        t = self._lib.oi_session_submit(self._h, px, pz, _ptr(offs, ctypes.c_int64), ncell, _ptr(xs),
                                        float(mean), _ptr(x0a), 1 if opt else 0, _ptr(hypa), _ptr(out),
                                        _ptr(status, ctypes.c_int32), _ptr(info, ctypes.c_int32))
        return self._ticket(t, out, status, info, keep)

    def done(self, ticket):
        return self._lib.oi_session_done(self._h, int(ticket)) == 1

    def wait(self, ticket=-1):
        """Block until ``ticket`` completes and return its (out, status, info).
        ``ticket = -1`` drains all submitted work and returns
        ``{ticket: (out, status, info)}`` for every ticket not collected yet
        (those can still be collected one by one with ``wait(ticket)``)."""
        ticket = int(ticket)
        if ticket in self._done:
            return self._done.pop(ticket)
        if ticket >= 0:
            return super().wait(ticket)
        _check(self._lib.oi_session_wait(self._h, ticket))
        for t, r in self._live.items():
            self._done[t] = r[:3]
        self._live.clear()
        return dict(self._done)

    def close(self):
        super().close()
        self._done = {}


def nlml_grad_batch(xyt, y, mX, offs, h, **opt_kw):
    """oi_nlml_grad_batch: returns (nlz [ncell], grad [ncell x 6], status [ncell])."""
    lib = load()
    offs = _i64(offs)
    px, py, _keep = _obs(xyt, y, offs)
    mX = _f64(mX)
    h = _f64(h).reshape(-1, 6)
    ncell = len(offs) - 1
    if h.shape[0] != ncell or len(mX) != offs[-1]:
        raise ValueError("inconsistent ragged batch")
    nlz = np.empty(ncell)
    grad = np.empty((ncell, 6))
    status = np.zeros(ncell, dtype=np.int32)
    o = options(**opt_kw)
    _check(lib.oi_nlml_grad_batch(px, py, _ptr(mX), _ptr(offs, ctypes.c_int64), ncell, _ptr(h),
                                  _ptr(nlz), _ptr(grad), _ptr(status, ctypes.c_int32), ctypes.byref(o)))
    return nlz, grad, status


def _inducing(sel, soffs, ncell, what="inconsistent inducing rows"):
    """The ragged inducing rows (0-based within each cell), checked against ncell."""
    sel, soffs = _i64(sel), _i64(soffs)
    if len(soffs) != ncell + 1 or soffs[-1] != len(sel):
        raise ValueError(what)
    return sel, soffs


def nystrom_batch(xyt, y, offs, sel, soffs, hyp, xs=None, mean=0.0, objective=True,
                  predict=True, **opt_kw):
    """oi_nystrom_batch: returns (nlz [ncell] | None, grad [ncell x 5] | None,
    pred [ncell x 3] | None, status [ncell]).  ``hyp`` are LINEAR hypers
    (ell_x, ell_y, ell_t, sf2, sn2) per cell; ``sel``/``soffs`` the ragged
    inducing rows (0-based within each cell)."""
    lib = load()
    offs = _i64(offs)
    ncell = len(offs) - 1
    px, py, _keep = _obs(xyt, y, offs)
    hyp = _f64(hyp).reshape(ncell, 5)
    sel, soffs = _inducing(sel, soffs, ncell, "inconsistent ragged batch")
    xs = _f64(xs).reshape(ncell, 3) if predict else None
    nlz = np.empty(ncell) if objective else None
    grad = np.empty((ncell, 5)) if objective else None
    pred = np.empty((ncell, 3)) if predict else None
    status = np.zeros(ncell, dtype=np.int32)
    o = options(**opt_kw)
    _check(lib.oi_nystrom_batch(px, py, _ptr(offs, ctypes.c_int64), ncell, _ptr(sel, ctypes.c_int64),
                                _ptr(soffs, ctypes.c_int64), _ptr(hyp), _ptr(xs), float(mean),
                                _ptr(nlz), _ptr(grad), _ptr(pred), _ptr(status, ctypes.c_int32),
                                ctypes.byref(o)))
    return nlz, grad, pred, status


def nystrom_predict_multi(xyt, y, offs, sel, soffs, hyp, xs, toffs, mean=0.0, cov=False, **opt_kw):
    """oi_nystrom_predict_multi: the Nystrom prediction of every cell at its own
    list of targets (``xs`` [T x 3], cell c owning rows toffs[c]:toffs[c+1]) at
    LINEAR hypers ``hyp`` [ncell x 5]; ``sel``/``soffs`` as nystrom_batch.
    Returns (fs [T], sd [T], cov | None, status [ncell]); ``cov`` is the flat
    array of the cells' nt x nt matrices back to back (``split_cov``).  With
    device_inputs=True ``xyt`` / ``y`` are fp64 contiguous torch tensors on
    cuda:``device``; targets, offsets and hypers stay on the host."""
    offs, toffs = _i64(offs), _i64(toffs)
    xs = _f64(xs).reshape(-1, 3)
    ncell = len(offs) - 1
    if len(toffs) != ncell + 1 or toffs[0] != 0 or toffs[-1] != xs.shape[0]:
        raise ValueError("inconsistent ragged batch")
    hyp = _f64(hyp).reshape(-1, 5)
    if hyp.shape[0] != ncell:
        raise ValueError("hyp must be [ncell x 5]")
    dev_in, dev = bool(opt_kw.get('device_inputs')), int(opt_kw.get('device', 0))
    px, py, _keep = _obs(xyt, y, offs, dev_in, dev)
    if dev_in:
        _sync_producers(dev)
    sel, soffs = _inducing(sel, soffs, ncell, "inconsistent ragged batch")
    T = int(toffs[-1])
    fs = np.empty(T)
    sd = np.empty(T)
    nt = np.diff(toffs)
    cova = np.empty(int((nt * nt).sum())) if cov else None
    status = np.zeros(ncell, dtype=np.int32)
    o = options(**opt_kw)
    _check(load().oi_nystrom_predict_multi(px, py, _ptr(offs, ctypes.c_int64), ncell,
                                           _ptr(sel, ctypes.c_int64), _ptr(soffs, ctypes.c_int64),
                                           _ptr(hyp), _ptr(xs), _ptr(toffs, ctypes.c_int64), float(mean),
                                           _ptr(fs), _ptr(sd), _ptr(cova), _ptr(status, ctypes.c_int32),
                                           ctypes.byref(o)))
    return fs, sd, cova, status


def _nystrom_fit_args(xyt, y, offs, sel, soffs, x0, xs, device_inputs, device):
    """What oi_nystrom_fit_batch and oi_nystrom_session_submit both take, checked:
    the leading C arguments up to ``xs``, ncell, and the inputs to keep alive."""
    offs = _i64(offs)
    ncell = len(offs) - 1
    x0 = _f64(x0).reshape(5)
    xs = _f64(xs).reshape(ncell, 3)
    px, py, keep = _obs(xyt, y, offs, device_inputs, device)
    if device_inputs:
        _sync_producers(device)
    sel, soffs = _inducing(sel, soffs, ncell)
    args = (px, py, _ptr(offs, ctypes.c_int64), ncell, _ptr(sel, ctypes.c_int64),
            _ptr(soffs, ctypes.c_int64), _ptr(x0), _ptr(xs))
    return args, ncell, (keep, offs, sel, soffs, x0, xs)


def nystrom_fit_batch(xyt, y, offs, sel, soffs, x0, xs, mean, **opt_kw):
    """oi_nystrom_fit_batch: returns (out [ncell x 8] = (fs, sd, prior sd, 5 linear
    hypers), status [ncell], info [ncell x 4]).  With device_inputs=True, xyt
    and y are torch device tensors."""
    lib = load()
    args, ncell, _keep = _nystrom_fit_args(xyt, y, offs, sel, soffs, x0, xs,
                                           opt_kw.get('device_inputs'), opt_kw.get('device', 0))
    out = np.empty((ncell, 8))
    status = np.zeros(ncell, dtype=np.int32)
    info = np.zeros((ncell, 4), dtype=np.int32)
    o = options(**opt_kw)
    _check(lib.oi_nystrom_fit_batch(*args, float(mean), _ptr(out), _ptr(status, ctypes.c_int32),
                                    _ptr(info, ctypes.c_int32), ctypes.byref(o)))
    return out, status, info


class NystromSession(_SessionBase):
    """oi_nystrom_session_*: Nystrom fits (oi_nystrom_fit_batch) as a stream of
    batches with continuous batching across calls.  ``submit`` takes
    nystrom_fit_batch's arguments and returns a ticket; ``wait(ticket)``
    returns that batch's (out, status, info) once its last cell is fitted and
    predicted.  Device inputs (``device_inputs=True``) must stay alive until
    their ticket completes (the session keeps a reference)."""
    _PREFIX = 'oi_nystrom_session'

    def submit(self, xyt, y, offs, sel, soffs, x0, xs, mean):
        args, ncell, keep = _nystrom_fit_args(xyt, y, offs, sel, soffs, x0, xs, self.device_inputs,
                                              self.device)
        out = np.empty((ncell, 8))
        status = np.zeros(ncell, dtype=np.int32)
        info = np.zeros((ncell, 4), dtype=np.int32)
        t = self._lib.oi_nystrom_session_submit(self._h, *args, float(mean), _ptr(out),
                                                _ptr(status, ctypes.c_int32), _ptr(info, ctypes.c_int32))
        return self._ticket(t, out, status, info, keep)


def svgp_batch(xyt, y, offs, Z0, init, xs, batch=100, iterations=10000, log_every=10, seed=0,
               lr=1e-3, want_params=False, **opt_kw):
    """oi_svgp_batch: returns (pred [ncell x 2] = (mean, variance of f), status,
    params [ncell x P] or None, elbo [ncell x nlog] or None).
    Z0 [ncell x M x 3]; init [ncell x 6] = (ls_x, ls_y, ls_t, kernel var, noise var, mean)."""
    lib = load()
    offs = _i64(offs)
    ncell = len(offs) - 1
    Z0 = _f64(Z0).reshape(ncell, -1, 3)
    M = Z0.shape[1]
    init = _f64(init).reshape(ncell, 6)
    xs = _f64(xs).reshape(ncell, 3)
    px, py, _keep = _obs(xyt, y, offs, opt_kw.get('device_inputs'), opt_kw.get('device', 0))
    if opt_kw.get('device_inputs'):
        _sync_producers(opt_kw.get('device', 0))
    P = int(lib.oi_svgp_param_count(M))
    nlog = (iterations + log_every - 1) // log_every if log_every else 0
    pred = np.empty((ncell, 2))
    status = np.zeros(ncell, dtype=np.int32)
    params = np.empty((ncell, P)) if want_params else None
    elbo = np.empty((ncell, nlog)) if nlog else None
    o = options(**opt_kw)
    _check(lib.oi_svgp_batch(px, py, _ptr(offs, ctypes.c_int64), ncell, _ptr(Z0), M, _ptr(init),
                             int(batch), int(iterations), int(log_every), int(seed), float(lr),
                             _ptr(xs), _ptr(pred), _ptr(params), _ptr(elbo),
                             _ptr(status, ctypes.c_int32), ctypes.byref(o)))
    return pred, status, params, elbo


def _svgp_rows(params):
    """``params`` as [ncell x P] rows and the M that P = 6 + 4 M + M (M + 1) / 2 belongs to."""
    params = _f64(params)
    if params.ndim == 1:
        params = params[None]
    if params.ndim != 2:
        raise ValueError("params must be [ncell x P]")
    for M in range(1, 65):
        if 6 + 4 * M + M * (M + 1) // 2 == params.shape[1]:
            return params, M
    raise ValueError(f"params rows of length {params.shape[1]} belong to no M in [1, 64]")


def svgp_predict(params, xs, toffs, with_noise=False, cov=False, **opt_kw):
    """oi_svgp_predict: GPflow SVGP.predict_f (``with_noise``: predict_y) of
    trained cells -- ``params`` [ncell x P] as svgp_batch(want_params=True)
    returns them -- at ``xs`` [T x 3], cell c owning rows toffs[c]:toffs[c+1].
    Returns (mean [T], var [T], cov | None, status [ncell]); ``cov`` is the flat
    array of the cells' nt x nt matrices back to back (``split_cov``).  With
    device_inputs=True ``xs`` is a torch device tensor."""
    lib = load()
    params, M = _svgp_rows(params)
    ncell = params.shape[0]
    toffs = _i64(toffs)
    if len(toffs) != ncell + 1 or toffs[0] != 0 or np.any(np.diff(toffs) < 0):
        raise ValueError("inconsistent ragged batch")
    T = int(toffs[-1])
    if opt_kw.get('device_inputs'):
        pxs = _dptr(xs, opt_kw.get('device', 0), n=3 * T, what='xs')
        _sync_producers(opt_kw.get('device', 0))
    else:
        xs = _f64(xs).reshape(-1, 3)
        if xs.shape[0] != T:
            raise ValueError("inconsistent ragged batch")
        pxs = _ptr(xs)
    mean = np.empty(T)
    var = np.empty(T)
    nt = np.diff(toffs)
    cova = np.empty(int((nt * nt).sum())) if cov else None
    status = np.zeros(ncell, dtype=np.int32)
    o = options(**opt_kw)
    _check(lib.oi_svgp_predict(_ptr(params), M, ncell, pxs, _ptr(toffs, ctypes.c_int64),
                               1 if with_noise else 0, _ptr(mean), _ptr(var), _ptr(cova),
                               _ptr(status, ctypes.c_int32), ctypes.byref(o)))
    return mean, var, cova, status


def svgp_elbo(params, xyt, y, offs, **opt_kw):
    """oi_svgp_elbo: model.elbo((X, Y)) on all of each cell's data at ``params``
    [ncell x P].  Returns (elbo [ncell], status [ncell]).  With
    device_inputs=True ``xyt`` and ``y`` are torch device tensors."""
    lib = load()
    params, M = _svgp_rows(params)
    ncell = params.shape[0]
    offs = _i64(offs)
    if len(offs) != ncell + 1:
        raise ValueError("inconsistent ragged batch")
    px, py, _keep = _obs(xyt, y, offs, opt_kw.get('device_inputs'), opt_kw.get('device', 0))
    if opt_kw.get('device_inputs'):
        _sync_producers(opt_kw.get('device', 0))
    elbo = np.empty(ncell)
    status = np.zeros(ncell, dtype=np.int32)
    o = options(**opt_kw)
    _check(lib.oi_svgp_elbo(_ptr(params), M, px, py, _ptr(offs, ctypes.c_int64), ncell, _ptr(elbo),
                            _ptr(status, ctypes.c_int32), ctypes.byref(o)))
    return elbo, status


class CG:
    """The host optimiser (scipy CG restated in C++), driven from Python."""

    def __init__(self, x0, gtol=1e-5, maxiter=-1):
        self._lib = load()
        x0 = _f64(x0)
        self._h = self._lib.oi_cg_create(_ptr(x0), float(gtol), int(maxiter))
        if not self._h:
            raise OiError(self._lib.oi_last_error().decode())
        self._x = np.empty(6)

    def step(self):
        """None when finished, else the point (6,) whose f, g are needed."""
        rc = self._lib.oi_cg_step(self._h, _ptr(self._x))
        if rc < 0:
            _check(rc)
        return None if rc == 0 else self._x.copy()

    def feed(self, f, g):
        g = _f64(g)
        _check(self._lib.oi_cg_feed(self._h, float(f), _ptr(g)))

    def result(self):
        x = np.empty(6)
        fun = ctypes.c_double()
        nit = ctypes.c_int32()
        st = ctypes.c_int32()
        nfev = ctypes.c_int64()
        njev = ctypes.c_int64()
        nobj = ctypes.c_int64()
        _check(self._lib.oi_cg_result(self._h, _ptr(x), ctypes.byref(fun), ctypes.byref(nit),
                                      ctypes.byref(st), ctypes.byref(nfev), ctypes.byref(njev),
                                      ctypes.byref(nobj)))
        return dict(x=x, fun=fun.value, nit=nit.value, status=st.value, nfev=nfev.value,
                    njev=njev.value, nobj=nobj.value)

    def __del__(self):
        if getattr(self, '_h', None):
            self._lib.oi_cg_destroy(self._h)
            self._h = None


def smooth_fields(fields, vmax, mask, kern, **opt_kw):
    """oi_smooth_fields (GPR:65-76 for nf fields): fields [nf, ny, nx] host
    arrays; kern the Gaussian2DKernel array (odd square).  Returns [nf, ny, nx]."""
    lib = load()
    f = _f64(fields)
    if f.ndim == 2:
        f = f[None]
    nf, ny, nx = f.shape
    vm = np.ascontiguousarray(np.broadcast_to(np.asarray(vmax, dtype=np.float64), (nf,)))
    m = _f64(mask)
    k = _f64(kern)
    if m.shape != (ny, nx) or k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 != 1:
        raise ValueError("mask must be [ny, nx] and kern an odd square")
    out = np.empty_like(f)
    _check(lib.oi_smooth_fields(_ptr(f), nf, ny, nx, _ptr(vm), _ptr(m), 0.0, _ptr(k), k.shape[0],
                                _ptr(out), ctypes.byref(options(**opt_kw))))
    return out


# The three day helpers below take device tensors on ANY GPU (_dptr with
# device=None) and launch on ``device=`` (default 0): callers on other ranks
# rely on that today, see DESIGN.md.

def smooth_fields_device(fields_dev, vmax, mask_dev, kern, out_dev, **opt_kw):
    """oi_smooth_fields on HBM-resident tensors ([nf, ny, nx] fp64 in and out)."""
    lib = load()
    nf, ny, nx = fields_dev.shape
    if tuple(mask_dev.shape) != (ny, nx) or tuple(out_dev.shape) != (nf, ny, nx):
        raise ValueError("shape mismatch")
    vm = np.ascontiguousarray(np.broadcast_to(np.asarray(vmax, dtype=np.float64), (nf,)))
    k = _f64(kern)
    _check(lib.oi_smooth_fields(_dptr(fields_dev, None), nf, ny, nx, _ptr(vm), _dptr(mask_dev, None),
                                0.0, _ptr(k), k.shape[0], _dptr(out_dev, None),
                                ctypes.byref(options(device_inputs=True, **opt_kw))))
    return out_dev


def ball_query(pts, q, r, **opt_kw):
    """oi_ball_query on host arrays: returns (offs [Q+1], idx [offs[-1]])."""
    lib = load()
    P = _f64(pts).reshape(-1, 2)
    Qa = _f64(q).reshape(-1, 2)
    offs = np.zeros(len(Qa) + 1, dtype=np.int64)
    o = options(**opt_kw)
    _check(lib.oi_ball_query(_ptr(P), len(P), _ptr(Qa), len(Qa), float(r), _ptr(offs, ctypes.c_int64),
                             None, 0, ctypes.byref(o)))
    idx = np.empty(int(offs[-1]), dtype=np.int64)
    if len(idx):
        _check(lib.oi_ball_query(_ptr(P), len(P), _ptr(Qa), len(Qa), float(r),
                                 _ptr(offs, ctypes.c_int64), _ptr(idx, ctypes.c_int64), len(idx),
                                 ctypes.byref(o)))
    return offs, idx


def ball_query_device(pts_dev, q_dev, r, counts_only=False, **opt_kw):
    """oi_ball_query on HBM-resident [M, 2] / [Q, 2] tensors: returns
    (offs host [Q+1], idx device int64 tensor, or None with counts_only)."""
    import torch
    lib = load()
    M, Q = pts_dev.shape[0], q_dev.shape[0]
    offs = np.zeros(Q + 1, dtype=np.int64)
    o = options(device_inputs=True, **opt_kw)
    _check(lib.oi_ball_query(_dptr(pts_dev, None), M, _dptr(q_dev, None), Q, float(r),
                             _ptr(offs, ctypes.c_int64), None, 0, ctypes.byref(o)))
    if counts_only:
        return offs, None
    idx = torch.empty(int(offs[-1]), dtype=torch.int64, device=pts_dev.device)
    if idx.numel():
        _check(lib.oi_ball_query(_dptr(pts_dev, None), M, _dptr(q_dev, None), Q, float(r),
                                 _ptr(offs, ctypes.c_int64), _dptr(idx, None, ctypes.c_int64),
                                 idx.numel(), ctypes.byref(o)))
    return offs, idx


def gather_rows(x_train, y_train, t_train, z, idx, **opt_kw):
    """oi_gather_rows on host arrays: returns (xyt [N, 3], z [N])."""
    lib = load()
    cols = [_f64(a) for a in (x_train, y_train, t_train, z)]
    M = len(cols[0])
    if any(len(c) != M for c in cols):
        raise ValueError("training columns differ in length")
    I = np.ascontiguousarray(idx, dtype=np.int64)
    xyt = np.empty((len(I), 3))
    zo = np.empty(len(I))
    _check(lib.oi_gather_rows(*[_ptr(c) for c in cols], M, _ptr(I, ctypes.c_int64), len(I), _ptr(xyt),
                              _ptr(zo), ctypes.byref(options(**opt_kw))))
    return xyt, zo


def gather_rows_device(cols_dev, idx_dev, **opt_kw):
    """oi_gather_rows on HBM-resident tensors: cols_dev = (x, y, t, z) [M] each;
    returns (xyt [N, 3], z [N]) device tensors."""
    import torch
    lib = load()
    M = cols_dev[0].numel()
    N = idx_dev.numel()
    xyt = torch.empty((N, 3), dtype=torch.float64, device=idx_dev.device)
    zo = torch.empty(N, dtype=torch.float64, device=idx_dev.device)
    if N:
        _check(lib.oi_gather_rows(*[_dptr(c, None) for c in cols_dev], M,
                                  _dptr(idx_dev, None, ctypes.c_int64), N, _dptr(xyt, None),
                                  _dptr(zo, None),
                                  ctypes.byref(options(device_inputs=True, **opt_kw))))
    return xyt, zo


def profile_json():
    import json
    lib = load()
    n = lib.oi_profile_json(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib.oi_profile_json(buf, n)
    return json.loads(buf.value.decode())


def profile_reset():
    load().oi_profile_reset()
