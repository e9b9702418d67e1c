"""The one reader of include/oi.h for the ABI tests: its text without comments,
its prototypes, and the ctypes type of a C type as the header spells it."""
import ctypes
import os
import re

from optimalinterpolation_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'oi.h')


def source():
    """include/oi.h without its comments."""
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S))


def protos():
    """(return type, name, [argument types]) of every prototype, in the header's order."""
    found = re.findall(r'([A-Za-z_][\w\s\*]*?)\b(oi_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', source())
    out = []
    for ret, name, args in found:
        args = [a.strip() for a in args.split(',')] if args.strip() not in ('', 'void') else []
        out.append((ret.strip(), name, [re.match(r'(.*?)\w+$', a).group(1) for a in args]))
    return out


def nargs(name):
    """The number of arguments the header declares for ``name``."""
    return {n: len(a) for _, n, a in protos()}[name]


def _ctype(decl):
    """The ctypes type of a C type as include/oi.h spells it."""
    t = re.sub(r'\s+', ' ', re.sub(r'\bconst\b', '', decl)).strip().replace(' *', '*')
    scalar = {'double': ctypes.c_double, 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32,
              'uint64_t': ctypes.c_uint64, 'int': ctypes.c_int}
    if t in scalar:
        return scalar[t]
    if t.endswith('*') and t[:-1] in scalar:
        return ctypes.POINTER(scalar[t[:-1]])
    if t in ('void', 'void*', 'char*'):
        return {'void': None, 'void*': ctypes.c_void_p, 'char*': ctypes.c_char_p}[t]
    if t == 'oi_options*':
        return ctypes.POINTER(_lib.OiOptions)
    assert re.fullmatch(r'(struct )?oi_\w+\*', t), f"unmapped C type {decl!r}"
    return ctypes.c_void_p    # an opaque handle


def exported():
    """The oi_* symbols the built library defines (nm -D)."""
    import subprocess
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r'\b[TW] (oi_\w+)', out))
