"""What the fifteen ctypes bindings share: where a library lies, how it is opened and checked, and how a return code
becomes an exception.  No fallback anywhere: a missing or stale library is an ImportError."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path(env, soname):
    """the library $<env> names, else lib/<soname> of the package"""
    return os.environ.get(env) or os.path.join(_HERE, "lib", soname)


def load(soname, path, prefix, abi, signatures):
    """Open the library at `path` and bind it.  signatures: {symbol: (argtypes or None, restype)} for everything but
    <prefix>_version and <prefix>_last_error.  -> the ctypes.CDLL"""
    if not os.path.exists(path):
        raise ImportError(
            "%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`python -m aquaticgymenv_amd.build` (needs hipcc); there is no CPU fallback" % soname)
    # torch ships its own libamdhip64 (soname libamdhip64.so.7, requested as "libamdhip64.so"); loading it
    # FIRST makes the dynamic loader satisfy our NEEDED libamdhip64.so.7 with that same runtime.  In the
    # other order two HIP runtimes end up in the process and the second one finds no device.
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    version = getattr(lib, prefix + "_version")
    version.restype = ctypes.c_int
    getattr(lib, prefix + "_last_error").restype = ctypes.c_char_p
    for symbol, (argtypes, restype) in signatures.items():
        fn = getattr(lib, symbol)
        if argtypes is not None:
            fn.argtypes = argtypes
        fn.restype = restype
    if version() != abi:
        raise ImportError("%s ABI %d != binding %d: rebuild" % (soname, version(), abi))
    return lib


def checker(lib, prefix, error):
    """-> check(rc, what): nothing for 0, ValueError for E_INVALID (-1), `error` for every other code"""
    last_error = getattr(lib, prefix + "_last_error")

    def check(rc, what):
        if rc != 0:
            msg = last_error().decode("utf-8", "replace")
            if rc == -1:
                raise ValueError("%s: %s" % (what, msg))
            raise error("%s failed (code %d): %s" % (what, rc, msg))
    return check
