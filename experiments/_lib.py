"""ctypes binding of experiments/libcim_exp.so (experiments/include/cim_exp.h): the superseded engines.  Test infrastructure."""
import ctypes
import os

from cim_amd._lib import CimHipError, parse_header, ptr, stream_ptr      # noqa: F401  (same helpers as the product binding)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcim_exp.so")
FUNCTIONS = parse_header(os.path.join(HERE, "include", "cim_exp.h"))[0]         # name -> (restype, argtypes)
SIGNATURES = {name: argtypes for name, (_, argtypes) in FUNCTIONS.items()}
VALUE_RETURNING = {"cim_gemm_f32_splits", "cim_gemm_f16x2_splits"}
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (PyTorch's HIP runtime first, as in cim_amd/_lib.py)
    if not os.path.exists(LIB_PATH):
        from . import build
        build.build()
    lib = ctypes.CDLL(LIB_PATH)
    lib.cim_last_error.restype = ctypes.c_char_p
    for name, (restype, argtypes) in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if name in VALUE_RETURNING:
        return rc
    if rc != 0:
        raise CimHipError("%s failed (rc=%d): %s" % (name, rc, lib.cim_last_error().decode()))
