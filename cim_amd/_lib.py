"""ctypes binding of libcim_hip.so (include/cim_hip.h).  There is NO fallback: if the HIP
library is missing or a call fails, this raises."""
import ctypes
import os

from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
# CIM_HIP_LIB: an ablation build (python -m cim_amd.build --out=...) for whole-step A/B runs; must export the same ABI
LIB_PATH = os.environ.get("CIM_HIP_LIB") or os.path.join(HERE, "libcim_hip.so")
HEADER = os.path.join(HERE, "..", "include", "cim_hip.h")       # (where cim_amd/build.py finds it)


class CimHipError(RuntimeError):
    pass


def parse_header(path):
    """_abi.parse of a header file: (functions, structs, constants).  A missing header is an error like a missing library."""
    if not os.path.exists(path):
        raise CimHipError("C header %s not found: the ctypes binding is derived from it (there is no second copy of the ABI)" % path)
    with open(path) as f:
        return _abi.parse(f.read())


# The binding IS the header: name -> (restype, argtypes), the `typedef struct`s as ctypes.Structure classes, the integer #defines
FUNCTIONS, STRUCTS, CONSTANTS = parse_header(HEADER)
SIGNATURES = {name: argtypes for name, (_, argtypes) in FUNCTIONS.items() if name not in ("cim_last_error", "cim_abi_version")}

ABI_VERSION = 16         # cim_abi_version() of include/cim_hip.h this binding was written against
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime of this process, so
    # import torch BEFORE dlopen-ing our library (otherwise /opt/rocm's copy is loaded first and
    # the two runtimes do not share devices / streams).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise CimHipError(
            "libcim_hip.so not found at %s - build it with `python -m cim_amd.build` "
            "(there is no CPU fallback for the CIM hot path)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.cim_abi_version.restype, lib.cim_abi_version.argtypes = FUNCTIONS["cim_abi_version"]
    if lib.cim_abi_version() != ABI_VERSION:
        raise CimHipError("%s exports ABI %d, this package binds ABI %d: rebuild with `python -m cim_amd.build`"
                          % (LIB_PATH, lib.cim_abi_version(), ABI_VERSION))
    for name, (restype, argtypes) in FUNCTIONS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


# return a value, not a status: every `long long` entry point (byte counts) and the int entry points that return a count - which
# no C type tells apart from a status, so they are named here (a name missing from this set fails loudly: call() raises on its value)
VALUE_RETURNING = {name for name, (restype, _) in FUNCTIONS.items() if restype is ctypes.c_longlong} | {
    "cim_bn_act_bwd_chunks", "cim_conv3x3_dx_parts", "cim_conv3x3_nchw_splits", "cim_gemm_pair_splits", "cim_gemm_small_splits",
    "cim_maxpool2d_out_size", "cim_segm_words"}


# split counts / workspace sizes of the body's layers: pure functions of their integer arguments (their tuning switches are read
# once per process), asked ~100 times per training step with the step's few dozen layer shapes
PURE = {"cim_maxpool2d_out_size", "cim_conv3x3_dx_parts", "cim_gemm_small_splits", "cim_conv3x3_nchw_splits", "cim_conv1x1_bwd_workspace", "cim_conv3x3_nchw_bwd_workspace",
        "cim_bn_act_bwd_chunks", "cim_gemm_pair_splits", "cim_bn_train_workspace"}
_PURE_VALUES = {}


def call(name, *args):
    if name in PURE:
        key = (name,) + args
        v = _PURE_VALUES.get(key)
        if v is None:
            v = _PURE_VALUES[key] = getattr(load(), name)(*args)
        return v
    lib = load()
    rc = getattr(lib, name)(*args)
    if name in VALUE_RETURNING:
        return rc
    if rc != 0:
        raise CimHipError("%s failed (rc=%d): %s" % (name, rc, lib.cim_last_error().decode()))


def stream_ptr():
    """Raw hipStream_t of the calling thread's current stream on its current device (called ~120 times per training step:
    torch.cuda.current_stream().cuda_stream builds a Stream object through three Python layers, ~9 us; the raw query ~0.3 us)."""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:              # (a torch build without the private query)
        return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a dense tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
