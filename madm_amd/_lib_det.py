"""ctypes binding of libmadm_det.so (the C ABI declared in include/madm_det.h): the fixed-order reductions of the
deterministic training mode.  Loaded by the first ``ops.set_deterministic(True)`` only -- importing the package does not touch
it.  Built in-tree by ``madm_amd/csrc/Makefile``; as with ``_lib.py`` the binding is read from the header (``_cabi.py``) and
there is no fallback: a missing library, header or symbol raises on import."""
import ctypes
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MADM_DET_LIB") or os.path.join(_HERE, "libmadm_det.so")

ABI = _cabi.parse_packaged("madm_det.h")
_C = ABI.constants
MDET_OK, MDET_ERR_INVALID_ARG, MDET_ERR_LAUNCH = _C["MDET_OK"], _C["MDET_ERR_INVALID_ARG"], _C["MDET_ERR_LAUNCH"]
MIN_SLICE_ROWS, MAX_SLICES = _C["MDET_MIN_SLICE_ROWS"], _C["MDET_MAX_SLICES"]
ABI_VERSION = 1           # what mdet_abi_version() returns: the header states it in a comment, not in a #define

SYMBOLS = ABI.symbols()   # every symbol include/madm_det.h declares: (name, restype, argtypes)


class MadmDetError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or __graft_entry__.build()); the deterministic mode has no fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mdet_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {lib.mdet_abi_version()}, this binding is for {ABI_VERSION}: rebuild")
    return lib


lib = _load()


def last_error():
    return lib.mdet_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise MadmDetError(f"{what} failed (status {rc}): {last_error()}")
