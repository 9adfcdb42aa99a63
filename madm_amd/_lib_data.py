"""ctypes binding of libmadm_data.so (the C ABI declared in include/madm_data.h): the dataset pipeline's kernels and the
PNG reader's unfilter loop.  Loaded by ``madm_amd/data.py`` and ``madm_amd/png_read.py`` only -- importing the package does
not touch it.  Built in-tree by ``madm_amd/csrc/Makefile``; as with ``_lib.py`` the binding is read from the header
(``_cabi.py``) and there is no fallback: a missing library, header or symbol raises on import."""
import ctypes
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MADM_DATA_LIB") or os.path.join(_HERE, "libmadm_data.so")

ABI = _cabi.parse_packaged("madm_data.h")
_C = ABI.constants
MDATA_OK, MDATA_ERR_INVALID_ARG = _C["MDATA_OK"], _C["MDATA_ERR_INVALID_ARG"]
MDATA_ERR_LAUNCH, MDATA_ERR_FORMAT = _C["MDATA_ERR_LAUNCH"], _C["MDATA_ERR_FORMAT"]
MAX_TAPS = _C["MDATA_MAX_TAPS"]
ABI_VERSION = 1           # what mdata_abi_version() returns: the header states it in a comment, not in a #define

SYMBOLS = ABI.symbols()   # every symbol include/madm_data.h declares: (name, restype, argtypes)


class MadmDataError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or __graft_entry__.build()); the dataset pipeline has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mdata_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {lib.mdata_abi_version()}, this binding is for {ABI_VERSION}: rebuild")
    return lib


lib = _load()


def last_error():
    return lib.mdata_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise MadmDataError(f"{what} failed (status {rc}): {last_error()}")
