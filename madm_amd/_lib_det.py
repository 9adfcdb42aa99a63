"""ctypes binding of libmadm_det.so (the C ABI declared in include/madm_det.h): the fixed-order reductions of the
deterministic training mode.  Loaded by the first ``ops.set_deterministic(True)`` only -- importing the package does not touch
it.  Built in-tree by ``madm_amd/csrc/Makefile``; as with ``_lib.py`` the binding is read from the header (``_cabi.py``) and
there is no fallback: a missing library, header or symbol raises on import."""
import os

from . import _cabi


class MadmDetError(RuntimeError):
    pass


ABI_VERSION = 1           # what mdet_abi_version() returns: the header states it in a comment, not in a #define
_B = _cabi.load(header="madm_det.h", libname="libmadm_det.so", override=os.environ.get("MADM_DET_LIB"),
                version_fn="mdet_abi_version", version=ABI_VERSION, last_error_fn="mdet_last_error", error=MadmDetError,
                no_fallback="the deterministic mode has no fallback")
ABI, SYMBOLS, LIB_PATH, lib, last_error, check = _B.ABI, _B.SYMBOLS, _B.LIB_PATH, _B.lib, _B.last_error, _B.check
_C = ABI.constants
MDET_OK, MDET_ERR_INVALID_ARG, MDET_ERR_LAUNCH = _C["MDET_OK"], _C["MDET_ERR_INVALID_ARG"], _C["MDET_ERR_LAUNCH"]
MIN_SLICE_ROWS, MAX_SLICES = _C["MDET_MIN_SLICE_ROWS"], _C["MDET_MAX_SLICES"]
