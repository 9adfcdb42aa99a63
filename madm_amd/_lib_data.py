"""ctypes binding of libmadm_data.so (the C ABI declared in include/madm_data.h): the dataset pipeline's kernels and the
PNG reader's unfilter loop.  Loaded by ``madm_amd/data.py`` and ``madm_amd/png_read.py`` only -- importing the package does
not touch it.  Built in-tree by ``madm_amd/csrc/Makefile``; as with ``_lib.py`` the binding is read from the header
(``_cabi.py``) and there is no fallback: a missing library, header or symbol raises on import."""
import os

from . import _cabi


class MadmDataError(RuntimeError):
    pass


ABI_VERSION = 1           # what mdata_abi_version() returns: the header states it in a comment, not in a #define
_B = _cabi.load(header="madm_data.h", libname="libmadm_data.so", override=os.environ.get("MADM_DATA_LIB"),
                version_fn="mdata_abi_version", version=ABI_VERSION, last_error_fn="mdata_last_error", error=MadmDataError,
                no_fallback="the dataset pipeline has no CPU fallback")
ABI, SYMBOLS, LIB_PATH, lib, last_error, check = _B.ABI, _B.SYMBOLS, _B.LIB_PATH, _B.lib, _B.last_error, _B.check
_C = ABI.constants
MDATA_OK, MDATA_ERR_INVALID_ARG = _C["MDATA_OK"], _C["MDATA_ERR_INVALID_ARG"]
MDATA_ERR_LAUNCH, MDATA_ERR_FORMAT = _C["MDATA_ERR_LAUNCH"], _C["MDATA_ERR_FORMAT"]
MAX_TAPS = _C["MDATA_MAX_TAPS"]
