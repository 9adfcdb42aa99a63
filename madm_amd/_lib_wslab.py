"""ctypes binding of libmadm_wslab.so (the C ABI declared in include/madm_wslab.h): the ordered-slab weight gradient of the
deterministic training mode.  Loaded by the first ``ops.conv2d_wgrad`` that takes the slab path only (the mode
``ops.set_deterministic("slabs")`` or an explicit ``slabs=``) -- importing the package or switching the deterministic mode on
does not touch it.  Built in-tree by ``madm_amd/csrc/Makefile``; as with ``_lib.py`` the binding is read from the header
(``_cabi.py``) and there is no fallback: a missing library, header or symbol raises on import."""
import os

from . import _cabi


class MadmWslabError(RuntimeError):
    pass


ABI_VERSION = 1           # what mws_abi_version() returns: the header states it in a comment, not in a #define
_B = _cabi.load(header="madm_wslab.h", libname="libmadm_wslab.so", override=os.environ.get("MADM_WSLAB_LIB"),
                version_fn="mws_abi_version", version=ABI_VERSION, last_error_fn="mws_last_error", error=MadmWslabError,
                no_fallback="the slab weight gradient has no fallback")
ABI, SYMBOLS, LIB_PATH, lib, last_error, check = _B.ABI, _B.SYMBOLS, _B.LIB_PATH, _B.lib, _B.last_error, _B.check
_C = ABI.constants
MWS_OK, MWS_ERR_INVALID_ARG, MWS_ERR_LAUNCH = _C["MWS_OK"], _C["MWS_ERR_INVALID_ARG"], _C["MWS_ERR_LAUNCH"]
MAX_SLICES, TARGET_BLOCKS = _C["MWS_MAX_SLICES"], _C["MWS_TARGET_BLOCKS"]
Conv2dWgradArgs = ABI.struct("mws_conv2d_wgrad_args")
