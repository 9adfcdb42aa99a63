"""ctypes binding of libmadm_headfuse.so (the C ABI declared in include/madm_headfuse.h): upsample + concat + classifier of
``DAFormerHead(final_fuse_vae_decoder_feat=True)`` in one pass.  Loaded by the first flagged head that takes the fused route
(``ops.upsample_cat_classify``) only -- importing the package does not touch it.  Built in-tree by ``madm_amd/csrc/Makefile``; as
with ``_lib.py`` the binding is read from the header (``_cabi.py``) and there is no fallback: a missing library, header or
symbol raises on import."""
import os

from . import _cabi


class MadmHeadfuseError(RuntimeError):
    pass


ABI_VERSION = 1           # what mhf_abi_version() returns: the header states it in a comment, not in a #define
_B = _cabi.load(header="madm_headfuse.h", libname="libmadm_headfuse.so", override=os.environ.get("MADM_HEADFUSE_LIB"),
                version_fn="mhf_abi_version", version=ABI_VERSION, last_error_fn="mhf_last_error", error=MadmHeadfuseError,
                no_fallback="the fused classifier has no fallback")
ABI, SYMBOLS, LIB_PATH, lib, last_error, check = _B.ABI, _B.SYMBOLS, _B.LIB_PATH, _B.lib, _B.last_error, _B.check
_C = ABI.constants
MHF_OK, MHF_ERR_INVALID_ARG, MHF_ERR_LAUNCH = _C["MHF_OK"], _C["MHF_ERR_INVALID_ARG"], _C["MHF_ERR_LAUNCH"]
TILE_H, TILE_W = _C["MHF_TILE_H"], _C["MHF_TILE_W"]
MAX_ROW_BYTES, MAX_CLASSES = _C["MHF_MAX_ROW_BYTES"], _C["MHF_MAX_CLASSES"]
