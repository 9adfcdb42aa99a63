"""ctypes binding of libmadm_headfuse.so (the C ABI declared in include/madm_headfuse.h): upsample + concat + classifier of
``DAFormerHead(final_fuse_vae_decoder_feat=True)`` in one pass.  Loaded by the first flagged head that takes the fused route
(``ops.upsample_cat_classify``) only -- importing the package does not touch it.  Built in-tree by ``madm_amd/csrc/Makefile``; as
with ``_lib.py`` the binding is read from the header (``_cabi.py``) and there is no fallback: a missing library, header or
symbol raises on import."""
import ctypes
import os

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MADM_HEADFUSE_LIB") or os.path.join(_HERE, "libmadm_headfuse.so")

ABI = _cabi.parse_packaged("madm_headfuse.h")
_C = ABI.constants
MHF_OK, MHF_ERR_INVALID_ARG, MHF_ERR_LAUNCH = _C["MHF_OK"], _C["MHF_ERR_INVALID_ARG"], _C["MHF_ERR_LAUNCH"]
TILE_H, TILE_W = _C["MHF_TILE_H"], _C["MHF_TILE_W"]
MAX_ROW_BYTES, MAX_CLASSES = _C["MHF_MAX_ROW_BYTES"], _C["MHF_MAX_CLASSES"]
ABI_VERSION = 1           # what mhf_abi_version() returns: the header states it in a comment, not in a #define

SYMBOLS = ABI.symbols()   # every symbol include/madm_headfuse.h declares: (name, restype, argtypes)


class MadmHeadfuseError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or __graft_entry__.build()); the fused classifier has no fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mhf_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {lib.mhf_abi_version()}, this binding is for {ABI_VERSION}: rebuild")
    return lib


lib = _load()


def last_error():
    return lib.mhf_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise MadmHeadfuseError(f"{what} failed (status {rc}): {last_error()}")
