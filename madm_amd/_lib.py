"""ctypes binding of libmadm_hip.so (the C ABI declared in include/madm_hip.h).

The library is built in-tree by ``madm_amd/csrc/Makefile`` (``__graft_entry__.build()``).  Structures, signatures and
constants are read from the header by ``_cabi.py``; the names below only bind them.  There is no CPU or PyTorch fallback:
if the shared object or the header is missing, a declared symbol is not exported, or the library was built for another
ABI version, importing this module raises.
"""
import os

from . import _cabi


class MadmHipError(RuntimeError):
    pass


_B = _cabi.load(header="madm_hip.h", libname="libmadm_hip.so", override=os.environ.get("MADM_HIP_LIB"),   # A/B kernel builds
                version_fn="madm_abi_version", version="MADM_ABI_VERSION", version_from="include/madm_hip.h declares",
                last_error_fn="madm_last_error", error=MadmHipError, no_fallback="madm_amd has no CPU fallback")
ABI, SYMBOLS, LIB_PATH, lib, last_error, check = _B.ABI, _B.SYMBOLS, _B.LIB_PATH, _B.lib, _B.last_error, _B.check
_C = ABI.constants

MADM_F32, MADM_BF16, MADM_F16 = _C["MADM_F32"], _C["MADM_BF16"], _C["MADM_F16"]
EPI_NONE, EPI_GEGLU, EPI_RELU = _C["MADM_EPI_NONE"], _C["MADM_EPI_GEGLU"], _C["MADM_EPI_RELU"]
ACT_NONE, ACT_SILU, ACT_RELU = _C["MADM_ACT_NONE"], _C["MADM_ACT_SILU"], _C["MADM_ACT_RELU"]
VIS_IMAGE, VIS_LABEL, VIS_LOGITS, VIS_HEAT = _C["MADM_VIS_IMAGE"], _C["MADM_VIS_LABEL"], _C["MADM_VIS_LOGITS"], _C["MADM_VIS_HEAT"]
VIS_MAX_TILES = _C["MADM_VIS_MAX_TILES"]
EXPORT_IMAGE_F32, EXPORT_IMAGE_U8 = _C["MADM_EXPORT_IMAGE_F32"], _C["MADM_EXPORT_IMAGE_U8"]

Conv2dArgs = ABI.struct("madm_conv2d_args")
Conv2dPlan = ABI.struct("madm_conv2d_plan")
Conv2dWgradArgs = ABI.struct("madm_conv2d_wgrad_args")
AttentionArgs = ABI.struct("madm_attention_args")
AttentionBwdArgs = ABI.struct("madm_attention_bwd_args")
VisTile = ABI.struct("madm_vis_tile")


class _PoisonedLib:
    """Debug harness (MADM_DEBUG_POISON_LDS=1; tests/test_poison_gpu.py drives it): every launch
    through the C ABI is preceded, on the same stream, by madm_debug_poison_lds -- all LDS of the chip holds quiet NaNs when
    the kernel starts.  A kernel that reads LDS it did not write then fails its parity test deterministically; without the
    harness such a read returns whatever the previous kernel on that CU left there (a dependence on history)."""

    def __init__(self, raw):
        object.__setattr__(self, "_raw", raw)
        object.__setattr__(self, "_sink", None)
        object.__setattr__(self, "_launching", {n for n, _r, params in ABI.prototypes
                                                if params and params[-1][0] == "stream" and not n.startswith("madm_debug")})

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        if name not in self._launching:
            return fn

        def call(*args):
            import torch
            if self._sink is None:
                object.__setattr__(self, "_sink", torch.zeros(1, dtype=torch.int32, device="cuda"))
            self._raw.madm_debug_poison_lds(0x7fc00000, self._sink.data_ptr(), args[-1])
            return fn(*args)
        return call


if int(os.environ.get("MADM_DEBUG_POISON_LDS", "0")):
    lib = _PoisonedLib(lib)

