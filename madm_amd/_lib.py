"""ctypes binding of libmadm_hip.so (the C ABI declared in include/madm_hip.h).

The library is built in-tree by ``madm_amd/csrc/Makefile`` (``__graft_entry__.build()``).  There is
no CPU or PyTorch fallback: if the shared object is missing or does not export a symbol, importing
this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MADM_HIP_LIB") or os.path.join(_HERE, "libmadm_hip.so")   # env override: A/B kernel builds

MADM_F32 = 0
MADM_BF16 = 1
MADM_F16 = 2
EPI_NONE = 0
EPI_GEGLU = 1
EPI_RELU = 2
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t


class Conv2dArgs(ctypes.Structure):
    _fields_ = [
        ("dtype", c_int),
        ("in1", c_void_p), ("in2", c_void_p),
        ("C1", c_int), ("C2", c_int),
        ("ld1", c_int), ("ld2", c_int),
        ("B", c_int), ("IH", c_int), ("IW", c_int),
        ("OH", c_int), ("OW", c_int),
        ("KH", c_int), ("KW", c_int),
        ("stride", c_int),
        ("pad_t", c_int), ("pad_l", c_int),
        ("upsample", c_int),
        ("w", c_void_p),
        ("ldw", c_int),
        ("N", c_int),
        ("bias", c_void_p),
        ("rowvec", c_void_p),
        ("ldrv", c_int),
        ("residual", c_void_p),
        ("ldr", c_int),
        ("out", c_void_p),
        ("ldo", c_int),
        ("out_f32", c_int),
        ("epilogue", c_int),
        ("stats", c_void_p),
        ("gn_sums1", c_void_p), ("gn_sums2", c_void_p), ("gn_gamma", c_void_p), ("gn_beta", c_void_p),
        ("gn_groups", c_int), ("gn_eps", ctypes.c_float), ("gn_act", c_int),
        ("splitk", c_int),
        ("workspace", c_void_p),
        ("workspace_bytes", c_size_t),
        ("ln_colsum", c_void_p), ("ln_eps", ctypes.c_float),
        ("pn_gamma", c_void_p), ("pn_beta", c_void_p), ("pn_groups", c_int), ("pn_eps", ctypes.c_float), ("pn_act", c_int),
    ]


class Conv2dPlan(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("tile", "splitk", "splitk_eff", "post_gn", "tuned_row")] + [("workspace_bytes", c_size_t)]


class Conv2dWgradArgs(ctypes.Structure):
    _fields_ = [
        ("dtype", c_int),
        ("in1", c_void_p), ("in2", c_void_p),
        ("C1", c_int), ("C2", c_int),
        ("ld1", c_int), ("ld2", c_int),
        ("dout", c_void_p), ("ldd", c_int),
        ("dw", c_void_p),
        ("B", c_int), ("IH", c_int), ("IW", c_int), ("OH", c_int), ("OW", c_int),
        ("KH", c_int), ("KW", c_int), ("stride", c_int), ("pad_t", c_int), ("pad_l", c_int), ("upsample", c_int),
        ("N", c_int),
        ("splitm", c_int),
        ("dbias", c_void_p),
    ]


class AttentionArgs(ctypes.Structure):
    _fields_ = [
        ("dtype", c_int),
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("o", c_void_p),
        ("ldq", c_int), ("ldk", c_int), ("ldv", c_int), ("ldo", c_int),
        ("B", c_int), ("H", c_int), ("Lq", c_int), ("Lk", c_int), ("D", c_int),
        ("scale", c_float),
    ]


class AttentionBwdArgs(ctypes.Structure):
    _fields_ = [
        ("dtype", c_int),
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("o", c_void_p), ("dout", c_void_p),
        ("dq", c_void_p), ("dk", c_void_p), ("dv", c_void_p),
        ("ldq", c_int), ("ldk", c_int), ("ldv", c_int), ("ldo", c_int), ("lddo", c_int),
        ("lddq", c_int), ("lddk", c_int), ("lddv", c_int),
        ("B", c_int), ("H", c_int), ("Lq", c_int), ("Lk", c_int), ("D", c_int),
        ("scale", c_float),
        ("workspace", c_void_p),
        ("workspace_bytes", c_size_t),
    ]


VIS_IMAGE, VIS_LABEL, VIS_LOGITS, VIS_HEAT = 0, 1, 2, 3
VIS_MAX_TILES = 16
EXPORT_IMAGE_F32, EXPORT_IMAGE_U8 = 0, 1


class VisTile(ctypes.Structure):
    _fields_ = [("kind", c_int), ("src", c_void_p), ("C", c_int), ("h", c_int), ("w", c_int), ("p0", c_float), ("p1", c_float)]


# every symbol include/madm_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("madm_abi_version", c_int, []),
    ("madm_last_error", ctypes.c_char_p, []),
    ("madm_calib_mfma_loop", c_int, [c_int, c_int, c_void_p, ctypes.POINTER(ctypes.c_double), c_void_p]),
    ("madm_conv2d_make_plan", c_int, [ctypes.POINTER(Conv2dArgs), ctypes.POINTER(Conv2dPlan)]),
    ("madm_conv2d_tile_name", ctypes.c_char_p, [c_int]),
    ("madm_set_tuning_profile", c_int, [c_int]),
    ("madm_get_tuning_profile", c_int, []),
    ("madm_conv2d_can_fuse_groupnorm", c_int, [ctypes.POINTER(Conv2dArgs)]),
    ("madm_groupnorm_finalize", c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                        c_float, c_void_p, c_void_p, c_void_p]),
    ("madm_conv2d_fwd", c_int, [ctypes.POINTER(Conv2dArgs), c_void_p]),
    ("madm_debug_set_conv_tile", None, [c_int]),
    ("madm_debug_poison_lds", c_int, [ctypes.c_uint, c_void_p, c_void_p]),
    ("madm_groupnorm_stats", c_int, [c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("madm_groupnorm_apply", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_int,
                                     c_void_p]),
    ("madm_groupnorm_apply_cat", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    ("madm_layernorm_fwd", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_float,
                                   c_void_p]),
    ("madm_softmax_rows", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    ("madm_attention_fwd", c_int, [ctypes.POINTER(AttentionArgs), c_void_p]),
    ("madm_image_to_nhwc", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                   c_float, c_void_p, c_void_p]),
    ("madm_stem_conv3x3", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                  c_float, c_void_p, c_void_p, c_void_p]),
    ("madm_image_to_im2col3x3", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                        c_void_p, c_void_p]),
    ("madm_latents_add_noise", c_int, [c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    ("madm_timestep_embedding", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    ("madm_silu", c_int, [c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_rows_to_f32", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_copy_columns", c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_size_t, c_int, c_void_p]),
    ("madm_clamp_f32", c_int, [c_void_p, c_void_p, c_size_t, c_float, c_float, c_void_p]),
    ("madm_cast_from_f32", c_int, [c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_nhwc_to_nchw_f32", c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p]),
    ("madm_resize_bilinear", c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p]),
    ("madm_resize_bilinear_nchw_f32", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    ("madm_scale_pad_crop_nchw_f32", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                             c_void_p]),
    ("madm_slide_merge", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("madm_confusion_matrix", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p, c_void_p]),
    ("madm_dwconv3x3", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_void_p]),
    ("madm_tanh_gate", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    ("madm_argmax_nchw_f32", c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_void_p]),
    ("madm_sumsq_f32", c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    ("madm_adamw_step", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float, c_float,
                                c_int, c_float, c_void_p]),
    ("madm_adamw_step_table", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_float, c_float,
                                      c_float, c_float, c_void_p]),
    ("madm_ema_update", c_int, [c_void_p, c_void_p, c_size_t, c_float, c_void_p]),
    ("madm_snapshot_f32", c_int, [c_void_p, c_void_p, c_size_t, ctypes.c_ulonglong, c_void_p, c_void_p]),
    ("madm_label_to_rgb", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    ("madm_pseudo_label", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    ("madm_label_presence", c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    ("madm_class_mix", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    ("madm_nchw_f32_to_nhwc", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    ("madm_conv2d_wgrad", c_int, [ctypes.POINTER(Conv2dWgradArgs), c_void_p]),
    ("madm_pack_dgrad_weights", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    ("madm_pack_weight", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int,
                                 c_int, c_void_p]),
    ("madm_fold_layernorm_pack", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                         c_int, c_int, c_void_p]),
    ("madm_attention_bwd_workspace_bytes", c_size_t, [ctypes.POINTER(AttentionBwdArgs)]),
    ("madm_attention_bwd", c_int, [ctypes.POINTER(AttentionBwdArgs), c_void_p]),
    ("madm_zero_insert2x", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    ("madm_sumpool2x2", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    ("madm_silu_bwd", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_add", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_colsum", c_int, [c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("madm_groupnorm_bwd_sums", c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]),
    ("madm_groupnorm_bwd_apply", c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    ("madm_layernorm_bwd", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    ("madm_geglu_bwd", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    ("madm_scale_channels", c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    ("madm_bn_fold_stats", c_int, [c_void_p, c_int, c_int, ctypes.c_double, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("madm_relu_bwd", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_dwconv3x3_wgrad", c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p]),
    ("madm_resize_bilinear_bwd_workspace_bytes", c_size_t, [c_int, c_int, c_int, c_int]),
    ("madm_resize_bilinear_bwd", c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_size_t, c_void_p]),
    ("madm_softmax_ce", c_int, [c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p,
                                c_float, c_void_p, c_int, c_void_p]),
    ("madm_masked_l1", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                               c_void_p, c_float, c_void_p, c_void_p]),
    ("madm_gray_sum", c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    ("madm_color_jitter_step", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("madm_blur_axis_f32", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("madm_mic_minmax_parts", c_int, [c_size_t]),
    ("madm_mic_minmax", c_int, [c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    ("madm_block_mask", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_float,
                                c_float, c_void_p, c_int, c_void_p, c_void_p]),
    ("madm_tanh_gate_bwd", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_size_t, c_int, c_void_p]),
    ("madm_token_embedding", c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("madm_causal_attention_fwd", c_int, [ctypes.POINTER(AttentionArgs), c_void_p]),
    ("madm_quick_gelu", c_int, [c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("madm_vis_compose", c_int, [ctypes.POINTER(VisTile), c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("madm_eval_export_pack", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p]),
]


class MadmHipError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or __graft_entry__.build()); madm_amd has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


lib = _load()


class _PoisonedLib:
    """Debug harness (MADM_DEBUG_POISON_LDS=1; tests/test_poison_gpu.py drives it): every launch
    through the C ABI is preceded, on the same stream, by madm_debug_poison_lds -- all LDS of the chip holds quiet NaNs when
    the kernel starts.  A kernel that reads LDS it did not write then fails its parity test deterministically; without the
    harness such a read returns whatever the previous kernel on that CU left there (a dependence on history)."""

    def __init__(self, raw):
        object.__setattr__(self, "_raw", raw)
        object.__setattr__(self, "_sink", None)
        object.__setattr__(self, "_launching", {n for n, _r, a in SYMBOLS if a and a[-1] is c_void_p and n.startswith("madm_")
                                                and not n.startswith("madm_debug")})

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


def check(rc, what):
    if rc != 0:
        msg = lib.madm_last_error().decode("utf-8", "replace")
        raise MadmHipError(f"{what} failed (status {rc}): {msg}")
