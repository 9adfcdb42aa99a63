"""Host tests of the canary helper (tests/window_util.py) -- its negative control: no kernel is made to misbehave, the
buffers are clobbered by hand on the CPU -- and of the table that says which test covers which entry point."""
import pytest
import torch

from window_util import Guarded, PATTERN, guarded_flat

ALL_DTYPES = list(PATTERN)


def _g(dtype, **kw):
    return Guarded(5, 8, dtype, ld=24, c0=8, pre=4, post=4, device="cpu", **kw)


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=[str(d).split(".")[1] for d in ALL_DTYPES])
def test_untouched_buffer_passes_and_the_window_may_hold_anything(dtype):
    g = _g(dtype)
    g.check()
    if dtype.is_floating_point:
        assert bool(torch.isnan(g.buf.double()).all())          # the pattern is a NaN in every floating type
    g.load(torch.arange(40).reshape(5, 8))
    g.check()
    g.view.zero_()
    g.check()
    if dtype.is_floating_point:
        g.view.fill_(float("nan"))
        g.check()
    assert g.view.shape == (5, 8) and g.view.stride() == (24, 1)
    assert g.view.data_ptr() == g.buf.data_ptr() + (4 * 24 + 8) * g.buf.element_size()


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=[str(d).split(".")[1] for d in ALL_DTYPES])
@pytest.mark.parametrize("where", [("rows before", 3, 9), ("rows before", 0, 0), ("rows after", 9, 9), ("rows after", 12, 23),
                                   ("columns left", 4, 7), ("columns left", 8, 0), ("columns right", 4, 16),
                                   ("columns right", 8, 23)],
                         ids=lambda w: f"{w[0].replace(' ', '_')}_{w[1]}_{w[2]}")
def test_one_clobbered_element_is_reported_with_its_region(dtype, where):
    region, r, c = where
    g = _g(dtype)
    g.buf[r, c] = 0          # a stray store of zeros: what a zero canary cannot see
    hit = g.clobbered()
    assert hit is not None and hit[0] == region and hit[1] == r - 4 and hit[2] == c - 8 and hit[3] == 0, hit
    with pytest.raises(AssertionError, match=region):
        g.check("probe")


@pytest.mark.parametrize("dtype", [d for d in ALL_DTYPES if d.is_floating_point],
                         ids=[str(d).split(".")[1] for d in ALL_DTYPES if d.is_floating_point])
def test_a_nan_with_another_payload_counts_as_clobbered(dtype):
    g = _g(dtype)
    g.buf[10, 3] = float("nan")          # torch's own NaN: still a NaN, another bit pattern
    assert bool(torch.isnan(g.buf.double()).all())
    hit = g.clobbered()
    assert hit is not None and hit[0] == "rows after" and hit[1:3] == (6, -5) and hit[3] != g.pattern


def test_the_first_offender_is_named():
    g = _g(torch.float32)
    g.buf[6, 20] = 1.0
    g.buf[5, 19] = 1.0
    g.buf[11, 0] = 1.0
    assert g.clobbered()[:3] == ("rows after", 7, -8)       # regions in order: before, after, left, right
    g = _g(torch.float32)
    g.buf[6, 20] = 1.0
    g.buf[5, 19] = 1.0
    assert g.clobbered()[:3] == ("columns right", 1, 11)


def test_flat_buffers_start_their_canary_at_element_n():
    g = guarded_flat(1001, torch.float32, pre=16, post=16, device="cpu")
    assert g.flat.numel() == 1001 and g.flat.is_contiguous()
    g.flat.zero_()
    g.check()
    g.buf.view(-1)[16 + 1001] = 0.0
    assert g.clobbered()[:3] == ("columns right", 0, 1001)
    g = guarded_flat(7, torch.uint8, pre=16, post=16, device="cpu")
    g.buf.view(-1)[15] = 0
    assert g.clobbered()[:3] == ("columns left", 0, -1)


def _header_symbols():
    from madm_amd import _cabi
    return {name for name, _restype, _params in _cabi.parse_packaged("madm_hip.h").prototypes}


def test_every_entry_point_is_covered_by_a_window_test_or_exempt_with_a_reason():
    """A new entry point fails here until someone decides whether it gets a strided-window / write-containment test
    (COVERED: symbol -> test in test_windows_gpu.py) or needs none (EXEMPT: symbol -> reason)."""
    import test_windows_gpu as tw
    syms = _header_symbols()
    assert len(syms) > 80, len(syms)
    both = set(tw.COVERED) & set(tw.EXEMPT)
    assert not both, f"in both tables: {sorted(both)}"
    listed = set(tw.COVERED) | set(tw.EXEMPT)
    assert not (syms - listed), f"neither covered nor exempt: {sorted(syms - listed)}"
    assert not (listed - syms), f"not in the header: {sorted(listed - syms)}"
    for sym, test in tw.COVERED.items():
        assert callable(getattr(tw, test, None)) and test.startswith("test_"), (sym, test)
    for sym, reason in tw.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 3, (sym, reason)


# ---- pointer alignment: refused by the entry points before anything is launched (include/madm_hip.h states it per field)
def _aligned_buffer():
    import ctypes
    buf = ctypes.create_string_buffer(1024)
    return buf, (ctypes.addressof(buf) + 63) & ~63


def _conv_args(p):
    from madm_amd._lib import Conv2dArgs
    a = Conv2dArgs()
    a.dtype = 1
    a.in1 = a.w = a.out = p
    a.C1, a.B, a.IH, a.IW, a.OH, a.OW, a.KH, a.KW, a.stride, a.N, a.ldo, a.splitk = 64, 1, 1, 1, 1, 1, 1, 1, 1, 8, 8, 1
    return a


def test_conv2d_refuses_misaligned_pointers_without_gpu():
    """Every pointer of madm_conv2d_args outside its documented alignment is refused (-1, nothing launched) with a message
    naming it.  (Only refusals are exercised here: accepted arguments would launch; the windows of test_windows_gpu.py --
    8-byte aligned 16-bit outputs, 4-byte aligned GEGLU outputs -- are the accepted side.)"""
    import ctypes
    from madm_amd._lib import lib
    keep, p = _aligned_buffer()
    cases = [("in1", 8, b"in1 / in2 / w"), ("w", 2, b"in1 / in2 / w"), ("in2", 8, b"in1 / in2 / w"), ("bias", 4, b"bias"),
             ("rowvec", 8, b"rowvec"), ("ln_colsum", 4, b"ln_colsum"), ("gn_gamma", 4, b"gn_"), ("pn_beta", 8, b"pn_"),
             ("workspace", 8, b"workspace"), ("stats", 4, b"statistics"), ("gn_sums2", 4, b"statistics"),
             ("out", 4, b"out must be aligned to 8"), ("residual", 4, b"residual")]
    for field, off, msg in cases:
        a = _conv_args(p)
        if field == "in2":
            a.C2 = 64
        if field == "rowvec":
            a.ldrv = 8
        if field == "residual":
            a.ldr = 8
        if field == "ln_colsum":
            a.ln_eps = 1e-5
        setattr(a, field, p + off)
        assert lib.madm_conv2d_fwd(ctypes.byref(a), None) == -1, field
        assert msg in lib.madm_last_error(), (field, lib.madm_last_error())
    a = _conv_args(p)
    a.residual, a.ldr = p, 10               # ldr: a multiple of 4 elements outside GEGLU
    assert lib.madm_conv2d_fwd(ctypes.byref(a), None) == -1 and b"ldr" in lib.madm_last_error()
    a = _conv_args(p)
    a.dtype, a.C1, a.out = 0, 32, p + 8     # f32 output: 16 bytes
    assert lib.madm_conv2d_fwd(ctypes.byref(a), None) == -1 and b"aligned to 16" in lib.madm_last_error()
    a = _conv_args(p)
    a.out_f32, a.out = 1, p + 8
    assert lib.madm_conv2d_fwd(ctypes.byref(a), None) == -1 and b"aligned to 16" in lib.madm_last_error()
    a = _conv_args(p)
    a.epilogue, a.out, a.ldo = 1, p + 2, 4     # GEGLU: N / 2 columns stored in pairs
    assert lib.madm_conv2d_fwd(ctypes.byref(a), None) == -1 and b"aligned to 4" in lib.madm_last_error()


def test_gradient_and_attention_entry_points_refuse_misaligned_pointers_without_gpu():
    import ctypes
    from madm_amd._lib import lib, Conv2dWgradArgs, AttentionArgs, AttentionBwdArgs
    keep, p = _aligned_buffer()

    def wg():
        a = Conv2dWgradArgs()
        a.in1 = a.dout = a.dw = p
        a.dtype, a.C1, a.N = 1, 16, 8
        a.B = a.IH = a.IW = a.OH = a.OW = a.KH = a.KW = a.stride = 1
        return a
    for field, off, msg in (("in1", 8, b"in1 / in2"), ("in2", 8, b"in1 / in2"), ("dout", 4, b"dout"), ("dw", 2, b"dw / dbias"),
                            ("dbias", 2, b"dw / dbias")):
        a = wg()
        if field == "in2":
            a.C2 = 16
        setattr(a, field, p + off)
        assert lib.madm_conv2d_wgrad(ctypes.byref(a), None) == -1 and msg in lib.madm_last_error(), field

    def at(cls):
        a = cls()
        for f, _t in cls._fields_:
            if _t is ctypes.c_void_p:
                setattr(a, f, p)
        a.dtype, a.B, a.H, a.Lq, a.Lk, a.D, a.scale = 1, 1, 2, 4, 4, 40, 1.0
        for f, _t in cls._fields_:
            if f.startswith("ld"):
                setattr(a, f, 80)
        return a
    for field, off in (("q", 8), ("k", 8), ("v", 8), ("o", 4)):
        a = at(AttentionArgs)
        setattr(a, field, p + off)
        assert lib.madm_attention_fwd(ctypes.byref(a), None) == -1 and b"aligned" in lib.madm_last_error(), field
    for field, off in (("q", 8), ("k", 8), ("v", 8), ("o", 8), ("dout", 8), ("dq", 4), ("dk", 4), ("dv", 4), ("workspace", 2)):
        a = at(AttentionBwdArgs)
        a.workspace_bytes = 1024
        setattr(a, field, p + off)
        assert lib.madm_attention_bwd(ctypes.byref(a), None) == -1 and b"aligned" in lib.madm_last_error(), field


def test_chunked_entry_points_refuse_misaligned_tensors_without_gpu():
    """The norm / spatial / gradient entry points that address tensors in 16-byte chunks: one misaligned tensor each."""
    from madm_amd._lib import lib
    keep, p = _aligned_buffer()
    q = p + 8
    calls = [
        lambda: lib.madm_groupnorm_stats(1, q, 1, 1, 8, p, None),
        lambda: lib.madm_groupnorm_apply(1, p, q, 8, 1, 1, 8, 0, 8, 1, p, 8, None, p, p, 1e-5, 0, None, 0, None),
        lambda: lib.madm_groupnorm_apply(1, p, p, 8, 1, 1, 8, 0, 8, 1, p, 8, None, p, p, 1e-5, 0, q, 8, None),
        lambda: lib.madm_groupnorm_apply_cat(1, p, q, p, 16, 1, 1, 8, 8, 1, p, p, p, p, 1e-5, 0, None),
        lambda: lib.madm_groupnorm_bwd_sums(1, p, q, 8, 1, 1, 8, 0, 8, 1, p, 8, None, p, p, 1e-5, 0, p, None),
        lambda: lib.madm_groupnorm_bwd_apply(1, p, p, 8, q, 1, 1, 8, 0, 8, 1, p, 8, None, p, p, 1e-5, 0, p, None, None, None, 0, None),
        lambda: lib.madm_layernorm_fwd(1, p, q, 1, 8, p, p, 1e-5, None),
        lambda: lib.madm_layernorm_bwd(1, p, p, p, 1, 8, p, 1e-5, None, None, q, None),
        lambda: lib.madm_softmax_rows(1, p + 4, p, 1, 4, 4, 4, 1.0, None),
        lambda: lib.madm_softmax_rows(1, p, p + 4, 1, 4, 4, 4, 1.0, None),
        lambda: lib.madm_resize_bilinear(1, p, 8, q, 8, 1, 1, 1, 1, 1, 8, None),
        lambda: lib.madm_dwconv3x3(1, q, p, p, p, p, 8, 1, 1, 1, 8, 1, 0, None),
        lambda: lib.madm_scale_channels(1, p, 8, p, q, 8, 1, 1, 8, None),
        lambda: lib.madm_relu_bwd(1, p, q, p, 8, None),
        lambda: lib.madm_dwconv3x3_wgrad(1, p, q, 8, p, 1, 1, 1, 8, 1, None),
        lambda: lib.madm_resize_bilinear_bwd(1, q, 8, p, 1, 1, 1, 1, 1, 8, p, 64, None),
        lambda: lib.madm_zero_insert2x(1, p, q, 1, 1, 1, 1, 1, 8, None),
        lambda: lib.madm_sumpool2x2(1, q, p, 1, 1, 1, 8, None),
        lambda: lib.madm_colsum(1, q, 8, 1, 1, 8, p, None),
        lambda: lib.madm_add(1, p, p, q, 8, None),
        lambda: lib.madm_stem_conv3x3(1, p, p, p, q, 128, 1, 1, 1, 128, 0.5, 0.5, None, None, None),
        lambda: lib.madm_stem_conv3x3(1, p + 4, p, p, p, 128, 1, 1, 1, 128, 0.5, 0.5, None, p, None),      # img under the range probe
        lambda: lib.madm_geglu_bwd(1, q, p, p, 1, 8, None),
        lambda: lib.madm_geglu_bwd(1, p, q, p, 1, 8, None),
        lambda: lib.madm_geglu_bwd(1, p, p, q, 1, 8, None),
        lambda: lib.madm_dwconv3x3(1, p, p + 4, p, p, p, 8, 1, 1, 1, 8, 1, 0, None),                       # w / scale / shift: float4
        lambda: lib.madm_dwconv3x3(1, p, p, q, p, p, 8, 1, 1, 1, 8, 1, 0, None),
        lambda: lib.madm_dwconv3x3(1, p, p, p, p + 4, p, 8, 1, 1, 1, 8, 1, 0, None),
        lambda: lib.madm_image_to_nhwc(1, p, q, 1, 3, 1, 1, 8, 0.5, 0.5, None, None),
        lambda: lib.madm_image_to_nhwc(1, p + 4, p, 1, 3, 1, 1, 8, 0.5, 0.5, p, None),
        lambda: lib.madm_image_to_im2col3x3(1, p, q, 1, 1, 1, 32, 0.5, 0.5, None, None),
        lambda: lib.madm_image_to_im2col3x3(1, p + 4, p, 1, 1, 1, 32, 0.5, 0.5, p, None),
        lambda: lib.madm_nchw_f32_to_nhwc(1, p, q, 1, 3, 1, 8, None),
        lambda: lib.madm_latents_add_noise(1, p, 8, 0.18215, p, p, p, p, None, q, 1, 1, 8, None),
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert b"aligned" in lib.madm_last_error(), (i, lib.madm_last_error())
