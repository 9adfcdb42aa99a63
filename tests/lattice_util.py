"""Integer-lattice data and exact references for the conv / linear / gradient GEMM kernels (host-only torch code).

Products of small integers are exact in the MFMA's f32 accumulator, integer sums are exact below 2^24, and the epilogues
add bias, time row and residual in f32 and round once.  On integer inputs an output therefore has ONE correct bit pattern,
whatever the tile, the split, the summation order or the atomics: the tests built on this file assert equality, not a
tolerance, and see a single dropped, duplicated or misplaced product.

Two kinds of data:

* exact mode: both GEMM operands are +-1 at density min(1/2, sqrt(100 / Kred)), 0 elsewhere (Kred = the reduction length
  of the launch: KH KW sum(Cin) of a forward or data-gradient launch -- the data gradient is the forward kernel run on dout,
  whose input channels are the conv's Cout -- and B OH OW of the weight gradient); bias, time row and residual / skip are dense integers in [-2, 2].  Every
  output is a small integer that the 16-bit formats represent, and every f32 partial sum of values or squares a kernel can
  form is exact (check_reference asserts both on the reference itself).
* rounding mode: dense operands of amplitude 4 (bf16) / 16 (f16): outputs leave the format's integer range, many of them
  on exact ties, and the expected result is ONE round-to-nearest-even of the exact integer.

References are the torch statements of tests/test_ops_gpu.py (cat, nearest upsample, F.pad for the asymmetric padding,
F.conv2d / F.linear, autograd for the gradients) in float64 on the CPU; they are cached, read-only, and shared by every
test and dtype that uses them.
"""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT3, ID3 = [F32, BF16, F16], ["f32", "bf16", "f16"]
ACC_MAX = float(1 << 24)                     # integers below 2^24 are exact in f32
EXACT_OUT_MAX = {F32: ACC_MAX - 1, BF16: 256.0, F16: 2048.0}   # every integer up to here is representable
ROUND_AMP = {F32: 16, BF16: 4, F16: 16}      # rounding mode (f32 only as the operand type of an f32-output launch)


def lattice(shape, seed, amp, density=1.0):
    """Integer-valued float64 CPU tensor: ``density`` of the entries uniform in {-amp..amp} \\ {0}, the rest 0."""
    g = torch.Generator().manual_seed(int(seed))
    mag = torch.randint(1, int(amp) + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    keep = torch.rand(tuple(shape), generator=g, dtype=torch.float64) < density
    return (mag * sign * keep).double()


def small_dense(shape, seed):
    """Dense integers in [-2, 2] (bias, time row, residual, skip)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-2, 3, tuple(shape), generator=g).double()


def exact_density(kred):
    return min(0.5, math.sqrt(100.0 / kred))


def _operand_params(kred, amp):
    """(amp, density) of the two GEMM operands: exact mode for amp None, else dense at ``amp`` (rounding mode)."""
    return (1, exact_density(kred)) if amp is None else (int(amp), 1.0)


def _is_integer(t):
    return bool(torch.equal(t, t.round())) and bool(torch.isfinite(t).all())


def _finish(ref, kred, amp_a, amp_b):
    """The dtype-independent conditions on a reference: integers everywhere, and an accumulator that stays below 2^24 in
    ANY summation order (the sum of the products' magnitudes is bounded by Kred amp_a amp_b)."""
    assert kred * amp_a * amp_b < ACC_MAX, (kred, amp_a, amp_b)
    for name in ("acc", "out"):
        t = getattr(ref, name)
        assert t.dtype == torch.float64 and _is_integer(t), f"{name}: not integer-valued"
    assert float(ref.acc.abs().max()) < ACC_MAX
    assert float(ref.out.abs().max()) < ACC_MAX
    ref.kred = kred
    return ref


def _conv_statement(x, w, KH, stride, pad_mode, ups):
    """The forward conv as tests/test_ops_gpu.py::test_conv2d states it; returns (y, pad)."""
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if pad_mode == "same":
        return F.conv2d(x, w, None, stride=stride, padding=KH // 2), KH // 2
    if pad_mode == "asym":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=stride, padding=0), 0
    return F.conv2d(x, w, None, stride=stride, padding=0), 0


@functools.lru_cache(maxsize=None)
def conv_reference(B, cins, H, W, Cout, KH, stride, pad_mode, ups, amp=None, with_bias=True, with_row=True,
                   with_res=True, relu=False, seed=0):
    """Forward conv2d (+ bias + time row + residual, + ReLU) on lattice data.  ``cins``: tuple of source channel counts;
    ``amp`` None = exact mode, else the rounding-mode amplitude.  Returns a namespace of float64 CPU tensors: xs, w, bias,
    rowvec, res (None where not asked for), acc (the GEMM alone), pre (before the ReLU) and out (after the whole epilogue), plus
    OH, OW, pad, hw."""
    Cin = sum(cins)
    kred = KH * KH * Cin
    a, d = _operand_params(kred, amp)
    xs = [lattice((B, c, H, W), 1000 + 17 * seed + i, a, d) for i, c in enumerate(cins)]
    w = lattice((Cout, Cin, KH, KH), 2000 + seed, a, d)
    acc, pad = _conv_statement(torch.cat(xs, 1), w, KH, stride, pad_mode, ups)
    OH, OW = acc.shape[2], acc.shape[3]
    bias = small_dense((Cout,), 3000 + seed) if with_bias else None
    rowvec = small_dense((B, Cout), 4000 + seed) if with_row else None
    res = small_dense((B, Cout, OH, OW), 5000 + seed) if with_res else None
    out = acc
    if bias is not None:
        out = out + bias[None, :, None, None]
    if rowvec is not None:
        out = out + rowvec[:, :, None, None]
    if res is not None:
        out = out + res
    pre = out
    if relu:
        out = F.relu(out)
    ref = SimpleNamespace(xs=xs, w=w, bias=bias, rowvec=rowvec, res=res, acc=acc, pre=pre, out=out, OH=OH, OW=OW, pad=pad,
                          hw=OH * OW, cins=cins, exact=amp is None)
    return _finish(ref, kred, a, a)


@functools.lru_cache(maxsize=None)
def linear_reference(M, ks, N, amp=None, with_bias=True, with_res=False, f32_matmul=False, images=1, seed=0):
    """out = cat(xs) @ w.T (+ bias) (+ residual) on lattice data; ``ks``: tuple of the sources' widths (two = the LoRA
    K extension ``x2``).  ``f32_matmul``: the product runs in float32, exact under the bound _finish asserts (every partial
    sum is an integer below Kred amp^2 < 2^24).  ``images``: the rows are that many images of M / images tokens (ops.linear's
    B), which is what a kernel's per-image sums would run over."""
    K = sum(ks)
    a, d = _operand_params(K, amp)
    xs = [lattice((M, k), 1100 + 17 * seed + i, a, d) for i, k in enumerate(ks)]
    w = lattice((N, K), 2100 + seed, a, d)
    x = torch.cat(xs, 1)
    if f32_matmul:
        assert K * a * a < ACC_MAX
        acc = F.linear(x.float(), w.float()).double()
    else:
        acc = F.linear(x, w)
    bias = small_dense((N,), 3100 + seed) if with_bias else None
    res = small_dense((M, N), 5100 + seed) if with_res else None
    out = acc
    if bias is not None:
        out = out + bias[None, :]
    if res is not None:
        out = out + res
    assert M % images == 0
    ref = SimpleNamespace(xs=xs, w=w, bias=bias, res=res, acc=acc, out=out, hw=M // images, ks=ks, exact=amp is None)
    return _finish(ref, K, a, a)


@functools.lru_cache(maxsize=None)
def dgrad_reference(B, cins, H, W, Cout, KH, seed=0):
    """Input gradient of a stride-1 'same' conv (autograd, float64) + the gradient arriving through a skip connection, as
    test_conv2d_dgrad states it.  The launch is the forward kernel on dout: its reduction runs over KH KH Cout."""
    Cin = sum(cins)
    kred = KH * KH * Cout
    a, d = _operand_params(kred, None)
    x = torch.zeros((B, Cin, H, W), dtype=torch.float64, requires_grad=True)
    w = lattice((Cout, Cin, KH, KH), 2200 + seed, a, d)
    y = F.conv2d(x, w, None, padding=KH // 2)
    dy = lattice(tuple(y.shape), 1200 + seed, a, d)
    skip = small_dense((B, Cin, H, W), 5200 + seed)
    y.backward(dy)
    acc = x.grad.detach()
    ref = SimpleNamespace(w=w, dy=dy, skip=skip, acc=acc, out=acc + skip, hw=H * W, cins=cins, exact=True)
    return _finish(ref, kred, a, a)


@functools.lru_cache(maxsize=None)
def wgrad_reference(B, cins, H, W, Cout, KH, stride, pad_mode, ups, seed=0):
    """Weight and bias gradient (autograd, float64) of the conv of conv_reference, as test_conv2d_wgrad states it.  The
    reduction runs over the B OH OW output pixels; ``out`` is the gradient [Cout, Cin, KH, KH], ``dbias`` the sum of dy."""
    Cin = sum(cins)
    w = torch.zeros((Cout, Cin, KH, KH), dtype=torch.float64, requires_grad=True)
    # the output size first (it sets the density): the statement on an empty-valued input
    probe, pad = _conv_statement(torch.zeros((1, Cin, H, W), dtype=torch.float64), w.detach(), KH, stride, pad_mode, ups)
    OH, OW = probe.shape[2], probe.shape[3]
    kred = B * OH * OW
    a, d = _operand_params(kred, None)
    xs = [lattice((B, c, H, W), 1300 + 17 * seed + i, a, d) for i, c in enumerate(cins)]
    y, _ = _conv_statement(torch.cat(xs, 1), w, KH, stride, pad_mode, ups)
    dy = lattice(tuple(y.shape), 1400 + seed, a, d)
    y.backward(dy)
    acc = w.grad.detach()
    dbias = dy.sum((0, 2, 3))
    assert _is_integer(dbias) and float(dbias.abs().max()) < ACC_MAX / 2
    assert float(acc.abs().max()) < ACC_MAX / 2        # the accumulating second call doubles it
    ref = SimpleNamespace(xs=xs, dy=dy, acc=acc, out=acc, dbias=dbias, OH=OH, OW=OW, pad=pad, hw=1, cins=cins, exact=True)
    return _finish(ref, kred, a, a)


def stats_of(out_nchw):
    """(sum, sum of squares) per (image, channel) of an NCHW reference, float64 [B, C] each."""
    return out_nchw.sum((2, 3)), (out_nchw ** 2).sum((2, 3))


def changed_fraction(out_f64, dtype):
    """Share of the outputs that one rounding to ``dtype`` changes."""
    return float((out_f64.to(dtype).double() != out_f64).double().mean())


def check_reference(ref, dtype, f32_out=False):
    """The dtype-dependent conditions on a reference.  Exact mode: hw max|out|^2 < 2^24, so every f32 partial sum of
    values or squares over an image is exact, and the outputs are integers the dtype represents.  Rounding mode: the outputs
    stay finite in the dtype and at least 1 % of them change under one rounding to it (``f32_out``: the launch stores f32,
    which must then hold the exact integer although the dtype would have rounded it)."""
    m = float(ref.out.abs().max())
    if ref.exact:
        assert ref.hw * m * m < ACC_MAX, (ref.hw, m)
        assert m <= EXACT_OUT_MAX[dtype], (m, dtype)
        assert torch.equal(ref.out.to(dtype).double(), ref.out)
    else:
        assert m < 65504.0, m
        if dtype != F32:
            frac = changed_fraction(ref.out, dtype)
            assert frac >= 0.01, f"only {100 * frac:.2f} % of the outputs change under .to({dtype})"
    return ref


_BUILDERS = {"conv": conv_reference, "linear": linear_reference, "dgrad": dgrad_reference, "wgrad": wgrad_reference}


def exact_reference(kind, *geometry, dtype, f32_out=False, **options):
    """The reference of one launch with EVERY condition asserted on it: ``kind`` names the torch statement ("conv", "linear",
    "dgrad", "wgrad"), ``geometry`` / ``options`` are its builder's arguments (the data does not depend on ``dtype`` in exact
    mode, so one cached reference serves the three of them), ``dtype`` the type the launch computes in.  The gradients of
    "wgrad" are f32 whatever the operand type."""
    return check_reference(_BUILDERS[kind](*geometry, **options), F32 if kind == "wgrad" else dtype, f32_out=f32_out)


def nonzero_fraction(out_f64):
    return float((out_f64 != 0).double().mean())


def to_tokens_cpu(x_nchw):
    B, C, H, W = x_nchw.shape
    return x_nchw.permute(0, 2, 3, 1).reshape(B * H * W, C)


def assert_exact(got, want_f64, dtype, what):
    """``got`` equals ``want_f64`` rounded ONCE to ``dtype`` (round-to-nearest-even; float32 for f32 outputs), bit pattern for
    bit pattern as torch.equal sees it.  ``got``: the kernel's [B*H*W, C] channels-last tensor for an NCHW ``want_f64``, else a
    tensor of want's shape.  A failure names the number of mismatches, the first one as (image, y, x, channel), got and want
    there, and the residues of channel, x and y modulo 16 among all mismatches: a lane, a tap or a tail."""
    got = got.detach().cpu()
    want = want_f64.float() if dtype == F32 else want_f64.to(dtype)
    geom = None
    if want.dim() == 4 and got.dim() == 2:
        B, C, H, W = want.shape
        geom = (B, H, W)
        want = to_tokens_cpu(want).contiguous()
    elif want.dim() == 2:
        geom = (1, want.shape[0], 1)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, expected {want.dtype}"
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    n = bad.shape[0]
    if geom is not None:
        B, H, W = geom
        row, ch = bad[:, 0], bad[:, 1]
        img, y, x = row // (H * W), (row // W) % H, row % W
        r0, c0 = int(row[0]), int(ch[0])
        first = f"(image {int(img[0])}, y {int(y[0])}, x {int(x[0])}, channel {c0})"
        g0, w0 = got[r0, c0], want[r0, c0]
        res = (f"channel % 16 in {sorted(set((ch % 16).tolist()))}, x % 16 in {sorted(set((x % 16).tolist()))}, "
               f"y % 16 in {sorted(set((y % 16).tolist()))}")
    else:
        i0 = tuple(int(v) for v in bad[0])
        first = f"index {i0}"
        g0, w0 = got[i0], want[i0]
        res = f"last index % 16 in {sorted(set((bad[:, -1] % 16).tolist()))}"
    raise AssertionError(f"{what}: {n} of {want.numel()} outputs differ from the exact result; first at {first}: "
                         f"got {float(g0)!r}, want {float(w0)!r}; {res}")


# ---- the case rows of tests/test_lattice_gpu.py, and the reference of each (test_lattice_host.py checks them all on the CPU) ----
from test_ops_gpu import CONV_CASES, H16_CASES, LN_FOLD_CASES, DGRAD_CASES, WGRAD_CASES   # noqa: E402

# (b) the rows of H16_CASES without a GroupNorm input
H16_ROWS = [c for c in H16_CASES if c[0] in ("full", "ragged_n192", "concat", "relu_nores")]
# (c) the case tuples of test_conv_fused_groupnorm_stats: B, Cin, H, W, Cout, tile, splitk
STATS_ROWS = [("tile_auto", 2, 64, 16, 16, 128, 0, 1), ("tile64", 2, 64, 8, 8, 320, 3, 1), ("splitk", 2, 256, 4, 4, 64, 3, 4),
              ("straddle", 3, 64, 3, 3, 64, 0, 1), ("autosplit", 2, 640, 2, 2, 128, 0, None)]
# (d) out_f32: M, C, N of a plain linear (M = 70 is ragged in every tile; K long enough that the 16-bit formats would round)
OUT_F32_SHAPE = (70, 640, 64)
OUT_F32_TILES = [3, 8, 13]
# (e) rounding rows, one per store path: name, kind, geometry, tile, splitk, residual, out window (columns past N in a row of out)
#     conv geometry = (B, cins, H, W, Cout, KH, stride, pad_mode, upsample); linear geometry = (M, ks, N)
ROUNDING_ROWS = [
    ("reg64x64", "conv", (2, (64,), 8, 8, 64, 3, 1, "same", False), 3, 1, True, 0),
    ("glds128x64_wide", "conv", (1, (64,), 12, 20, 320, 3, 1, "same", False), 8, 1, True, 0),
    ("glds128x128_wide", "conv", (1, (64,), 13, 21, 192, 3, 1, "same", False), 14, 1, True, 0),
    ("halodma", "conv", (1, (64,), 13, 21, 192, 3, 1, "same", False), 9, 1, True, 0),
    ("h16_lds_transposed", "conv", (1, (64,), 21, 37, 192, 3, 1, "same", False), 12, 1, True, 0),
    # ldo = N + 4: rows of out lose their 16-byte alignment, launch_conv3x3_h16 takes the direct path (conv3x3_h16.hip)
    ("h16_direct_ldo", "conv", (1, (64,), 21, 37, 192, 3, 1, "same", False), 12, 1, True, 4),
    # the A-stationary kernel takes no residual (conv_plan.hip, apanel_eligible): bias only
    ("apanel", "linear", (130, (640,), 640), 13, 1, False, 0),
    ("splitk_reduction", "conv", (2, (256,), 4, 4, 128, 3, 1, "same", False), 7, 4, True, 0),
]
# (f) plain linear: the non-GEGLU rows of LN_FOLD_CASES up to M = 1024, the LoRA K extension on two tiles, one full-chip row on two
LINEAR_ROWS = [(c[0], c[1], (c[2],), c[3], c[4], c[6], False, 1) for c in LN_FOLD_CASES if not c[5] and c[1] <= 1024]
LINEAR_ROWS += [("lora_x2_reg64x64", 77, (320, 64), 320, 3, True, False, 1), ("lora_x2_glds64", 77, (320, 64), 320, 7, True, False, 1)]
# full chip: the reference product runs in f32 under the exactness bound; the rows are 8 images of 1024 tokens (ops.linear's B)
LINEAR_ROWS += [("fullchip_glds128", 8192, (320,), 960, 8, False, True, 8), ("fullchip_apanel", 8192, (320,), 960, 13, False, True, 8)]


def linear_row_skipped(row, dtype):
    """The one skip: f32 rows of more than 2560 bytes do not fit the A-stationary kernel's 32-row panel."""
    return row[4] == 13 and dtype == F32 and sum(row[2]) > 640


def ref_conv_row(case, dtype):                                   # (a)
    name, B, cins, H, W, Cout, KH, stride, pad_mode, ups, tile, splitk = case
    return exact_reference("conv", B, tuple(cins), H, W, Cout, KH, stride, pad_mode, ups, dtype=dtype)


def ref_h16_row(case, dtype):                                    # (b)
    name, B, cins, H, W, Cout, fuse, relu, with_res, with_stats = case
    return exact_reference("conv", B, tuple(cins), H, W, Cout, 3, 1, "same", False, dtype=dtype, with_res=with_res, relu=relu,
                           seed=1)


def ref_stats_row(row, dtype):                                   # (c)
    name, B, Cin, H, W, Cout, tile, splitk = row
    return exact_reference("conv", B, (Cin,), H, W, Cout, 3, 1, "same", False, dtype=dtype, with_row=False, with_res=False,
                           seed=2)


def ref_out_f32(dtype):                                          # (d)
    M, C, N = OUT_F32_SHAPE
    return exact_reference("linear", M, (C,), N, dtype=dtype, f32_out=True, amp=ROUND_AMP[dtype], seed=3)


def ref_rounding_row(row, dtype):                                # (e)
    name, kind, geom, tile, splitk, with_res, window = row
    extra = {"with_row": False} if kind == "conv" else {}
    return exact_reference(kind, *geom, dtype=dtype, amp=ROUND_AMP[dtype], with_res=with_res, seed=4, **extra)


def ref_linear_row(row, dtype):                                  # (f)
    name, M, ks, N, tile, with_res, f32_matmul, images = row
    return exact_reference("linear", M, tuple(ks), N, dtype=dtype, with_res=with_res, f32_matmul=f32_matmul, images=images, seed=5)


def ref_dgrad_row(case, dtype):                                  # (g)
    name, B, cins, H, W, Cout, KH = case
    return exact_reference("dgrad", B, tuple(cins), H, W, Cout, KH, dtype=dtype, seed=6)


def ref_wgrad_row(case, dtype):                                  # (h): dw and dbias are f32 whatever the operand type
    name, B, cins, H, W, Cout, KH, stride, pad_mode, ups, splitm = case
    return exact_reference("wgrad", B, tuple(cins), H, W, Cout, KH, stride, pad_mode, ups, dtype=dtype, seed=7)


def all_reference_rows():
    """(id, dtype, builder) for every case row of sections (a) - (h) in every dtype it runs in."""
    rows = []
    for dt, dn in zip(DT3, ID3):
        rows += [(f"a-{c[0]}-{dn}", dt, functools.partial(ref_conv_row, c)) for c in CONV_CASES]
        rows += [(f"b-{c[0]}-{dn}", dt, functools.partial(ref_h16_row, c)) for c in H16_ROWS]
        rows += [(f"c-{c[0]}-{dn}", dt, functools.partial(ref_stats_row, c)) for c in STATS_ROWS]
        rows += [(f"d-out_f32-{dn}", dt, ref_out_f32)]
        if dt != F32:
            rows += [(f"e-{c[0]}-{dn}", dt, functools.partial(ref_rounding_row, c)) for c in ROUNDING_ROWS]
        rows += [(f"f-{c[0]}-{dn}", dt, functools.partial(ref_linear_row, c)) for c in LINEAR_ROWS if not linear_row_skipped(c, dt)]
        rows += [(f"g-{c[0]}-{dn}", dt, functools.partial(ref_dgrad_row, c)) for c in DGRAD_CASES]
        rows += [(f"h-{c[0]}-{dn}", dt, functools.partial(ref_wgrad_row, c)) for c in WGRAD_CASES]
    return rows
