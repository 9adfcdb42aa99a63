"""Exact tests of the conv / linear / gradient GEMM kernels on integer lattices (tests/lattice_util.py): on small-integer
inputs every output has ONE correct bit pattern, whatever the tile, the split-K, the summation order or the atomics, so
every assertion in this file is an equality and one dropped, duplicated or misplaced product fails it.  Each launch with a
forced tile code also asserts, from the plan ops.conv2d resolved (ops.TILE_LOG), that this tile ran: no row of this file is
substituted by the planner's rules (tile 12 on a map under 16 x 16 would become 9, tile 13 with a residual a register tile),
so the expected tile is the forced one everywhere and a silent fallback fails the test."""
import pytest
import torch

import lattice_util as L
from lattice_util import F32, DT3, ID3
from util import to_tokens

pytestmark = pytest.mark.gpu


def _launch(x1, wp, B, IH, IW, N, tile, splitk, **kw):
    """ops.conv2d under a forced tile code; asserts the tile (and the requested split-K) the plan resolved."""
    from madm_amd import ops
    from madm_amd._lib import lib
    lib.madm_debug_set_conv_tile(tile)
    ops.TILE_LOG = []
    try:
        out = ops.conv2d(x1, wp, B, IH, IW, N=N, splitk=splitk, **kw)
        torch.cuda.synchronize()
        log = ops.TILE_LOG
    finally:
        ops.TILE_LOG = None
        lib.madm_debug_set_conv_tile(0)
    assert len(log) == 1, log
    desc, ran, sk = log[0][0], log[0][1], log[0][2]
    assert tile == 0 or ran == tile, f"tile {tile} was forced, tile {ran} ran ({desc})"
    assert splitk is None or sk == splitk, f"split-K {splitk} was asked for, {sk} planned ({desc})"
    return out


def _dev(t):
    return None if t is None else t.float().cuda()


def _run_conv(ref, dtype, B, H, W, Cout, KH, stride, ups, tile, splitk, relu=False, stats=None, window=0):
    """The forward launch of a conv_reference: its sources, packed weights and epilogue operands, cast (exactly) to dtype."""
    from madm_amd import ops, packing
    kt = ops.k_tile(dtype)
    cins = list(ref.cins)
    toks = [to_tokens(x, dtype, packing.round_up(c, kt)) for x, c in zip(ref.xs, cins)]
    wp = packing.pack_conv_weight(ref.w.float(), dtype, kt, splits=cins).cuda()
    out = None
    if window:      # rows of out `window` columns longer than N
        out = torch.zeros((B * ref.OH * ref.OW, Cout + window), dtype=dtype, device="cuda")[:, :Cout]
    return _launch(toks[0], wp, B, H, W, Cout, tile, splitk, x2=toks[1] if len(toks) > 1 else None, KH=KH, KW=KH, stride=stride,
                   pad_t=ref.pad, pad_l=ref.pad, OH=ref.OH, OW=ref.OW, upsample=ups, bias=_dev(ref.bias), rowvec=_dev(ref.rowvec),
                   residual=None if ref.res is None else to_tokens(ref.res, dtype),
                   epilogue=ops.EPI_RELU if relu else ops.EPI_NONE, stats=stats, out=out)


def _run_linear(ref, dtype, N, tile, splitk=1, images=1, out_f32=False):
    from madm_amd import ops, packing
    kt = ops.k_tile(dtype)
    xs = [x.to(dtype).cuda() for x in ref.xs]
    assert all(k % kt == 0 for k in ref.ks)
    wq = packing.pack_linear_weight(ref.w.float(), dtype, kt).cuda()
    M = xs[0].shape[0]
    return _launch(xs[0], wq, images, M // images, 1, N, tile, splitk, x2=xs[1] if len(xs) > 1 else None, bias=_dev(ref.bias),
                   residual=None if ref.res is None else ref.res.to(dtype).cuda(), out_f32=out_f32)


def _assert_stats(st, ref, what):
    """Both f64 columns equal the exact sum and sum of squares of the output per (image, channel)."""
    s, q = L.stats_of(ref.out)
    got = st.cpu()
    L.assert_exact(got[..., 0].contiguous(), s, torch.float64, what + ": sum")
    L.assert_exact(got[..., 1].contiguous(), q, torch.float64, what + ": sum of squares")


# ---- (a) forward conv: every row of CONV_CASES with its tile and split-K, bias + time row + residual ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", L.CONV_CASES, ids=[c[0] for c in L.CONV_CASES])
def test_conv2d_exact(cuda, dtype, case):
    name, B, cins, H, W, Cout, KH, stride, pad_mode, ups, tile, splitk = case
    ref = L.ref_conv_row(case, dtype)
    out = _run_conv(ref, dtype, B, H, W, Cout, KH, stride, ups, tile, splitk)
    L.assert_exact(out, ref.out, dtype, name)


# ---- (b) the 16 x 16-patch kernel: ReLU, residual and fused statistics as H16_CASES asks for them ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", L.H16_ROWS, ids=[c[0] for c in L.H16_ROWS])
def test_conv3x3_h16_exact(cuda, dtype, case):
    name, B, cins, H, W, Cout, fuse, relu, with_res, with_stats = case
    ref = L.ref_h16_row(case, dtype)
    st = torch.zeros((B, Cout, 2), device="cuda", dtype=torch.float64) if with_stats else None
    out = _run_conv(ref, dtype, B, H, W, Cout, 3, 1, False, 12, 1, relu=relu, stats=st)
    L.assert_exact(out, ref.out, dtype, name)
    if with_stats:
        _assert_stats(st, ref, name)


# ---- (c) fused output statistics on the igemm and halo tiles ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", L.STATS_ROWS, ids=[c[0] for c in L.STATS_ROWS])
def test_conv_fused_stats_exact(cuda, dtype, row):
    name, B, Cin, H, W, Cout, tile, splitk = row
    ref = L.ref_stats_row(row, dtype)
    st = torch.zeros((B, Cout, 2), device="cuda", dtype=torch.float64)
    out = _run_conv(ref, dtype, B, H, W, Cout, 3, 1, False, tile, splitk, stats=st)
    L.assert_exact(out, ref.out, dtype, name)
    _assert_stats(st, ref, name)


# ---- (d) out_f32: the f32 output holds the exact integer, which the operand type would have rounded ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("tile", L.OUT_F32_TILES, ids=["reg64x64", "glds128", "apanel"])
def test_out_f32_exact(cuda, dtype, tile):
    M, C, N = L.OUT_F32_SHAPE
    ref = L.ref_out_f32(dtype)
    out = _run_linear(ref, dtype, N, tile, out_f32=True)
    assert out.dtype == F32
    L.assert_exact(out, ref.out, F32, f"out_f32 tile {tile}")


# ---- (e) rounding: one round-to-nearest-even of the exact integer, ties included, on every store path ----
@pytest.mark.parametrize("dtype", DT3[1:], ids=ID3[1:])
@pytest.mark.parametrize("row", L.ROUNDING_ROWS, ids=[c[0] for c in L.ROUNDING_ROWS])
def test_output_rounding_exact(cuda, dtype, row):
    name, kind, geom, tile, splitk, with_res, window = row
    ref = L.ref_rounding_row(row, dtype)
    if kind == "conv":
        B, cins, H, W, Cout, KH, stride, pad_mode, ups = geom
        out = _run_conv(ref, dtype, B, H, W, Cout, KH, stride, ups, tile, splitk, window=window)
        assert out.stride(0) == Cout + window
        if window:      # the columns behind N in a row of the buffer are not the kernel's
            rows = torch.as_strided(out, (out.shape[0], Cout + window), (Cout + window, 1))
            assert float(rows[:, Cout:].abs().max()) == 0.0, f"{name}: wrote past column N"
    else:
        M, ks, N = geom
        out = _run_linear(ref, dtype, N, tile, splitk=splitk)
    L.assert_exact(out, ref.out, dtype, name)


# ---- (f) plain linear: no LayerNorm, no GEGLU ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("row", L.LINEAR_ROWS, ids=[c[0] for c in L.LINEAR_ROWS])
def test_linear_exact(cuda, dtype, row):
    name, M, ks, N, tile, with_res, f32_matmul, images = row
    if L.linear_row_skipped(row, dtype):
        pytest.skip("f32 rows of more than 2560 bytes do not fit the 32-row panel (the 64 x 64 kernels serve them)")
    ref = L.ref_linear_row(row, dtype)
    out = _run_linear(ref, dtype, N, tile, images=images)
    L.assert_exact(out, ref.out, dtype, name)


# ---- (g) data gradient: the forward kernel on dout with the repacked weights, + the skip tensor ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", L.DGRAD_CASES, ids=[c[0] for c in L.DGRAD_CASES])
def test_conv2d_dgrad_exact(cuda, dtype, case):
    from madm_amd import ops, packing
    name, B, cins, H, W, Cout, KH = case
    ref = L.ref_dgrad_row(case, dtype)
    kt = ops.k_tile(dtype)
    cpads = [packing.round_up(c, kt) for c in cins]
    wp = packing.pack_conv_weight(ref.w.float(), dtype, kt, splits=cins).cuda()
    wt = ops.pack_dgrad_weights(wp, KH * KH)
    assert tuple(wt.shape) == (sum(cpads), KH * KH * Cout)
    skip_tok = torch.cat([to_tokens(s_, dtype, cp) for s_, cp in zip(torch.split(ref.skip, cins, 1), cpads)], 1)
    din = ops.conv2d_dgrad(to_tokens(ref.dy, dtype), wt, B, H, W, C=sum(cpads), KH=KH, KW=KH, pad_t=KH // 2, pad_l=KH // 2,
                           residual=skip_tok)
    torch.cuda.synchronize()
    parts, p0 = [], 0
    for c, cp in zip(cins, cpads):
        parts.append(din[:, p0:p0 + c])
        p0 += cp
    L.assert_exact(torch.cat(parts, 1), ref.out, dtype, name)


# ---- (h) weight gradient: dw, dbias, accumulation, padding channels ----
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", L.WGRAD_CASES, ids=[c[0] for c in L.WGRAD_CASES])
def test_conv2d_wgrad_exact(cuda, dtype, case):
    from madm_amd import ops, packing
    name, B, cins, H, W, Cout, KH, stride, pad_mode, ups, splitm = case
    ref = L.ref_wgrad_row(case, dtype)
    kt = ops.k_tile(dtype)
    Cin = sum(cins)
    toks = [to_tokens(x, dtype, packing.round_up(c, kt)) for x, c in zip(ref.xs, cins)]
    dy = to_tokens(ref.dy, dtype)
    kw = dict(x2=toks[1] if len(toks) > 1 else None, KH=KH, KW=KH, stride=stride, pad_t=ref.pad, pad_l=ref.pad, OH=ref.OH,
              OW=ref.OW, upsample=ups, splitm=splitm)
    db = torch.zeros(Cout, device="cuda")
    dw = ops.conv2d_wgrad(toks[0], dy, B, H, W, dbias=db, **kw)
    torch.cuda.synchronize()
    L.assert_exact(db, ref.dbias, F32, f"{name}: bias gradient")
    got = packing.unpack_conv_weight_grad(dw.cpu(), Cin, KH, KH, kt, splits=cins).contiguous()
    L.assert_exact(got, ref.out, F32, f"{name}: weight gradient")
    # the gradient of the padding channels is exactly zero: nothing of dw lies outside the unpacked part
    assert float(dw.double().abs().sum()) == float(ref.out.abs().sum()), f"{name}: padding channels are not zero"
    ops.conv2d_wgrad(toks[0], dy, B, H, W, dw=dw, **kw)
    torch.cuda.synchronize()
    got2 = packing.unpack_conv_weight_grad(dw.cpu(), Cin, KH, KH, kt, splits=cins).contiguous()
    L.assert_exact(got2, 2 * ref.out, F32, f"{name}: accumulating second call")
    assert float(dw.double().abs().sum()) == 2 * float(ref.out.abs().sum()), f"{name}: padding channels after accumulation"
