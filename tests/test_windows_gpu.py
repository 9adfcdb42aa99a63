"""Strided windows and write containment of every entry point that takes a leading dimension or writes a tensor.

Each case runs its kernel on DENSE operands and again with every operand that has a row stride inside a canary-guarded
window (tests/window_util.py: ld > columns, live NaN canaries on both sides, 256 guard rows in front and behind), and
asserts (1) no canary changed -- around the outputs AND around the inputs --, (2) the windowed result meets the torch-CPU
reference of the kernel's dense test within that test's tolerance (named at each use), (3) it is bit-identical to the
dense run where the launch is deterministic (forced tile, split-K 1, no float atomics), (4) nothing in the window is NaN
-- an over-read into a neighbour column would carry the canary's NaN into the output.

Layouts: 'dense' ld = cols; 'tight' the smallest ld > cols and smallest c0 > 0 that include/madm_hip.h allows for the
operand; 'wide' c0 = cols, ld = 3 cols.  Every pointer and stride handed to a kernel is inside the documented contract.
Shapes are the ragged rows of the dense tests' tables (test_ops_gpu.py, test_train_gpu.py, test_eval_gpu.py)."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

from util import to_tokens, from_tokens, rel_err
from window_util import Guarded, guarded_flat, layout
from test_ops_gpu import TOL, _q, _gen     # TOL: test_ops_gpu.py:15, the dense conv / linear / dgrad tolerance

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT2, ID2 = [F32, BF16], ["f32", "bf16"]
DT3, ID3 = [F32, BF16, F16], ["f32", "bf16", "f16"]
KINDS = ["tight", "wide"]


def _epc(dtype):
    """Elements per 16-byte chunk: the stride / offset quantum of every chunk-loading kernel."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def _win(t, kind, q, oq=None):
    """The 2-D tensor ``t`` (any device) loaded into a guarded window on the GPU."""
    ld, c0 = layout(kind, t.shape[1], q, oq)
    g = Guarded(t.shape[0], t.shape[1], t.dtype, ld=ld, c0=c0)
    g.load(t.cuda())
    return g


def _owin(rows, cols, dtype, kind, q, oq=None):
    ld, c0 = layout(kind, cols, q, oq)
    return Guarded(rows, cols, dtype, ld=ld, c0=c0)


def _vec(t, post=64):
    """A dense 1-D / small operand or output behind canaries (bias, statistics, flat buffers): returns (guard, view)."""
    g = guarded_flat(t.numel(), t.dtype, pre=64, post=post)
    g.flat.copy_(t.reshape(-1).cuda())
    return g, g.flat.view(t.shape)


def _check_all(guards, what):
    torch.cuda.synchronize()
    for name, g in guards.items():
        g.check(f"{what}: {name}")


def _no_nan(t, what):
    assert not bool(torch.isnan(t.float()).any()), f"{what}: NaN in the window (an over-read of a canary neighbour)"


# ----------------------------------------------------------------------------- conv2d forward
def _conv_reference(dtype, B, cins, H, W, Cout, KH, stride, pad_mode, ups, *, with_res=True, relu=False, seed=10):
    """The operands and the torch-CPU reference of test_ops_gpu.py::test_conv2d (same seeds, same expression)."""
    xs = [_q(_gen((B, c, H, W), seed + i), dtype) for i, c in enumerate(cins)]
    Cin = sum(cins)
    w = _q(_gen((Cout, Cin, KH, KH), 3) / math.sqrt(Cin * KH * KH), dtype)
    bias, rowvec = _gen((Cout,), 4), _gen((B, Cout), 5)
    x = torch.cat(xs, 1)
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if pad_mode == "same":
        ref, pad = F.conv2d(x, w, None, stride=stride, padding=KH // 2), KH // 2
    elif pad_mode == "asym":
        ref, pad = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=stride, padding=0), 0
    else:
        ref, pad = F.conv2d(x, w, None, stride=stride, padding=0), 0
    OH, OW = ref.shape[2], ref.shape[3]
    res = _q(_gen((B, Cout, OH, OW), 6), dtype) if with_res else None
    ref = ref + bias[None, :, None, None] + rowvec[:, :, None, None]
    if res is not None:
        ref = ref + res
    if relu:
        ref = F.relu(ref)
    return dict(xs=xs, w=w, bias=bias, rowvec=rowvec, res=res, ref=ref, pad=pad, OH=OH, OW=OW)


def _conv_launch(kind, dtype, toks, wp, B, H, W, N, *, tile, splitk, expect_tile=None, bias=None, rowvec=None, res=None,
                 ocols=None, odt=None, stats_shape=None, ld_out=None, ld_res=None, **kw):
    """One madm_conv2d_fwd launch with every strided operand in a ``kind`` window.  Returns (out clone, stats clone or
    None, extra result of ops.conv2d, the guards -- already checked)."""
    from madm_amd import ops
    from madm_amd._lib import lib
    e = _epc(dtype)
    ocols = N if ocols is None else ocols
    odt = dtype if odt is None else odt
    M = B * kw.get("OH", H * (2 if kw.get("upsample") else 1)) * kw.get("OW", W * (2 if kw.get("upsample") else 1))
    gs = {}
    for i, t in enumerate(toks):
        gs[f"in{i + 1}"] = _win(t, kind, e)
    gs["w"] = _win(wp, kind, e)
    args = dict(kw)
    if bias is not None:
        gs["bias"], args["bias"] = _vec(bias)
    if rowvec is not None:
        gs["rowvec"] = _win(rowvec, kind, 4)
        args["rowvec"] = gs["rowvec"].view
    oq = 2 if kw.get("epilogue") == ops.EPI_GEGLU else 4          # the contract's stride / offset quantum of out and residual
    if res is not None:
        # ldr != ldo in every window: tight ldr = cols + 3 quanta against ldo = cols + 1; wide ldr = 3 cols + 8 quanta at
        # c0 = cols + 8 quanta (8: ldr and the offset stay in ldo's residue class modulo a 16-byte chunk, so the 16 x 16-patch
        # kernel keeps the store path it takes for the window of out)
        if ld_res is not None:
            ld, c0 = ld_res
        else:
            ld, c0 = layout(kind, ocols, oq, 3 * oq)
            if kind == "wide":
                ld, c0 = ld + 8 * oq, c0 + 8 * oq
        gs["residual"] = Guarded(M, ocols, dtype, ld=ld, c0=c0)
        gs["residual"].load(res.cuda())
        args["residual"] = gs["residual"].view
    if ld_out is not None:
        gs["out"] = Guarded(M, ocols, odt, ld=ld_out[0], c0=ld_out[1])
    else:
        gs["out"] = _owin(M, ocols, odt, kind, oq)
    if stats_shape is not None:
        gs["stats"], args["stats"] = _vec(torch.zeros(stats_shape, dtype=torch.float64))
    lib.madm_debug_set_conv_tile(tile)
    ops.TILE_LOG = []
    try:
        r = ops.conv2d(gs["in1"].view, gs["w"].view, B, H, W, N=N, x2=gs["in2"].view if len(toks) > 1 else None,
                       out=gs["out"].view, splitk=splitk, **args)
        ran = ops.TILE_LOG[0][1]
    finally:
        ops.TILE_LOG = None
        lib.madm_debug_set_conv_tile(0)
    _check_all(gs, f"conv2d tile {tile} {kind}")
    assert expect_tile is None or ran == expect_tile, f"tile {ran} ran, not {expect_tile}"
    st = args["stats"].clone() if stats_shape is not None else None
    return gs["out"].view.clone(), st, r, gs


RAG_A = (2, [64], 5, 7, 320, 3, 1, "same", False)       # 3x3_s1_ragged / glds64_ragged: M = 70, N = 320
RAG_B = (1, [64], 13, 21, 192, 3, 1, "same", False)     # halo_ragged / glds128sq_3x3_ragged / ...: M = 273, N = 192
CONV_TILE_CASES = [
    # name, geometry, tile (0 = tuned table then heuristic), splitk: the ragged rows of CONV_CASES, one per tile code
    ("auto_ragged", RAG_A, 0, 1),
    ("reg128x128_ragged", RAG_B, 1, 1),
    ("reg128x64_ragged", RAG_B, 2, 1),
    ("reg64x64_ragged", RAG_A, 3, 1),
    ("reg64x64d_ragged", RAG_A, 6, 1),
    ("halo128_ragged", RAG_B, 4, 1),
    ("halo64_ragged", RAG_B, 5, 1),
    ("glds64_ragged", RAG_A, 7, 1),
    ("glds128_ragged", RAG_B, 8, 1),
    ("glds128_tiny_cout", (2, [64], 8, 8, 4, 3, 1, "same", False), 8, 1),
    ("tiny_cout", (2, [64], 8, 8, 4, 3, 1, "same", False), 3, 1),
    ("glds64s_ragged", (2, [128], 5, 7, 192, 3, 1, "same", False), 11, 1),
    ("glds128sq_ragged", RAG_B, 14, 1),
    ("glds128sq2_ragged", RAG_B, 15, 1),
    ("glds64d_ragged", RAG_B, 16, 1),
    ("glds128x64d_ragged", RAG_B, 17, 1),
    ("halodma128_ragged", RAG_B, 9, 1),
    ("halodma64_ragged", RAG_B, 10, 1),
    ("h16_upsample_ragged_concat", (1, [128, 64], 9, 13, 192, 3, 1, "same", True), 12, 1),
    ("concat_s2", (2, [128, 64], 16, 16, 192, 3, 2, "same", False), 7, 1),          # ld2 on an igemm tile, stride 2
    ("asym_s2", (2, [64], 16, 16, 128, 3, 2, "asym", False), 8, 1),
    # split-K > 1: the partial tiles go to the workspace, the reduction kernel stores through ldo
    ("reg64x64_splitk", (2, [256], 4, 4, 128, 3, 1, "same", False), 3, 4),
    ("glds64s_ragged_splitk", (2, [128], 5, 7, 192, 3, 1, "same", False), 11, 2),
    ("halo_splitk", (2, [256], 8, 16, 64, 3, 1, "same", False), 5, 2),
    ("halodma_splitk", (2, [256], 8, 16, 64, 3, 1, "same", False), 10, 2),
    ("h16_splitk3_ragged", (2, [128, 64], 19, 35, 192, 3, 1, "same", False), 12, 3),
]


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("case", CONV_TILE_CASES, ids=[c[0] for c in CONV_TILE_CASES])
def test_conv2d_windows(cuda, dtype, case):
    """madm_conv2d_fwd per tile code: in1 / in2 (ld1, ld2), w (ldw > K), rowvec (ldrv > N), residual (ldr != ldo) and out
    in windows; bias behind canaries.  Split-K sums its slabs in slab order (no atomics): bit-identical too."""
    from madm_amd import ops, packing
    name, (B, cins, H, W, Cout, KH, stride, pad_mode, ups), tile, splitk = case
    kt = ops.k_tile(dtype)
    c = _conv_reference(dtype, B, cins, H, W, Cout, KH, stride, pad_mode, ups)
    toks = [to_tokens(x, dtype, packing.round_up(ci, kt)) for x, ci in zip(c["xs"], cins)]
    wp = packing.pack_conv_weight(c["w"], dtype, kt, splits=cins)
    OH, OW = c["OH"], c["OW"]
    res = to_tokens(c["res"], dtype)
    outs = {}
    for kind in ["dense"] + KINDS:
        out, _, _, _ = _conv_launch(kind, dtype, toks, wp, B, H, W, Cout, tile=tile, splitk=splitk,
                                    expect_tile=tile if tile else None, bias=c["bias"], rowvec=c["rowvec"], res=res, KH=KH,
                                    KW=KH, stride=stride, pad_t=c["pad"], pad_l=c["pad"], OH=OH, OW=OW, upsample=ups)
        outs[kind] = out
        _no_nan(out, f"{name} {kind}")
        e, l2 = rel_err(from_tokens(out, B, OH, OW), c["ref"])
        assert e < TOL[dtype], f"{name} {kind}: max rel err {e:.3e} l2 {l2:.3e}"
    for kind in KINDS:
        assert torch.equal(outs[kind], outs["dense"]), f"{name}: {kind} window differs from the dense run"


LIN_CASES = [
    # name, M, C, N, tile, geglu, residual, dtypes: tile 13 (igemm_apanel.hip) and the GEGLU / LayerNorm-folded rows of LN_FOLD_CASES
    ("apanel32_ragged_n", 70, 1280, 72, 13, False, False, [BF16, F16]),      # f32 rows of 1280 do not fit the 32-row panel
    ("apanel64_geglu", 130, 640, 1024, 13, True, False, DT3),
    ("apanel128_onetile", 128, 64, 64, 13, False, False, DT3),
    ("q_glds64s_ragged", 130, 640, 640, 11, False, True, DT3),
    ("reg64x64", 96, 64, 128, 3, False, True, DT3),
    ("reg64x64d", 70, 128, 64, 6, False, False, DT3),
    ("geglu_reg128x64", 200, 640, 1024, 2, True, False, DT3),
    ("glds128sq_geglu", 256, 640, 1024, 14, True, False, DT3),
]
LIN_PARAMS = [pytest.param(c, dt, id=f"{c[0]}-{ID3[DT3.index(dt)]}") for c in LIN_CASES for dt in c[7]]


@pytest.mark.parametrize("case,dtype", LIN_PARAMS)
def test_linear_folded_layernorm_and_geglu_windows(cuda, dtype, case):
    """Linear(LayerNorm(x)) as one GEMM, with and without the fold, plain and GEGLU (the output window is N / 2 columns
    wide): x (ld1), W' (ldw), residual and out in windows.  Tolerances: test_linear_with_folded_layernorm's
    (test_ops_gpu.py:363) for the folded launch, TOL.get(dtype, 2.5e-3) (test_ops_gpu.py:360) for the plain one."""
    from madm_amd import ops, packing
    name, M, C, N, tile, geglu, with_res, _ = case
    kt = ops.k_tile(dtype)
    x = _gen((M, C), 1) * (0.5 + 2.0 * torch.rand((M, 1), generator=torch.Generator().manual_seed(7))) + 3.0 * _gen((M, 1), 8)
    x = _q(x, dtype)
    gamma, beta = 1.0 + 0.3 * _gen((C,), 2), 0.2 * _gen((C,), 3)
    w = _gen((N, C), 4) / math.sqrt(C)
    b = _gen((N,), 5)
    ref = F.linear(F.layer_norm(x, (C,), gamma, beta, 1e-5), w, b)
    if geglu:
        val, gate = ref.chunk(2, dim=-1)
        ref = val * F.gelu(gate)
        half = N // 2
        wk = torch.stack([w[:half], w[half:]], dim=1).reshape(N, C)
        bk = torch.stack([b[:half], b[half:]], dim=1).reshape(N)
    else:
        wk, bk = w, b
    res = _q(_gen((M, N), 6), dtype) if with_res else None
    if with_res:
        ref = ref + res
    r2 = F.linear(x, _q(wk, dtype), bk)
    if geglu:
        r2 = r2[:, 0::2] * F.gelu(r2[:, 1::2])
    if with_res:
        r2 = r2 + res
    wp, bp, cs = packing.fold_layernorm(wk, bk, gamma, beta, dtype, kt)
    wq = packing.pack_linear_weight(wk, dtype, kt)
    epi = ops.EPI_GEGLU if geglu else ops.EPI_NONE
    ocols = N // 2 if geglu else N
    tol = {F32: 3e-5, BF16: 1.5e-2, F16: 2.5e-3}[dtype]
    for fold in (True, False):
        outs = {}
        for kind in ["dense"] + KINDS:
            extra = {}
            if fold:
                g_cs, csv = _vec(cs)
                extra["ln"] = (csv, 1e-5)
            out, _, _, _ = _conv_launch(kind, dtype, [x.to(dtype)], wp if fold else wq, 1, M, 1, N, tile=tile, splitk=1,
                                        expect_tile=tile, bias=bp if fold else bk, res=None if res is None else res.to(dtype),
                                        ocols=ocols, epilogue=epi, **extra)
            if fold:
                g_cs.check("ln_colsum")
            outs[kind] = out
            _no_nan(out, f"{name} {kind}")
            e, l2 = rel_err(out.float().cpu(), ref if fold else r2)
            assert e < (tol if fold else TOL.get(dtype, 2.5e-3)), f"{name} {kind} fold={fold}: {e:.3e} {l2:.3e}"
        for kind in KINDS:
            assert torch.equal(outs[kind], outs["dense"]), f"{name} fold={fold}: {kind} window differs from the dense run"


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("tile", [3, 8, 13], ids=["reg64x64", "glds128", "apanel"])
def test_conv2d_out_f32_windows(cuda, dtype, tile):
    """out_f32 (the attention logits of the GEMM-based VAE mid-block attention): an f32 [M][ldo] window written from
    16-bit operands -- a store path of its own; shape = LN_FOLD_CASES reg64x64d (M = 70, ragged in every tile).  TOL as
    test_conv2d: the f32 output only drops the final rounding."""
    from madm_amd import ops, packing
    M, C, N = 70, 128, 64
    kt = ops.k_tile(dtype)
    x, w, b = _q(_gen((M, C), 1), dtype), _q(_gen((N, C), 4) / math.sqrt(C), dtype), _gen((N,), 5)
    ref = F.linear(x, w, b)
    wq = packing.pack_linear_weight(w, dtype, kt)
    outs = {}
    for kind in ["dense"] + KINDS:
        out, _, _, _ = _conv_launch(kind, dtype, [x.to(dtype)], wq, 1, M, 1, N, tile=tile, splitk=1, expect_tile=tile, bias=b,
                                    odt=F32, out_f32=True)
        assert out.dtype == F32
        outs[kind] = out
        _no_nan(out, kind)
        e, l2 = rel_err(out.cpu(), ref)
        assert e < TOL[dtype], f"{kind}: {e:.3e} {l2:.3e}"
    for kind in KINDS:
        assert torch.equal(outs[kind], outs["dense"])


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("case", [(3, 64, 3, 3, 64, 0, 1), (2, 64, 8, 8, 320, 3, 1), (2, 256, 4, 4, 64, 3, 4),
                                  (1, 64, 13, 21, 192, 4, 1), (1, 64, 13, 21, 192, 9, 1), (1, 64, 13, 21, 192, 8, 1)],
                         ids=["straddle", "tile64", "splitk", "halo_ragged", "halodma_ragged", "glds128_ragged"])
def test_conv2d_relu_and_stats_windows(cuda, dtype, case):
    """The ReLU epilogue and the fused output statistics (f64 [B][N][2] behind canaries; accumulated with atomics, so
    held to the dense test's tolerance, test_conv_fused_groupnorm_stats, test_ops_gpu.py:427-428; the stored tensor itself
    stays bit-identical).  The first three shapes are that test's, the others the ragged row of CONV_CASES."""
    from madm_amd import ops, packing
    B, Cin, H, W, Cout, tile, splitk = case
    kt = ops.k_tile(dtype)
    x = _q(_gen((B, Cin, H, W), 1), dtype)
    w = _q(_gen((Cout, Cin, 3, 3), 2) / math.sqrt(Cin * 9), dtype)
    bias = _gen((Cout,), 3)
    ref = F.relu(F.conv2d(x, w, bias, padding=1))
    wp = packing.pack_conv_weight(w, dtype, kt)
    stol = 1e-4 if dtype == F32 else 2e-2
    outs = {}
    for kind in ["dense"] + KINDS:
        out, st, _, _ = _conv_launch(kind, dtype, [to_tokens(x, dtype)], wp, B, H, W, Cout, tile=tile, splitk=splitk,
                                     expect_tile=tile if tile else None, bias=bias, stats_shape=(B, Cout, 2), KH=3, KW=3,
                                     pad_t=1, pad_l=1, epilogue=ops.EPI_RELU)
        outs[kind] = out
        _no_nan(out, kind)
        e, l2 = rel_err(from_tokens(out, B, H, W), ref)
        assert e < TOL[dtype], f"{kind}: {e:.3e} {l2:.3e}"
        sums = st.float().cpu()
        assert rel_err(sums[..., 0], ref.sum((2, 3)))[0] < stol and rel_err(sums[..., 1], (ref ** 2).sum((2, 3)))[0] < stol
    if tile:
        for kind in KINDS:
            assert torch.equal(outs[kind], outs["dense"])


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", [("ragged_map", 3, 64, 5, 7, 128, 5, 3, True), ("ten_channel_groups", 2, 64, 8, 8, 320, 9, 3, True),
                                  ("unet8_1280_halo", 1, 128, 8, 8, 1280, 2, 9, False)], ids=lambda c: c[0])
def test_conv2d_post_groupnorm_windows(cuda, dtype, case):
    """post_gn carried by the split-K reduction (igemm.hip splitk_groupnorm_kernel stores through ldo, in 16-byte and in
    8-byte units): rows of POST_GN_CASES; tolerance as test_conv_post_groupnorm_on_the_splitk_reduction
    (test_ops_gpu.py:566).  No atomics (slab-order sums, one workgroup per group): bit-identical to the dense run."""
    from madm_amd import ops, packing
    name, B, Cin, H, W, Cout, splitk, tile, with_row = case
    kt = ops.k_tile(dtype)
    x = _q(_gen((B, Cin, H, W), 1), dtype)
    w = _q(_gen((Cout, Cin, 3, 3), 2) / math.sqrt(Cin * 9), dtype)
    bias = _gen((Cout,), 3)
    row = (0.5 * _gen((B, Cout), 6)) if with_row else None
    gamma, beta = 1.0 + 0.2 * _gen((Cout,), 4), 0.3 * _gen((Cout,), 5)
    conv_ref = F.conv2d(x, w, bias, padding=1)
    if row is not None:
        conv_ref = conv_ref + row[:, :, None, None]
    ref = F.silu(F.group_norm(conv_ref, 32, gamma, beta, eps=1e-5))
    wp = packing.pack_conv_weight(w, dtype, kt)
    outs = {}
    for kind in ["dense"] + KINDS:
        g_g, gv = _vec(gamma)
        g_b, bv = _vec(beta)
        out, st, (_, applied), _ = _conv_launch(kind, dtype, [to_tokens(x, dtype)], wp, B, H, W, Cout, tile=tile, splitk=splitk,
                                                expect_tile=tile, bias=bias, rowvec=row, stats_shape=(B, Cout, 2), KH=3, KW=3,
                                                pad_t=1, pad_l=1, post_gn=(gv, bv, 32, 1e-5, True))
        g_g.check("pn_gamma"), g_b.check("pn_beta")
        assert applied, name
        assert float(st.abs().max()) == 0.0
        outs[kind] = out
        _no_nan(out, kind)
        e, l2 = rel_err(from_tokens(out, B, H, W), ref)
        assert e < (3e-5 if dtype == F32 else 2e-2), f"{name} {kind}: {e:.3e} {l2:.3e}"
    for kind in KINDS:
        assert torch.equal(outs[kind], outs["dense"])


H16_CELLS = [(ldo8, n8) for ldo8 in (0, 4) for n8 in (0, 4)]
H16_VARIANTS = [
    # name, B, Cin(list), H, W, fused GroupNorm input, residual, stats, splitk: shapes of H16_CASES / h16_splitk3_ragged
    ("concat_res_stats", 1, [128, 64], 21, 37, None, True, True, 1),
    ("gn_silu_concat_straddle", 2, [1280, 640], 16, 16, "silu", True, True, 1),
    ("relu_nores", 1, [64], 21, 37, None, False, False, 1),
    ("splitk3_ragged", 2, [128, 64], 19, 35, None, True, False, 3),
]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cell", H16_CELLS, ids=[f"ldo8_{a}-n8_{b}" for a, b in H16_CELLS])
@pytest.mark.parametrize("var", H16_VARIANTS, ids=[v[0] for v in H16_VARIANTS])
def test_conv3x3_h16_store_paths_windows(cuda, dtype, cell, var):
    """Tile 12 in 16-bit, ldo % 8 in {0, 4} x N % 8 in {0, 4} (N = 192: N = 192 of the tables; N = 68 of 3x3_s1_sliced):
    the LDS-transposed 16-byte store path runs only in the (0, 0) cell with a 16-byte aligned window, the direct 8-byte
    path in the other three, in every split-K launch and, inside the (0, 0) cell, wherever out or residual keeps only the
    contract's 8 bytes or ldr % 8 == 4 (layouts 'tight', 'res8', 'ldr4').  Tolerances: test_conv3x3_h16 (test_ops_gpu.py:202,207)."""
    from madm_amd import ops, packing
    name, B, cins, H, W, fuse, with_res, with_stats, splitk = var
    ldo8, n8 = cell
    Cout = 192 if n8 == 0 else 68
    kt, Cin = ops.k_tile(dtype), sum(cins)
    xs = [_q(_gen((B, c, H, W), 30 + i) * (1.0 + 0.5 * i) + 0.25 * i, dtype) for i, c in enumerate(cins)]
    w = _q(_gen((Cout, Cin, 3, 3), 3) / math.sqrt(Cin * 9), dtype)
    bias, rowvec = _gen((Cout,), 4), _gen((B, Cout), 5)
    h = torch.cat(xs, 1)
    toks = [to_tokens(x, dtype) for x in xs]
    if fuse is not None:
        gamma, beta = 1.0 + 0.2 * _gen((Cin,), 6), 0.3 * _gen((Cin,), 7)
        h = F.silu(F.group_norm(h, 32, gamma, beta, eps=1e-5))
    relu = name == "relu_nores"
    ref = F.conv2d(h, w, None, padding=1) + bias[None, :, None, None] + rowvec[:, :, None, None]
    res = _q(_gen((B, Cout, H, W), 8), dtype) if with_res else None
    if res is not None:
        ref = ref + res
    if relu:
        ref = F.relu(ref)
    wp = packing.pack_conv_weight(w, dtype, kt, splits=cins)
    # The windows.  The contract of out / residual is 8 bytes (4 elements) for the pointers and 4 elements for ldo / ldr;
    # the launcher takes the 16-byte path only when N, ldo, ldr are multiples of 8 AND both pointers are 16-byte aligned.
    # name: (layout of the other operands, (ldo, c0 of out), (ldr, c0 of residual)); ldr != ldo everywhere
    def up(x, r):          # the smallest value >= x that is r modulo 8
        return x + ((r - x) % 8)
    if ldo8 == 0:
        ldt, ldw_ = up(Cout + 12, 0), up(3 * Cout, 0)
        lays = {
            "dense": ("dense", (Cout, 0), (Cout, 0)),
            # tight: the smallest c0 the contract allows -- out keeps 8 bytes only although ldo % 8 == 0 (direct path whatever
            # N % 8 is; the launcher used to look at ldo and N alone)
            "tight": ("tight", (ldt, 4), (ldt + 8, 8)),
            # out 16-byte aligned, residual 8 bytes only with ldr % 8 == 0 (the residual pointer decides)
            "res8": ("tight", (ldt, 8), (ldt + 8, 4)),
            # out and residual 16-byte aligned, ldr % 8 == 4: every other residual row keeps 8 bytes only (ldr decides)
            "ldr4": ("tight", (ldt, 8), (ldt + 12, 8)),
            # everything 16-byte aligned inside a strided window: with N % 8 == 0 the 16-byte path itself, strided
            "aligned": ("tight", (ldt, 8), (ldt + 8, 8)),
            "wide": ("wide", (ldw_, up(Cout, 0)), (ldw_ + 8, up(Cout, 0))),
        }
    else:
        ldt, ldw_ = up(Cout + 8, 4), up(3 * Cout, 4)
        lays = {"dense": ("dense", (Cout, 0), (Cout, 0)), "tight": ("tight", (ldt, 4), (ldt + 8, 4)),
                "wide": ("wide", (ldw_, Cout), (ldw_ + 8, Cout))}
    for kind, (_, (ld_, c0_), (ldr_, cr_)) in lays.items():
        if kind != "dense":
            assert ld_ % 8 == ldo8 and Cout % 8 == n8 and c0_ + Cout <= ld_ and cr_ + Cout <= ldr_ and ldr_ != ld_
            assert c0_ % 4 == 0 and cr_ % 4 == 0 and ld_ % 4 == 0 and ldr_ % 4 == 0          # inside the contract
    if not with_res:       # the layouts that differ in the residual alone collapse
        lays = {k: v for k, v in lays.items() if k not in ("res8", "ldr4")}
    tol = {BF16: 2e-2, F16: 3e-3}[dtype]
    outs = {}
    for kind, (okind, ld_out, ld_res) in lays.items():
        extra, gg = {}, {}
        if fuse is not None:
            sts = []
            for i, t in enumerate(toks):
                st = torch.zeros((B, t.shape[1], 2), dtype=torch.float64, device="cuda")
                ops.groupnorm_stats(t, B, H * W, st)
                gg[f"gn_sums{i + 1}"], sv = _vec(st)
                sts.append(sv)
            gg["gn_gamma"], gv = _vec(gamma)
            gg["gn_beta"], bv = _vec(beta)
            extra["gn"] = (sts, gv, bv, 32, 1e-5, fuse)
        out, st, _, _ = _conv_launch(okind, dtype, toks, wp, B, H, W, Cout, tile=12, splitk=splitk, expect_tile=12, bias=bias,
                                     rowvec=rowvec, res=None if res is None else to_tokens(res, dtype),
                                     stats_shape=(B, Cout, 2) if with_stats else None, ld_out=ld_out, ld_res=ld_res, KH=3, KW=3, pad_t=1,
                                     pad_l=1, epilogue=ops.EPI_RELU if relu else ops.EPI_NONE, **extra)
        _check_all(gg, f"{name} {kind}")
        outs[kind] = out
        _no_nan(out, f"{name} {kind}")
        e, l2 = rel_err(from_tokens(out, B, H, W), ref)
        assert e < tol, f"{name} {kind}: max rel err {e:.3e} l2 {l2:.3e}"
        if st is not None:
            sums = st.float().cpu()
            assert rel_err(sums[..., 0], ref.sum((2, 3)))[0] < tol and rel_err(sums[..., 1], (ref ** 2).sum((2, 3)))[0] < tol
    # the two store paths round the same f32 values once: the bits do not depend on which of them a layout takes (with
    # N % 8 == 0 the dense run takes the 16-byte path, 'tight' / 'res8' / 'ldr4' the direct one)
    for kind in lays:
        assert torch.equal(outs[kind], outs["dense"]), f"{name}: {kind} window differs from the dense run"


# ----------------------------------------------------------------------------- direct calls of the C ABI
def _call(name, *args):
    """The entry point itself (wrappers that allocate their own output cannot be handed a guarded one)."""
    from madm_amd import ops
    from madm_amd._lib import lib, check
    check(getattr(lib, name)(*args, ops._stream()), name)


def _code(dtype):
    from madm_amd import ops
    return ops.dtype_code(dtype)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _flat_out(shape, dtype):
    """A dense output of ``shape`` with the canary starting at its last element + 1 (and in front of it)."""
    n = 1
    for s in shape:
        n *= s
    g = guarded_flat(n, dtype, pre=64, post=1024)
    return g, g.flat.view(shape)


# ----------------------------------------------------------------------------- conv2d_wgrad / dgrad / weight packing
WGRAD_WIN_CASES = [
    # name, B, Cin(list), H, W, Cout, KH, splitm: N = 68 (N % 8 == 4: the last 16-byte chunk of a 16-bit dout row covers 4
    # elements of the neighbour) and the two-source linear_lora row of WGRAD_CASES; splitm 1 and > 1 with a remainder slice
    ("3x3_s1_sliced_splitm1", 2, [64], 12, 20, 68, 3, 1),
    ("3x3_s1_sliced_splitm7", 2, [64], 12, 20, 68, 3, 7),
    ("linear_lora_splitm1", 1, [320, 64], 77, 1, 320, 1, 1),
    ("linear_lora_splitm3", 1, [320, 64], 77, 1, 320, 1, 3),
    ("3x3_tiny_cout", 2, [64], 8, 8, 4, 3, 0),
]


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("case", WGRAD_WIN_CASES, ids=[c[0] for c in WGRAD_WIN_CASES])
def test_conv2d_wgrad_windows(cuda, dtype, case):
    """madm_conv2d_wgrad: x1 / x2 / dout in windows (ld1, ld2, ldd), dw and dbias behind canaries.  The slices add with
    float atomics: held to test_conv2d_wgrad's tolerance (2e-5, test_ops_gpu.py:630,634), not to bit-identity; with ONE
    slice every element has one owner and the windowed run must equal the dense one bit for bit."""
    from madm_amd import ops, packing
    name, B, cins, H, W, Cout, KH, splitm = case
    kt = ops.k_tile(dtype)
    xs = [_q(_gen((B, c, H, W), 30 + i), dtype) for i, c in enumerate(cins)]
    Cin = sum(cins)
    w = (_gen((Cout, Cin, KH, KH), 3) / math.sqrt(Cin * KH * KH)).requires_grad_(True)
    y = F.conv2d(torch.cat(xs, 1), w, None, padding=KH // 2)
    dy = _q(_gen(tuple(y.shape), 7), dtype)
    y.backward(dy)
    cpads = [packing.round_up(c, kt) for c in cins]
    toks = [to_tokens(xi, dtype, cp) for xi, cp in zip(xs, cpads)]
    dyt = to_tokens(dy, dtype)
    K = KH * KH * sum(cpads)
    e = _epc(dtype)
    dws = {}
    for kind in ["dense"] + KINDS:
        gs = {f"in{i + 1}": _win(t, kind, e) for i, t in enumerate(toks)}
        gs["dout"] = _win(dyt, kind, 4)                      # ldd: a multiple of 4 elements, dout aligned to 4 elements
        gs["dw"], dw = _flat_out((Cout, K), F32)
        gs["dbias"], db = _flat_out((Cout,), F32)
        dw.zero_(), db.zero_()
        ops.conv2d_wgrad(gs["in1"].view, gs["dout"].view, B, H, W, x2=gs["in2"].view if len(toks) > 1 else None, KH=KH, KW=KH,
                         pad_t=KH // 2, pad_l=KH // 2, splitm=splitm, dw=dw, dbias=db)
        _check_all(gs, f"wgrad {name} {kind}")
        _no_nan(dw, f"{name} {kind} dw"), _no_nan(db, f"{name} {kind} dbias")
        eb, _ = rel_err(db.cpu(), dy.sum((0, 2, 3)))
        assert eb < 2e-5, f"{name} {kind}: bias gradient {eb:.3e}"
        got = packing.unpack_conv_weight_grad(dw.cpu(), Cin, KH, KH, kt, splits=cins)
        er, l2 = rel_err(got, w.grad)
        assert er < 2e-5, f"{name} {kind}: max rel err {er:.3e} l2 {l2:.3e}"
        # the gradient of the padding channels is exactly zero
        assert float(dw.abs().sum()) == pytest.approx(float(got.abs().sum()), rel=1e-5)
        dws[kind] = dw.clone()
    if splitm == 1:
        for kind in KINDS:
            assert torch.equal(dws[kind], dws["dense"]), f"{name}: {kind} window differs from the dense run"


DGRAD_WIN_CASES = [("3x3_ragged", 1, [128], 5, 7, 64, 3), ("3x3_concat", 2, [128, 64], 8, 16, 192, 3), ("linear", 1, [320], 77, 1, 1280, 1)]


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("case", DGRAD_WIN_CASES, ids=[c[0] for c in DGRAD_WIN_CASES])
def test_conv2d_dgrad_windows(cuda, dtype, case):
    """madm_pack_dgrad_weights (wt behind canaries, bit-identical to the transposition stated in torch) and the data
    gradient through conv2d_dgrad with dout, wt, residual and out in windows; rows of DGRAD_CASES, tolerance TOL."""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    name, B, cins, H, W, Cout, KH = case
    kt, Cin, taps = ops.k_tile(dtype), sum(cins), KH * KH
    x = _gen((B, Cin, H, W), 40).requires_grad_(True)
    w = _q(_gen((Cout, Cin, KH, KH), 3) / math.sqrt(Cin * KH * KH), dtype)
    y = F.conv2d(x, w, None, padding=KH // 2)
    dy = _q(_gen(tuple(y.shape), 8), dtype)
    skip = _q(_gen((B, Cin, H, W), 9), dtype)
    y.backward(dy)
    ref = x.grad + skip
    cpads = [packing.round_up(c, kt) for c in cins]
    C = sum(cpads)
    wp = packing.pack_conv_weight(w, dtype, kt, splits=cins)
    g_w, wv = _vec(wp, post=1024)
    g_wt, wt = _flat_out((C, taps * Cout), dtype)
    _call("madm_pack_dgrad_weights", _code(dtype), _p(wv), _p(wt), Cout, taps, C)
    _check_all({"w": g_w, "wt": g_wt}, "pack_dgrad_weights")
    # wt[c][taps - 1 - t][n] = w[n][t][c] (madm_hip.h): pure data movement
    assert torch.equal(wt.cpu(), wp.view(Cout, taps, C).flip(1).permute(2, 1, 0).reshape(C, taps * Cout))
    skip_tok = torch.cat([to_tokens(s_, dtype, cp) for s_, cp in zip(torch.split(skip, cins, 1), cpads)], 1)
    dyt = to_tokens(dy, dtype)
    e = _epc(dtype)
    outs = {}
    for kind in ["dense"] + KINDS:
        gs = {"dout": _win(dyt, kind, e), "wt": _win(wt, kind, e), "out": _owin(B * H * W, C, dtype, kind, 4)}
        ld, c0 = layout(kind, C, 4, 12)
        gs["residual"] = Guarded(B * H * W, C, dtype, ld=ld, c0=c0)
        gs["residual"].load(skip_tok)
        lib.madm_debug_set_conv_tile(3)
        try:
            ops.conv2d_dgrad(gs["dout"].view, gs["wt"].view, B, H, W, C=C, KH=KH, KW=KH, pad_t=KH // 2, pad_l=KH // 2,
                             out=gs["out"].view, residual=gs["residual"].view, splitk=1)
        finally:
            lib.madm_debug_set_conv_tile(0)
        _check_all(gs, f"dgrad {name} {kind}")
        outs[kind] = gs["out"].view.clone()
        _no_nan(outs[kind], f"{name} {kind}")
        got = from_tokens(outs[kind], B, H, W)
        parts, p0 = [], 0
        for c, cp in zip(cins, cpads):
            parts.append(got[:, p0:p0 + c])
            p0 += cp
        er, l2 = rel_err(torch.cat(parts, 1), ref)
        assert er < TOL[dtype], f"{name} {kind}: max rel err {er:.3e} l2 {l2:.3e}"
    for kind in KINDS:
        assert torch.equal(outs[kind], outs["dense"])


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_weight_packing_windows(cuda, dtype):
    """madm_pack_weight with ldo > the packed width (the K padding belongs to the window and is exactly zero: the torch
    statement packing.pack_conv_weight holds the same zeros) and madm_fold_layernorm_pack (out / bias / colsum behind
    canaries); the shapes of test_weight_packing_kernels_equal_the_torch_statements, same assertions (bit for bit, folded
    bias to 1e-6, test_ops_gpu.py:507-508)."""
    from madm_amd import ops, packing
    kt = ops.k_tile(dtype)
    g = torch.Generator().manual_seed(11)
    e = _epc(dtype)
    for (N, splits, k, inter) in [(36, [4], 3, False), (68, [100, 28, 64], 1, False), (320, [640, 320], 3, False), (64, [320], 1, True)]:
        w = torch.randn((N, sum(splits), k, k), generator=g)
        if inter:
            ref, _ = packing.pack_geglu_weight(w.reshape(N, -1), torch.zeros(N), dtype, kt)
        else:
            ref = packing.pack_conv_weight(w, dtype, kt, splits)
        cols = ref.shape[1]
        g_w, wv = _vec(w, post=1024)
        arr = (ctypes.c_int * len(splits))(*splits)
        for kind in ["dense"] + KINDS:
            go = _owin(N, cols, dtype, kind, e)
            _call("madm_pack_weight", _code(dtype), _p(wv), _p(go.view), go.ld, N, sum(splits), k * k, len(splits), arr, kt,
                  1 if inter else 0)
            _check_all({"w": g_w, "out": go}, f"pack_weight {N} {splits} {kind}")
            assert torch.equal(go.view.cpu(), ref), (N, splits, k, kind)
    for (N, K, with_b, inter) in [(960, 320, True, False), (640, 640, False, False), (2560, 320, True, True)]:
        w = torch.randn((N, K), generator=g) / K ** 0.5
        b = torch.randn((N,), generator=g) if with_b else None
        gamma, beta = 1 + 0.2 * torch.randn((K,), generator=g), 0.3 * torch.randn((K,), generator=g)
        rW, rB, rC = packing.fold_layernorm(w, b, gamma, beta, dtype, kt, interleave=inter)
        gs = {}
        gs["w"], wv = _vec(w, post=1024)
        gs["gamma"], gv = _vec(gamma)
        gs["beta"], bv = _vec(beta)
        bb = None
        if with_b:
            gs["b"], bb = _vec(b)
        gs["out"], ov = _flat_out((N, K), dtype)
        gs["bias_out"], bo = _flat_out((N,), F32)
        gs["colsum"], co = _flat_out((N,), F32)
        _call("madm_fold_layernorm_pack", _code(dtype), _p(wv), _p(bb), _p(gv), _p(bv), _p(ov), _p(bo), _p(co), N, K, 1 if inter else 0)
        _check_all(gs, f"fold_layernorm_pack {N} {K}")
        assert torch.equal(ov.cpu(), rW) and torch.equal(co.cpu(), rC), (N, K)
        assert rel_err(bo.cpu(), rB)[0] < 1e-6, (N, K)


# ----------------------------------------------------------------------------- attention
ATTN_WIN_CASES = [(2, 8, 64, 64, 40), (2, 8, 64, 77, 40), (2, 8, 16, 77, 160), (1, 2, 200, 333, 64), (1, 1, 64, 64, 512),
                  (1, 8, 2048, 2048, 40), (1, 2, 2100, 2100, 40)]


@pytest.mark.parametrize("dtype", DT3, ids=ID3)
@pytest.mark.parametrize("case", ATTN_WIN_CASES, ids=[f"B{c[0]}H{c[1]}q{c[2]}k{c[3]}d{c[4]}" for c in ATTN_WIN_CASES])
def test_attention_windows(cuda, dtype, case):
    """madm_attention_fwd: q / k / v and o in windows (self, cross over the 77-token prompt, ragged tails, the VAE head,
    the 128-query long-map variant and its ragged form); rows of ATTN_CASES, test_attention's tolerance
    (test_ops_gpu.py:1009).  No atomics: bit-identical to the dense run."""
    from madm_amd import ops
    B, H, Lq, Lk, D = case
    q, k, v = _q(_gen((B, Lq, H, D), 1), dtype), _q(_gen((B, Lk, H, D), 2), dtype), _q(_gen((B, Lk, H, D), 3), dtype)
    scale = D ** -0.5
    ref = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale)
    ref = ref.transpose(1, 2).reshape(B * Lq, H * D)
    C, e = H * D, _epc(dtype)
    oq = 8 // (16 // e)          # o: rows and pointer keep 8 bytes
    outs = {}
    for kind in ["dense"] + KINDS:
        gs = {"q": _win(q.reshape(B * Lq, C).to(dtype), kind, e), "k": _win(k.reshape(B * Lk, C).to(dtype), kind, e),
              "v": _win(v.reshape(B * Lk, C).to(dtype), kind, e), "o": _owin(B * Lq, C, dtype, kind, oq)}
        ops.attention(gs["q"].view, gs["k"].view, gs["v"].view, B, H, Lq, Lk, D, scale, out=gs["o"].view)
        _check_all(gs, f"attention {case} {kind}")
        outs[kind] = gs["o"].view.clone()
        _no_nan(outs[kind], kind)
        er, l2 = rel_err(outs[kind].float().cpu(), ref)
        assert er < (2e-5 if dtype == F32 else (2e-3 if dtype == F16 else 1.5e-2)), f"{kind}: {er:.3e} {l2:.3e}"
    for kind in KINDS:
        assert torch.equal(outs[kind], outs["dense"])


@pytest.mark.parametrize("case", [(3, 12, 77), (1, 1, 128), (1, 12, 2)], ids=["B3H12L77", "B1H1L128", "B1H12L2"])
def test_causal_attention_windows(cuda, case):
    """madm_causal_attention_fwd (f32, single-float accesses: any stride >= H * D): q / k / v / o in windows whose stride
    and offset are odd element counts; test_causal_attention's reference and bound (test_clip_gpu.py:69-89)."""
    from madm_amd import ops
    B, H, L = case
    D, C = 64, H * 64
    g = torch.Generator().manual_seed(L * 100 + H * 10 + B)
    q, k, v = [torch.randn(B * L, C, generator=g) for _ in range(3)]
    scale = D ** -0.5
    qq, kk, vv = (t.double().view(B, L, H, D).transpose(1, 2) for t in (q, k, v))
    s = (qq @ kk.transpose(-1, -2)) * scale + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
    ref = (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(B * L, C)
    outs = {}
    for kind in ["dense"] + KINDS:
        gs = {"q": _win(q, kind, 1), "k": _win(k, kind, 1), "v": _win(v, kind, 1), "o": _owin(B * L, C, F32, kind, 1)}
        ops.causal_attention(gs["q"].view, gs["k"].view, gs["v"].view, B, H, L, D, scale, out=gs["o"].view)
        _check_all(gs, f"causal attention {case} {kind}")
        outs[kind] = gs["o"].view.clone()
        _no_nan(outs[kind], kind)
        err = ((outs[kind].cpu().double() - ref).norm() / ref.norm()).item()
        assert err < 2e-6, err
    for kind in KINDS:
        assert torch.equal(outs[kind], outs["dense"])


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("case", [(2, 8, 64, 64, 40), (1, 8, 100, 77, 80), (1, 2, 70, 130, 64), (2, 8, 64, 64, 160)],
                         ids=lambda c: f"B{c[0]}H{c[1]}q{c[2]}k{c[3]}d{c[4]}")
def test_attention_backward_windows(cuda, dtype, case):
    """madm_attention_bwd: q / k / v / o / dout in windows (ldq .. lddo), dq / dk / dv in windows of their own (lddq ..
    lddv, 8-byte quantum), the f32 workspace behind canaries.  Rows of ATTN_BWD_CASES, test_attention_backward's tolerance
    (test_ops_gpu.py:1038); two launches without atomics: bit-identical to the dense run."""
    from madm_amd import ops
    from madm_amd._lib import lib, check, AttentionBwdArgs
    B, H, Lq, Lk, D = case
    q = _q(_gen((B, Lq, H, D), 1), dtype).requires_grad_(True)
    k = _q(_gen((B, Lk, H, D), 2), dtype).requires_grad_(True)
    v = _q(_gen((B, Lk, H, D), 3), dtype).requires_grad_(True)
    scale = D ** -0.5
    ref = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale)
    ref = ref.transpose(1, 2).reshape(B * Lq, H * D)
    do = _q(_gen((B * Lq, H * D), 4), dtype)
    ref.backward(do)
    C, e = H * D, _epc(dtype)
    gq = 8 // (16 // e)
    tol = 3e-5 if dtype == F32 else 2e-2
    od = ops.attention(q.detach().reshape(B * Lq, C).to(dtype).cuda(), k.detach().reshape(B * Lk, C).to(dtype).cuda(),
                       v.detach().reshape(B * Lk, C).to(dtype).cuda(), B, H, Lq, Lk, D, scale)
    outs = {}
    for kind in ["dense"] + KINDS:
        gs = {"q": _win(q.detach().reshape(B * Lq, C).to(dtype), kind, e), "k": _win(k.detach().reshape(B * Lk, C).to(dtype), kind, e),
              "v": _win(v.detach().reshape(B * Lk, C).to(dtype), kind, e), "o": _win(od, kind, e), "dout": _win(do.to(dtype), kind, e),
              "dq": _owin(B * Lq, C, dtype, kind, gq), "dk": _owin(B * Lk, C, dtype, kind, gq), "dv": _owin(B * Lk, C, dtype, kind, gq)}
        a = AttentionBwdArgs()
        a.dtype = _code(dtype)
        for f in ("q", "k", "v", "o", "dout", "dq", "dk", "dv"):
            setattr(a, f, gs[f].view.data_ptr())
            setattr(a, "ld" + ("do" if f == "dout" else f), gs[f].ld)
        a.B, a.H, a.Lq, a.Lk, a.D, a.scale = B, H, Lq, Lk, D, scale
        nbytes = lib.madm_attention_bwd_workspace_bytes(ctypes.byref(a))
        gs["workspace"], ws = _flat_out((nbytes // 4,), F32)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        check(lib.madm_attention_bwd(ctypes.byref(a), ops._stream()), "madm_attention_bwd")
        _check_all(gs, f"attention_bwd {case} {kind}")
        outs[kind] = [gs[f].view.clone() for f in ("dq", "dk", "dv")]
        for nm, got, want in zip(("dq", "dk", "dv"), outs[kind], (q.grad, k.grad, v.grad)):
            _no_nan(got, f"{nm} {kind}")
            er, l2 = rel_err(got.float().cpu(), want.reshape(got.shape[0], C))
            assert er < tol, f"{nm} {kind}: {er:.3e} {l2:.3e}"
    for kind in KINDS:
        for a_, b_ in zip(outs[kind], outs["dense"]):
            assert torch.equal(a_, b_)


# ----------------------------------------------------------------------------- norms
def _coff_win(rows, C, c_off, dtype, kind):
    """A window for an operand the kernel addresses at column c_off + c of a base pointer (the channel window of a
    concatenation): returns (guard, base pointer).  'dense' is the concatenation itself (ld = c_off + C)."""
    e = _epc(dtype)
    c0, ld = {"dense": (c_off, c_off + C), "tight": (c_off + e, c_off + C + 2 * e), "wide": (c_off + C, c_off + 3 * C)}[kind]
    g = Guarded(rows, C, dtype, ld=ld, c0=c0)
    return g, ctypes.c_void_p(g.view.data_ptr() - c_off * g.buf.element_size())


def _chsums(t, B, HW):
    from madm_amd import ops
    st = torch.zeros((B, t.shape[1], 2), dtype=torch.float64, device="cuda")
    ops.groupnorm_stats(t, B, HW, st)
    return st


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("shape", [(2, 320, 320, 8, 8), (1, 64, 128, 5, 3)], ids=["cpg20", "ragged"])
def test_groupnorm_apply_windows(cuda, dtype, shape):
    """madm_groupnorm_apply per source (c_off = 0 and c_off = C1 > 0; ldy, ldres) and madm_groupnorm_apply_cat (ldy) over a
    two-source concat: y and the residual in windows, x / statistics / gamma / beta behind canaries.  Shapes and
    tolerance of test_groupnorm_two_sources (test_ops_gpu.py:399); the residual form is detectron2's relu(norm + shortcut)
    with the same bound.  Pure per-element arithmetic: bit-identical to the dense run."""
    from madm_amd import ops
    B, C1, C2, H, W = shape
    HW, Ct = H * W, C1 + C2
    xs = [_q(_gen((B, C1, H, W), 1) * 1.5 + 0.3, dtype), _q(_gen((B, C2, H, W), 2) * 0.7 - 0.2, dtype)]
    gamma, beta = _gen((Ct,), 3), _gen((Ct,), 4)
    res = _q(_gen((B, Ct, H, W), 5), dtype)
    gn = F.group_norm(torch.cat(xs, 1), 32, gamma, beta, eps=1e-5)
    refs = {"silu": F.silu(gn), "res_relu": F.relu(gn + res)}
    toks = [to_tokens(x, dtype) for x in xs]
    sts = [_chsums(t, B, HW) for t in toks]
    tol = 1e-5 if dtype == F32 else 1e-2
    outs = {}
    for kind in ["dense"] + KINDS:
        fixed = {}
        fixed["x1"], x1v = _vec(toks[0], post=1024)
        fixed["x2"], x2v = _vec(toks[1], post=1024)
        fixed["sums1"], s1v = _vec(sts[0])
        fixed["sums2"], s2v = _vec(sts[1])
        fixed["gamma"], gv = _vec(gamma)
        fixed["beta"], bv = _vec(beta)
        for variant in ("silu", "res_relu"):
            act = ops.ACT_SILU if variant == "silu" else ops.ACT_RELU
            got = []
            for xv, C, off in ((x1v, C1, 0), (x2v, C2, C1)):
                gy, ybase = _coff_win(B * HW, C, off, dtype, kind)
                gs = dict(fixed, y=gy)
                rbase, ldres = None, 0
                if variant == "res_relu":
                    gs["residual"], rbase = _coff_win(B * HW, C, off, dtype, "wide" if kind == "tight" else kind)
                    gs["residual"].load(to_tokens(res[:, off:off + C], dtype))
                    ldres = gs["residual"].ld
                _call("madm_groupnorm_apply", _code(dtype), _p(xv), ybase, gy.ld, B, HW, C, off, Ct, 32, _p(s1v), C1, _p(s2v),
                      _p(gv), _p(bv), 1e-5, act, rbase, ldres)
                _check_all(gs, f"groupnorm_apply {variant} c_off={off} {kind}")
                got.append(gy.view.clone())
            full = torch.cat(got, 1)
            _no_nan(full, f"{variant} {kind}")
            e_, l2 = rel_err(from_tokens(full, B, H, W), refs[variant])
            assert e_ < tol, f"{variant} {kind}: {e_:.3e} {l2:.3e}"
            outs[(variant, kind)] = full
        gy = _owin(B * HW, Ct, dtype, kind, _epc(dtype))
        _call("madm_groupnorm_apply_cat", _code(dtype), _p(x1v), _p(x2v), _p(gy.view), gy.ld, B, HW, C1, C2, 32, _p(s1v), _p(s2v),
              _p(gv), _p(bv), 1e-5, ops.ACT_SILU)
        _check_all(dict(fixed, y=gy), f"groupnorm_apply_cat {kind}")
        e_, l2 = rel_err(from_tokens(gy.view, B, H, W), refs["silu"])
        assert e_ < tol, f"cat {kind}: {e_:.3e} {l2:.3e}"
        outs[("cat", kind)] = gy.view.clone()
    for kind in KINDS:
        for variant in ("silu", "res_relu", "cat"):
            assert torch.equal(outs[(variant, kind)], outs[(variant, "dense")]), (variant, kind)


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("case", [(1, [64], 11, 19, "relu"), (2, [128, 64], 8, 16, "silu"), (2, [1280, 640], 4, 6, "silu")],
                         ids=["relu_ragged", "concat", "concat_straddle"])
def test_groupnorm_backward_windows(cuda, dtype, case):
    """madm_groupnorm_bwd_sums / _apply: dy (lddy) and dres (lddres) in windows read at column c_off + c; dx, the f64 sums
    and dgamma / dbeta behind canaries.  Rows and tolerance of test_groupnorm_backward (test_ops_gpu.py:713); dres adds the
    skip path's gradient.  The sums are f64 atomics: the windowed run is held to the tolerance."""
    from madm_amd import ops
    B, cins, H, W, act = case
    HW, Ct = H * W, sum(cins)
    xs = [_q(_gen((B, c, H, W), 50 + i) * (1.0 + i) + 0.5 * i, dtype).requires_grad_(True) for i, c in enumerate(cins)]
    gamma = (1.0 + 0.2 * _gen((Ct,), 2)).requires_grad_(True)
    beta = (0.3 * _gen((Ct,), 3)).requires_grad_(True)
    y = F.group_norm(torch.cat(xs, 1), 32, gamma, beta, eps=1e-5)
    y = F.silu(y) if act == "silu" else (F.relu(y) if act == "relu" else y)
    dy = _q(_gen(tuple(y.shape), 4), dtype)
    dres = _q(_gen(tuple(y.shape), 6), dtype)
    y.backward(dy)
    toks = [to_tokens(x.detach(), dtype) for x in xs]
    sts = [_chsums(t, B, HW) for t in toks]
    code = ops._act_code(act=act)
    tol = 3e-5 if dtype == F32 else 1.5e-2
    C1 = cins[0]
    for kind in ["dense"] + KINDS:
        gs = {}
        gs["dy"], dyb = _coff_win(B * HW, Ct, 0, dtype, kind)
        gs["dy"].load(to_tokens(dy, dtype))
        gs["dres"], drb = _coff_win(B * HW, Ct, 0, dtype, "wide" if kind == "tight" else kind)
        gs["dres"].load(to_tokens(dres, dtype))
        gs["gamma"], gv = _vec(gamma.detach())
        gs["beta"], bv = _vec(beta.detach())
        gs["bsums"], bs = _vec(torch.zeros((B, Ct, 2), dtype=torch.float64))
        gs["dgamma"], dg = _vec(torch.zeros(Ct))
        gs["dbeta"], db = _vec(torch.zeros(Ct))
        s2 = _p(sts[1]) if len(xs) > 1 else None
        off = 0
        for t in toks:
            _call("madm_groupnorm_bwd_sums", _code(dtype), _p(t), dyb, gs["dy"].ld, B, HW, t.shape[1], off, Ct, 32, _p(sts[0]), C1, s2,
                  _p(gv), _p(bv), 1e-5, code, _p(bs))
            off += t.shape[1]
        off = 0
        for i, (t, x) in enumerate(zip(toks, xs)):
            gs[f"dx{i}"], dx = _flat_out(tuple(t.shape), dtype)
            _call("madm_groupnorm_bwd_apply", _code(dtype), _p(t), dyb, gs["dy"].ld, _p(dx), B, HW, t.shape[1], off, Ct, 32,
                  _p(sts[0]), C1, s2, _p(gv), _p(bv), 1e-5, code, _p(bs), _p(dg), _p(db), drb, gs["dres"].ld)
            torch.cuda.synchronize()
            _no_nan(dx, f"dx{i} {kind}")
            want = x.grad + dres[:, off:off + t.shape[1]]
            e_, l2 = rel_err(from_tokens(dx, B, H, W), want)
            assert e_ < tol, f"dx{i} {kind}: {e_:.3e} {l2:.3e}"
            off += t.shape[1]
        _check_all(gs, f"groupnorm_bwd {kind}")
        assert rel_err(dg.cpu(), gamma.grad)[0] < tol and rel_err(db.cpu(), beta.grad)[0] < tol, kind


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
def test_row_kernels_windows(cuda, dtype):
    """madm_layernorm_fwd / madm_layernorm_bwd (dense rows: the canary starts at element M * C), madm_softmax_rows (lds, ldp),
    madm_geglu_bwd, madm_silu_bwd, madm_add, madm_colsum (ldx).  References and bounds: test_layernorm (1e-5 / 1e-2,
    test_ops_gpu.py:966), test_layernorm_backward (3e-5 / 1.5e-2, :739), the softmax line of
    test_vae_attention_gemm_path_equals_flash_path (1e-6 / 5e-3, :1073), test_geglu_backward and test_silu_backward (1e-5,
    :931, :849); madm_add is one rounded sum, colsum the bias gradient of test_conv2d_wgrad (2e-5, :630)."""
    from madm_amd import ops
    e = _epc(dtype)
    lo = dtype != F32
    # LayerNorm forward and backward (+ dres), M = 70 rows of 320 (test_layernorm), ragged against the 4-row blocks
    M, C = 70, 320
    x = _q(_gen((M, C), 1) * 3.0 - 1.0, dtype).requires_grad_(True)
    gamma, beta = _gen((C,), 2).requires_grad_(True), _gen((C,), 3).requires_grad_(True)
    y = F.layer_norm(x, (C,), gamma, beta, eps=1e-5)
    dy, dres = _q(_gen((M, C), 5), dtype), _q(_gen((M, C), 6), dtype)
    y.backward(dy)
    gs = {}
    gs["x"], xv = _vec(x.detach().to(dtype), post=1024)
    gs["gamma"], gv = _vec(gamma.detach())
    gs["beta"], bv = _vec(beta.detach())
    gs["y"], yv = _flat_out((M, C), dtype)
    _call("madm_layernorm_fwd", _code(dtype), _p(xv), _p(yv), M, C, _p(gv), _p(bv), 1e-5)
    gs["dy"], dyv = _vec(dy.to(dtype), post=1024)
    gs["dres"], drv = _vec(dres.to(dtype), post=1024)
    gs["dx"], dxv = _flat_out((M, C), dtype)
    gs["dgamma"], dgv = _vec(torch.zeros(C))
    gs["dbeta"], dbv = _vec(torch.zeros(C))
    _call("madm_layernorm_bwd", _code(dtype), _p(xv), _p(dyv), _p(dxv), M, C, _p(gv), 1e-5, _p(dgv), _p(dbv), _p(drv))
    _check_all(gs, "layernorm")
    _no_nan(yv, "layernorm"), _no_nan(dxv, "layernorm_bwd")
    assert rel_err(yv.float().cpu(), y.detach())[0] < (1e-2 if lo else 1e-5)
    t = 1.5e-2 if lo else 3e-5
    assert rel_err(dxv.float().cpu(), x.grad + dres)[0] < t
    assert rel_err(dgv.cpu(), gamma.grad)[0] < t and rel_err(dbv.cpu(), beta.grad)[0] < t
    # row softmax: f32 logits [37][256] (lds) -> dtype [37][256] (ldp)
    s = _gen((37, 256), 9) * 5
    ref = torch.softmax(s * 0.3, -1)
    outs = {}
    for kind in ["dense"] + KINDS:
        gi, go = _win(s, kind, 4), _owin(37, 256, dtype, kind, 4)
        _call("madm_softmax_rows", _code(dtype), _p(gi.view), _p(go.view), 37, 256, gi.ld, go.ld, 0.3)
        _check_all({"s": gi, "p": go}, f"softmax_rows {kind}")
        outs[kind] = go.view.clone()
        _no_nan(outs[kind], f"softmax_rows {kind}")
        assert rel_err(outs[kind].float().cpu(), ref)[0] < (5e-3 if lo else 1e-6), kind
    assert torch.equal(outs["tight"], outs["dense"]) and torch.equal(outs["wide"], outs["dense"])
    # GEGLU / SiLU backward (their dense tests run f32 only: so does this part), add: dense, n not a multiple of the block
    Mg, N = 37, 1288
    gdt = F32
    pre = _gen((Mg, 2 * N), 1).requires_grad_(True)
    dout = _gen((Mg, N), 2)
    (pre[:, 0::2] * F.gelu(pre[:, 1::2])).backward(dout)
    gs = {}
    gs["pre"], pv = _vec(pre.detach(), post=1024)
    gs["dout"], dv = _vec(dout, post=1024)
    gs["dpre"], dp = _flat_out((Mg, 2 * N), gdt)
    _call("madm_geglu_bwd", _code(gdt), _p(pv), _p(dv), _p(dp), Mg, 2 * N)
    xs_ = _gen((37, 1288), 1).requires_grad_(True)
    dys = _gen((37, 1288), 2)
    F.silu(xs_).backward(dys)
    gs["sx"], sxv = _vec(xs_.detach(), post=1024)
    gs["sdy"], sdv = _vec(dys, post=1024)
    gs["sdx"], sdx = _flat_out((37, 1288), gdt)
    _call("madm_silu_bwd", _code(gdt), _p(sxv), _p(sdv), _p(sdx), 37 * 1288)
    # a + b: ONE correctly rounded sum of two values of the dtype -- exact in torch
    a_, b_ = _q(_gen((37, 1288), 3), dtype), _q(_gen((37, 1288), 4), dtype)
    gs["a"], aav = _vec(a_.to(dtype), post=1024)
    gs["b"], abv = _vec(b_.to(dtype), post=1024)
    gs["sum"], av = _flat_out((37, 1288), dtype)
    _call("madm_add", _code(dtype), _p(aav), _p(abv), _p(av), 37 * 1288)
    _check_all(gs, "geglu_bwd / silu_bwd / add")
    assert rel_err(dp.cpu(), pre.grad)[0] < 1e-5
    assert rel_err(sdx.cpu(), xs_.grad)[0] < 1e-5
    assert torch.equal(av.cpu(), (a_ + b_).to(dtype))
    # column sums over a row-strided window: f32 [B][C] accumulated into; inputs exact in f32, 35 f32 additions per column: the
    # bias-gradient bound of test_conv2d_wgrad (2e-5, test_ops_gpu.py:630), which the same sums meet there
    B, HW, Cc = 3, 35, 8 * e
    xc = _q(_gen((B * HW, Cc), 7), dtype)
    for kind in ["dense"] + KINDS:
        gi = _win(xc.to(dtype), kind, e)
        go, ov = _flat_out((B, Cc), F32)
        ov.zero_()
        _call("madm_colsum", _code(dtype), _p(gi.view), gi.ld, B, HW, Cc, _p(ov))
        _check_all({"x": gi, "out": go}, f"colsum {kind}")
        _no_nan(ov, f"colsum {kind}")
        assert rel_err(ov.cpu(), xc.reshape(B, HW, Cc).sum(1))[0] < 2e-5, kind


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
def test_gradient_reshaping_kernels_are_contained(cuda, dtype):
    """madm_zero_insert2x / madm_sumpool2x2 (dense tensors: the canary starts right behind the last element) on ragged
    odd-sized maps; exact data movement / sums of four rounded values stated in torch."""
    B, OH, OW, C = 2, 5, 7, 4 * _epc(dtype)
    for (H, W) in ((10, 14), (9, 13)):                     # stride-2 conv with and without a last odd row / column
        oh, ow = (H + 1) // 2, (W + 1) // 2
        d = _q(_gen((B, C, oh, ow), 1), dtype)
        gs = {}
        gs["x"], xv = _vec(to_tokens(d, dtype), post=1024)
        gs["y"], yv = _flat_out((B * H * W, C), dtype)
        _call("madm_zero_insert2x", _code(dtype), _p(xv), _p(yv), B, oh, ow, H, W, C)
        _check_all(gs, "zero_insert2x")
        ref = torch.zeros((B, C, H, W))
        ref[:, :, 0::2, 0::2] = d
        assert torch.equal(from_tokens(yv, B, H, W), ref)
    x = _q(_gen((B, C, 2 * OH, 2 * OW), 2), dtype)
    gs = {}
    gs["x"], xv = _vec(to_tokens(x, dtype), post=1024)
    gs["y"], yv = _flat_out((B * OH * OW, C), dtype)
    _call("madm_sumpool2x2", _code(dtype), _p(xv), _p(yv), B, OH, OW, C)
    _check_all(gs, "sumpool2x2")
    # no dense test of this kernel exists to take a tolerance from, so none is introduced: the kernel's own statement -- the
    # four values added in f32 in the order (0, 0), (0, 1), (1, 0), (1, 1), ONE rounding to the dtype -- holds bit for bit
    ref = (((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + x[:, :, 1::2, 0::2]) + x[:, :, 1::2, 1::2]).to(dtype).float()
    assert torch.equal(from_tokens(yv, B, OH, OW), ref)


# ----------------------------------------------------------------------------- glue kernels of the forward
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_stem_conv3x3_windows(cuda, dtype):
    """madm_stem_conv3x3: out in a window (ldo; a multiple of 8 and 16-byte aligned in the 16-bit modes: the matrix-pipe
    kernel stores 16-byte chunks), the f64 statistics and the range probe behind canaries.  Shape 'ragged' of
    test_stem_conv3x3, its reference on rounded operands and its bounds (test_ops_gpu.py:235-239).
    'ld4' is the contract's own minimum, ldo % 4 == 0 with ldo % 8 == 4 (ldo = 140, 16-byte aligned base, rows that keep
    8 bytes only): there the 16-bit modes fall back to the exact-f32 FMA kernel with its 8-byte stores.  That kernel does
    not round the operands, so by design its bits differ from the matrix-pipe runs; it is held to the statement
    test_stem_conv3x3 makes for it (the unrounded reference, test_ops_gpu.py:247-248) and to bit-identity with the SAME
    kernel on a dense tensor (MADM_STEM_KERNEL=1, as that test selects it).  In f32 every layout runs the FMA kernel."""
    B, H, W = 1, 37, 133
    img = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(5))
    w = _gen((128, 3, 3, 3), 6) / math.sqrt(27)
    bias = _gen((128,), 7)
    mean, std = 0.5, 0.5
    ref0 = F.conv2d((img - mean) / std, w, bias, padding=1)
    ref = F.conv2d(_q((img - mean) / std, dtype), _q(w, dtype), bias, padding=1)
    wT = w.permute(2, 3, 1, 0).reshape(27, 128).contiguous()
    e = _epc(dtype)
    lays = {"dense": (layout("dense", 128, e), False), "tight": (layout("tight", 128, e), False),
            "wide": (layout("wide", 128, e), False), "ld4": ((140, 8), True)}
    if dtype != F32:
        lays["dense_fma"] = (layout("dense", 128, e), True)
    outs = {}
    for kind, ((ld, c0), fma) in lays.items():
        gs = {}
        gs["img"], iv = _vec(img, post=1024)
        gs["wT"], wv = _vec(wT)
        gs["bias"], bv = _vec(bias)
        gs["stats"], st = _vec(torch.zeros((B, 128, 2), dtype=torch.float64))
        gs["minmax"], mm = _vec(torch.tensor([float("inf"), float("-inf")]))
        gs["out"] = Guarded(B * H * W, 128, dtype, ld=ld, c0=c0)
        assert gs["out"].view.data_ptr() % 16 == 0 and ld % 4 == 0
        if kind == "dense_fma":
            os.environ["MADM_STEM_KERNEL"] = "1"
        try:
            _call("madm_stem_conv3x3", _code(dtype), _p(iv), _p(wv), _p(bv), _p(gs["out"].view), ld, B, H, W, 128, mean, std,
                  _p(st), _p(mm))
        finally:
            os.environ.pop("MADM_STEM_KERNEL", None)
        _check_all(gs, f"stem_conv3x3 {kind}")
        outs[kind] = gs["out"].view.clone()
        _no_nan(outs[kind], kind)
        r = ref0 if fma else ref
        er, l2 = rel_err(from_tokens(outs[kind], B, H, W), r)
        assert er < {F32: 2e-6, BF16: 6e-3, F16: 8e-4}[dtype], f"{kind}: {er:.3e} {l2:.3e}"
        sums = st.float().cpu()
        # the sums are taken of the f32 accumulators: each kernel's against its own exact statement
        assert rel_err(sums[..., 0], r.sum((2, 3)))[0] < 1e-4 and rel_err(sums[..., 1], (r ** 2).sum((2, 3)))[0] < 1e-4
        lo, hi = mm.tolist()
        x = (img - mean) / std
        assert abs(lo - float(x.min())) < 1e-6 and abs(hi - float(x.max())) < 1e-6
    assert torch.equal(outs["tight"], outs["dense"]) and torch.equal(outs["wide"], outs["dense"])
    assert torch.equal(outs["ld4"], outs["dense" if dtype == F32 else "dense_fma"])


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
def test_glue_kernels_windows(cuda, dtype):
    """The layout / conditioning kernels of LdmDiffusers.forward with every output behind canaries and every strided
    operand in a window: image_to_nhwc / image_to_im2col3x3 / nchw_f32_to_nhwc (the zero padding up to Cpad / Kpad belongs
    to the output and is exactly zero), nhwc_to_nchw_f32 (ld; only channels [c_off, c_off + C) of the NCHW tensor are
    written), copy_columns (lds, ldd), latents_add_noise (ldm), timestep_embedding, silu, rows_to_f32, cast_from_f32,
    clamp_f32 at sizes that are no multiple of 4.  Expressions and bounds of test_glue_kernels (test_ops_gpu.py:1093-1145)."""
    from madm_amd import ops
    kt, e = ops.k_tile(dtype), _epc(dtype)
    lo = dtype != F32
    Bi, Hi, Wi = 2, 15, 23
    img = torch.rand((Bi, 3, Hi, Wi), generator=torch.Generator().manual_seed(1))
    ref = (img - 0.5) / 0.5
    gs = {}
    # the range probe reads the image as float4 and its last numel % 4 = 2 elements singly: the canary starts right behind them
    assert img.numel() % 4 == 2
    gs["img"], iv = _vec(img, post=1024)
    gs["nhwc"], t = _flat_out((Bi * Hi * Wi, kt), dtype)
    gs["minmax1"], mm1 = _vec(torch.tensor([float("inf"), float("-inf")]))
    _call("madm_image_to_nhwc", _code(dtype), _p(iv), _p(t), Bi, 3, Hi, Wi, kt, 0.5, 0.5, _p(mm1))
    got = from_tokens(t, Bi, Hi, Wi)
    assert rel_err(got[:, :3], ref)[0] < (5e-3 if lo else 1e-6) and got[:, 3:].abs().max().item() == 0.0
    gs["im2col"], cols = _flat_out((Bi * Hi * Wi, kt), dtype)
    gs["minmax2"], mm2 = _vec(torch.tensor([float("inf"), float("-inf")]))
    _call("madm_image_to_im2col3x3", _code(dtype), _p(iv), _p(cols), Bi, Hi, Wi, kt, 0.5, 0.5, _p(mm2))
    unf = F.unfold(ref, 3, padding=1).reshape(Bi, 3, 9, -1).permute(0, 3, 2, 1).reshape(Bi * Hi * Wi, 27)
    cc = cols.float().cpu()
    assert rel_err(cc[:, :27], unf)[0] < (5e-3 if lo else 1e-6) and cc[:, 27:].abs().max().item() == 0.0
    for mm in (mm1, mm2):          # the range probe's bound of test_stem_conv3x3 (test_ops_gpu.py:251)
        assert abs(mm[0].item() - float(ref.min())) < 1e-6 and abs(mm[1].item() - float(ref.max())) < 1e-6
    gs["nhwc2"], t2 = _flat_out((Bi * Hi * Wi, kt), dtype)
    _call("madm_nchw_f32_to_nhwc", _code(dtype), _p(iv), _p(t2), Bi, 3, Hi * Wi, kt)
    g2 = from_tokens(t2, Bi, Hi, Wi)
    assert rel_err(g2[:, :3], img)[0] < (5e-3 if lo else 1e-6) and g2[:, 3:].abs().max().item() == 0.0
    _check_all(gs, "image layout kernels")
    # nhwc -> nchw: a row-strided source, channels [c_off, c_off + C) of a 7-channel f32 tensor; the others stay untouched
    HW, C, c_off, Ct = Hi * Wi, 3, 2, 7
    src = _q(_gen((Bi * HW, 37), 3), dtype).to(dtype)
    for kind in ["dense"] + KINDS:
        gi = _win(src, kind, 1)
        go = Guarded(Bi * Ct, HW, F32, ld=HW)          # (the window itself starts out as canaries too)
        _call("madm_nhwc_to_nchw_f32", _code(dtype), _p(gi.view), gi.ld, _p(go.view), Bi, C, c_off, Ct, HW)
        _check_all({"x": gi, "out": go}, f"nhwc_to_nchw {kind}")
        o = go.view.view(Bi, Ct, HW)
        assert torch.equal(o[:, c_off:c_off + C].cpu(), src.float()[:, :C].reshape(Bi, HW, C).permute(0, 2, 1)), kind
        mask = torch.ones(Ct, dtype=torch.bool)
        mask[c_off:c_off + C] = False
        assert bool((o.view(torch.int32)[:, mask] == go.pattern).all()), f"nhwc_to_nchw {kind}: wrote outside its channels"
    # copy_columns: single elements, any stride (tight: one element)
    rows, Cc = 131, 4
    a = _q(_gen((rows, Cc), 4), dtype).to(dtype)
    for kind in ["dense"] + KINDS:
        gi, go = _win(a, kind, 1), _owin(rows, Cc, dtype, "wide" if kind == "tight" else kind, 1)
        _call("madm_copy_columns", _code(dtype), _p(gi.view), gi.ld, _p(go.view), go.ld, rows, Cc)
        _check_all({"src": gi, "dst": go}, f"copy_columns {kind}")
        assert torch.equal(go.view, gi.view), kind
    # latent scaling + noise mixing: moments in a window (ldm)
    B, h, w = 2, 7, 9
    mom = _q(_gen((B * h * w, 8), 3), dtype)
    noise = _gen((1, 4, h, w), 4)
    ac = torch.linspace(0.999, 0.01, 1000)
    tsb = torch.tensor([0, 60], dtype=torch.int64)
    lat_ref = mom[:, :4].reshape(B, h, w, 4).permute(0, 3, 1, 2) * 0.18215
    noisy_ref = ac.sqrt()[tsb][:, None, None, None] * lat_ref + (1 - ac).sqrt()[tsb][:, None, None, None] * noise
    for kind in ["dense"] + KINDS:
        gs = {"moments": _win(mom.to(dtype), kind, 1)}
        gs["noise"], nv = _vec(noise)
        gs["sqrt_ac"], sa = _vec(ac.sqrt())
        gs["sqrt_1mac"], sn = _vec((1 - ac).sqrt())
        gs["timesteps"], tv = _vec(tsb)
        gs["latents"], lat = _flat_out((B, 4, h, w), F32)
        gs["noisy"], noisy = _flat_out((B * h * w, kt), dtype)
        _call("madm_latents_add_noise", _code(dtype), _p(gs["moments"].view), gs["moments"].ld, 0.18215, _p(nv), _p(sa), _p(sn), _p(tv),
              _p(lat), _p(noisy), B, h * w, kt)
        _check_all(gs, f"latents_add_noise {kind}")
        assert rel_err(lat.cpu(), lat_ref)[0] < 1e-6
        gotn = from_tokens(noisy, B, h, w)
        assert rel_err(gotn[:, :4], noisy_ref)[0] < (5e-3 if lo else 1e-6) and gotn[:, 4:].abs().max().item() == 0.0
    # flat kernels, n = 2 * 1283 (no multiple of 4)
    n = 2 * 1283
    gs = {}
    ts = torch.tensor([0, 60, 999], dtype=torch.int64)
    half = 160
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    arg = ts[:, None].float() * freqs[None]
    gs["ts"], tsv = _vec(ts)
    gs["freqs"], fv = _vec(freqs)
    gs["emb"], emb = _flat_out((3, 320), dtype)
    _call("madm_timestep_embedding", _code(dtype), _p(tsv), _p(fv), _p(emb), 3, 320)
    x = _q(_gen((2, 1283), 1), dtype)
    add = _gen((2, 1283), 2)
    gs["x"], xv = _vec(x.to(dtype))
    gs["add"], addv = _vec(add)
    gs["silu"], sv = _flat_out((n,), dtype)
    _call("madm_silu", _code(dtype), _p(xv), _p(sv), n)
    gs["rows"], rv = _flat_out((n,), F32)
    _call("madm_rows_to_f32", _code(dtype), _p(xv), _p(addv), _p(rv), n)
    gs["cast"], cv = _flat_out((n,), dtype)
    _call("madm_cast_from_f32", _code(dtype), _p(addv), _p(cv), n)
    gs["clamp"], clv = _flat_out((n,), F32)
    _call("madm_clamp_f32", _p(addv), _p(clv), n, -1.0, 1.0)
    _check_all(gs, "flat glue kernels")
    assert (emb.float().cpu() - torch.cat([torch.cos(arg), torch.sin(arg)], -1)).abs().max().item() < (5e-3 if lo else 2e-5)
    assert rel_err(sv.float().cpu(), F.silu(x).reshape(-1))[0] < (5e-3 if lo else 1e-6)
    assert rel_err(rv.cpu(), (x + add).reshape(-1))[0] < 1e-6
    assert torch.equal(cv.cpu(), add.reshape(-1).to(dtype)) and torch.equal(clv.cpu(), add.reshape(-1).clamp(-1.0, 1.0))


def test_clip_kernels_are_contained(cuda):
    """madm_token_embedding and madm_quick_gelu with their outputs behind canaries; test_quick_gelu's expression and bound
    (test_clip_gpu.py:109-113), the embedding is one f32 sum per element (exact)."""
    g = torch.Generator().manual_seed(9)
    N, L, C, vocab = 3, 7, 33, 50
    ids = torch.randint(0, vocab, (N, L), generator=g)
    tok, pos = torch.randn(vocab, C, generator=g), torch.randn(9, C, generator=g)
    gs = {}
    gs["ids"], iv = _vec(ids)
    gs["tok"], tv = _vec(tok)
    gs["pos"], pv = _vec(pos)
    gs["out"], ov = _flat_out((N * L, C), F32)
    _call("madm_token_embedding", _p(iv), N, L, _p(tv), vocab, _p(pv), 9, C, _p(ov))
    for dtype in DT3:
        x = (6 * torch.randn(100003, generator=g)).to(dtype)
        gs[f"x{dtype}"], xv = _vec(x, post=1024)
        gs[f"y{dtype}"], yv = _flat_out((100003,), dtype)
        _call("madm_quick_gelu", _code(dtype), _p(xv), _p(yv), 100003)
        torch.cuda.synchronize()
        xf = x.float()
        refq = (xf * torch.sigmoid(1.702 * xf)).to(dtype)
        if dtype == F32:
            assert torch.allclose(yv.cpu(), refq, rtol=2e-6, atol=1e-7)
        else:
            assert torch.allclose(yv.float().cpu(), refq.float(), rtol=1e-2, atol=1e-3)
    _check_all(gs, "token_embedding / quick_gelu")
    assert torch.equal(ov.cpu(), (tok[ids] + pos[:L][None]).reshape(N * L, C))


# ----------------------------------------------------------------------------- projection / head / evaluation kernels
@pytest.mark.parametrize("dtype", DT2, ids=ID2)
def test_spatial_kernels_windows(cuda, dtype):
    """madm_resize_bilinear (ldi, ldo), madm_resize_bilinear_nchw_f32, madm_scale_pad_crop_nchw_f32 with y1 / x1 != 0 (crop
    reaching over the border), madm_slide_merge, madm_tanh_gate, madm_argmax_nchw_f32, madm_confusion_matrix: windows for
    the strided operands, canaries behind every dense output.  Expressions and bounds of test_spatial_kernels
    (test_eval_gpu.py:26-94) and of the merge line of test_sliding_window_backbone (:264-270)."""
    e = _epc(dtype)
    lo = dtype != F32
    x = _q(_gen((2, 64, 5, 7), 1), dtype)
    for (oh, ow) in ((20, 28), (3, 4), (16, 9)):
        ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
        outs = {}
        for kind in ["dense"] + KINDS:
            gi, go = _win(to_tokens(x, dtype), kind, e), _owin(2 * oh * ow, 64, dtype, kind, e)
            _call("madm_resize_bilinear", _code(dtype), _p(gi.view), gi.ld, _p(go.view), go.ld, 2, 5, 7, oh, ow, 64)
            _check_all({"in": gi, "out": go}, f"resize_bilinear {oh}x{ow} {kind}")
            outs[kind] = go.view.clone()
            _no_nan(outs[kind], kind)
            assert rel_err(from_tokens(outs[kind], 2, oh, ow), ref)[0] < (8e-3 if lo else 1e-6)
        assert torch.equal(outs["tight"], outs["dense"]) and torch.equal(outs["wide"], outs["dense"])
    if dtype != F32:
        return                      # the rest is f32 / integer work, run once
    img = torch.rand((2, 3, 30, 50), generator=torch.Generator().manual_seed(2))
    gs = {}
    gs["img"], iv = _vec(img, post=1024)
    gs["resized"], rz = _flat_out((2, 3, 61, 67), F32)
    _call("madm_resize_bilinear_nchw_f32", _p(iv), _p(rz), 6, 30, 50, 61, 67)
    gs["padded"], pd = _flat_out((2, 3, 40, 61), F32)
    _call("madm_scale_pad_crop_nchw_f32", _p(iv), _p(pd), 6, 30, 50, 5, 7, 40, 61, 1 / 255.0)
    _check_all(gs, "resize_bilinear_nchw / scale_pad_crop")
    assert rel_err(rz.cpu(), F.interpolate(img, size=(61, 67), mode="bilinear", align_corners=False))[0] < 1e-6
    want = torch.zeros((2, 3, 40, 61))
    want[:, :, :25, :43] = img[:, :, 5:, 7:] * (1 / 255.0)
    assert torch.equal(pd.cpu(), want)
    # sliding-window merge
    for dt in DT2:
        w = torch.randn(3 * 2 * 4 * 64, 64, generator=torch.Generator().manual_seed(3))
        gs = {}
        gs["win"], wv = _vec(w.to(dt), post=1024)
        gs["out"], mv = _flat_out((2 * 4 * 128, 64), dt)
        x1 = (ctypes.c_int * 3)(0, 32, 64)
        _call("madm_slide_merge", _code(dt), _p(wv), _p(mv), 3, 2, 4, 64, 128, 64, x1)
        _check_all(gs, "slide_merge")
        wq = w.to(dt).float().reshape(3, 2, 4, 64, 64)
        ref = torch.zeros(2, 4, 128, 64)
        cnt = torch.zeros(1, 1, 128, 1)
        for k, xo in enumerate([0, 32, 64]):
            ref[:, :, xo:xo + 64] += wq[k]
            cnt[:, :, xo:xo + 64] += 1
        assert rel_err(mv.float().cpu().reshape(2, 4, 128, 64), ref / cnt)[0] < (1e-6 if dt == F32 else 8e-3)
    # tanh gates, argmax, confusion matrix
    n = 77 * 768 + 3
    a1, x1_, a2, x2 = torch.rand(n), _gen((n,), 7), torch.rand(n), _gen((n,), 8)
    gs = {}
    ptrs = []
    for nm, t in (("a1", a1), ("x1", x1_), ("a2", a2), ("x2", x2)):
        gs[nm], v = _vec(t, post=1024)
        ptrs.append(v)
    gs["gate"], gv = _flat_out((3, n), F32)
    _call("madm_tanh_gate", _p(ptrs[0]), _p(ptrs[1]), _p(ptrs[2]), _p(ptrs[3]), _p(gv), n, 3)
    lg = _gen((2, 11, 9, 13), 9)
    lg[0, 3, 2, 2] = lg[0, 7, 2, 2] = 100.0
    gs["logits"], lv = _vec(lg, post=1024)
    gs["labels"], lab = _flat_out((2, 9, 13), torch.int64)
    _call("madm_argmax_nchw_f32", _p(lv), _p(lab), 2, 11, 9 * 13)
    K = 11
    gt = torch.randint(0, K, (2, 9, 13), generator=torch.Generator().manual_seed(5))
    gt[0, :2] = 255
    gs["gt"], gtv = _vec(gt)
    gs["conf"], conf = _flat_out((K + 1, K + 1), torch.int64)
    conf.zero_()
    _call("madm_confusion_matrix", _p(lab), _p(gtv), 2 * 9 * 13, K, 255, _p(conf))
    _check_all(gs, "tanh_gate / argmax / confusion_matrix")
    assert rel_err(gv.cpu(), (torch.tanh(a1) * x1_ + torch.tanh(a2) * x2).repeat(3, 1))[0] < 1e-6
    assert torch.equal(lab.cpu(), lg.argmax(dim=1)) and lab[0, 2, 2].item() == 3
    pred = lg.argmax(dim=1).reshape(-1)
    g_ = torch.where(gt.reshape(-1) == 255, torch.full_like(pred, K), gt.reshape(-1))
    want = torch.bincount((K + 1) * pred + g_, minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    assert torch.equal(conf.cpu(), want)


@pytest.mark.parametrize("dtype", DT2, ids=ID2)
@pytest.mark.parametrize("kern", ["1", "2", "3", "4"])
def test_dwconv3x3_windows(cuda, dtype, kern):
    """madm_dwconv3x3 with each kernel variant forced (MADM_DWCONV_KERNEL, as test_spatial_kernels forces them): y in a
    window (ldy), x / weights / affine behind canaries; its ragged map, dilations and bound (test_eval_gpu.py:66-85)."""
    from madm_amd import ops
    C2, e = 128, _epc(dtype)
    xc = _q(_gen((2, C2, 35, 83), 14), dtype)
    w2 = _gen((C2, 1, 3, 3), 15) / 3
    s2, t2 = 1 + 0.1 * _gen((C2,), 16), 0.1 * _gen((C2,), 17)
    for dil in (1, 6, 12, 18):
        ref = F.relu(F.conv2d(xc, w2, None, padding=dil, dilation=dil, groups=C2) * s2[None, :, None, None] + t2[None, :, None, None])
        outs = {}
        for kind in ["dense"] + KINDS:
            gs = {}
            gs["x"], xv = _vec(to_tokens(xc, dtype), post=1024)
            gs["w"], wv = _vec(w2.reshape(C2, 9).t().contiguous())
            gs["scale"], sv = _vec(s2)
            gs["shift"], tv = _vec(t2)
            gs["y"] = _owin(2 * 35 * 83, C2, dtype, kind, e)
            os.environ["MADM_DWCONV_KERNEL"] = kern
            try:
                _call("madm_dwconv3x3", _code(dtype), _p(xv), _p(wv), _p(sv), _p(tv), _p(gs["y"].view), gs["y"].ld, 2, 35, 83, C2, dil,
                      ops.ACT_RELU)
            finally:
                del os.environ["MADM_DWCONV_KERNEL"]
            _check_all(gs, f"dwconv3x3 kernel {kern} dilation {dil} {kind}")
            outs[kind] = gs["y"].view.clone()
            _no_nan(outs[kind], kind)
            assert rel_err(from_tokens(outs[kind], 2, 35, 83), ref)[0] < (1e-6 if dtype == F32 else 8e-3), (dil, kind)
        assert torch.equal(outs["tight"], outs["dense"]) and torch.equal(outs["wide"], outs["dense"]), dil


# ----------------------------------------------------------------------------- training-step kernels
@pytest.mark.parametrize("dtype", DT3, ids=ID3)
def test_train_kernels_windows(cuda, dtype):
    """madm_scale_channels (ldx, ldy), madm_relu_bwd, madm_dwconv3x3_wgrad (lddy; the lattice kernel forced as well),
    madm_resize_bilinear_bwd (lddo; din and the f32 workspace behind canaries), madm_softmax_ce (ldx; the gradient's
    columns K .. ldd belong to it and are exactly zero).  Expressions and bounds of test_dropout_relu_dwconv_grad_kernels,
    test_resize_bilinear_backward_is_the_adjoint and test_softmax_ce_loss_and_gradient (test_train_gpu.py:66-156)."""
    from madm_amd._lib import lib
    from test_train_gpu import _tol
    qd = lambda t: t.to(dtype).float()
    e = _epc(dtype)
    B, C, H, W, dil = 2, 64, 20, 24, 6
    g = torch.Generator().manual_seed(4)
    x = qd(torch.randn((B, C, H, W), generator=g))
    dy = qd(torch.randn((B, C, H, W), generator=g))
    w = torch.randn((C, 1, 3, 3), generator=g) / 3
    s = (torch.rand((B, C), generator=g) >= 0.1).float() / 0.9
    xt, dyt = to_tokens(x, dtype), to_tokens(dy, dtype)
    outs = {}
    for kind in ["dense"] + KINDS:
        gi, go = _win(xt, kind, e), _owin(B * H * W, C, dtype, "wide" if kind == "tight" else kind, e)
        gsc, sv = _vec(s)
        _call("madm_scale_channels", _code(dtype), _p(gi.view), gi.ld, _p(sv), _p(go.view), go.ld, B, H * W, C)
        _check_all({"x": gi, "scale": gsc, "y": go}, f"scale_channels {kind}")
        outs[kind] = go.view.clone()
        _no_nan(outs[kind], kind)
        assert rel_err(from_tokens(outs[kind], B, H, W), x * s[:, :, None, None])[0] < _tol(dtype, 1e-6, 8e-3, 1e-3)
    assert torch.equal(outs["tight"], outs["dense"]) and torch.equal(outs["wide"], outs["dense"])
    yr = F.relu(x)
    gs = {}
    gs["y"], yv = _vec(to_tokens(yr, dtype), post=1024)
    gs["dy"], dv = _vec(dyt, post=1024)
    gs["dx"], dxv = _flat_out((B * H * W, C), dtype)
    _call("madm_relu_bwd", _code(dtype), _p(yv), _p(dv), _p(dxv), B * H * W * C)
    _check_all(gs, "relu_bwd")
    assert torch.equal(from_tokens(dxv, B, H, W), dy * (yr > 0))
    # depthwise weight gradient: dy in a window; both kernel families (the lattice kernel on a ragged map)
    C2, H2, W2 = 128, 37, 83
    x2 = qd(torch.randn((B, C2, H2, W2), generator=g))
    dy2 = qd(torch.randn((B, C2, H2, W2), generator=g))
    w2 = torch.randn((C2, 1, 3, 3), generator=g) / 3
    for (xx, dd, ww, Cc, Hh, Ww, d_, kern) in ((x, dy, w, C, H, W, dil, None), (x2, dy2, w2, C2, H2, W2, 12, "4")):
        xr, wr = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True)
        F.conv2d(xr, wr, padding=d_, dilation=d_, groups=Cc).backward(dd)
        for kind in ["dense"] + KINDS:
            gs = {"dy": _win(to_tokens(dd, dtype), kind, e)}
            gs["x"], xv = _vec(to_tokens(xx, dtype), post=1024)
            gs["dw"], dw = _flat_out((9, Cc), F32)
            dw.zero_()
            if kern:
                os.environ["MADM_DWCONV_KERNEL"] = kern
            try:
                _call("madm_dwconv3x3_wgrad", _code(dtype), _p(xv), _p(gs["dy"].view), gs["dy"].ld, _p(dw), B, Hh, Ww, Cc, d_)
            finally:
                os.environ.pop("MADM_DWCONV_KERNEL", None)
            _check_all(gs, f"dwconv3x3_wgrad {kern} {kind}")
            _no_nan(dw, kind)
            assert rel_err(dw.t().reshape(Cc, 1, 3, 3).cpu(), wr.grad)[0] < _tol(dtype, 2e-5, 2e-5, 2e-5), (kern, kind)
    # adjoint of the bilinear resize: row-strided gradient window, dense din, guarded workspace
    for (IH, IW, OH, OW) in ((5, 7, 40, 56), (9, 30, 17, 11)):
        Cr = 16
        xr = torch.randn((B, Cr, IH, IW), generator=g, requires_grad=True)
        dyr = qd(torch.randn((B, Cr, OH, OW), generator=g))
        F.interpolate(xr, size=(OH, OW), mode="bilinear", align_corners=False).backward(dyr)
        outs = {}
        for kind in ["dense"] + KINDS:
            gs = {"dout": _win(to_tokens(dyr, dtype), kind, e)}
            gs["din"], din = _flat_out((B * IH * IW, Cr), dtype)
            nbytes = lib.madm_resize_bilinear_bwd_workspace_bytes(B, IW, OH, Cr)
            gs["workspace"], ws = _flat_out((nbytes // 4,), F32)
            _call("madm_resize_bilinear_bwd", _code(dtype), _p(gs["dout"].view), gs["dout"].ld, _p(din), B, IH, IW, OH, OW, Cr, _p(ws),
                  nbytes)
            _check_all(gs, f"resize_bilinear_bwd {kind}")
            outs[kind] = din.clone()
            _no_nan(din, kind)
            assert rel_err(from_tokens(din, B, IH, IW), xr.grad)[0] < _tol(dtype, 2e-6, 8e-3, 1e-3)
        assert torch.equal(outs["tight"], outs["dense"]) and torch.equal(outs["wide"], outs["dense"])     # gather form: no atomics
    # pixel-weighted cross entropy
    K, Hc, Wc = 11, 9, 13
    g = torch.Generator().manual_seed(6)
    logits = (3 * torch.randn((B, K, Hc, Wc), generator=g)).requires_grad_(True)
    label = torch.randint(0, K, (B, Hc, Wc), generator=g)
    label[torch.rand((B, Hc, Wc), generator=g) < 0.2] = 255
    pw = torch.rand((B, Hc, Wc), generator=g)
    M = B * Hc * Wc
    loss = (F.cross_entropy(logits, label, reduction='none', ignore_index=255) * pw).mean() * 1.7
    loss.backward()
    lt = logits.detach().permute(0, 2, 3, 1).reshape(M, K)
    ldd = 32 if dtype == F32 else 64
    for kind in ["dense"] + KINDS:
        gs = {"logits": _win(lt, kind, 1)}
        gs["labels"], lv = _vec(label)
        gs["weight"], wv = _vec(pw)
        gs["loss"], ls = _vec(torch.zeros(1, dtype=torch.float64))
        gs["gscale"], gsv = _vec(torch.tensor([2.0]))
        gs["dlogits"], dl = _flat_out((M, ldd), dtype)
        _call("madm_softmax_ce", _code(dtype), _p(gs["logits"].view), gs["logits"].ld, K, _p(lv), _p(wv), 255, M, _p(ls), _p(gsv),
              1.7 / M, _p(dl), ldd)
        _check_all(gs, f"softmax_ce {kind}")
        assert abs(ls.item() * 1.7 / M - loss.item()) < 1e-5 * abs(loss.item())
        got = dl.float().cpu()
        _no_nan(got, kind)
        assert got[:, K:].abs().max() == 0
        assert rel_err(got[:, :K], 2.0 * logits.grad.permute(0, 2, 3, 1).reshape(M, K))[0] < _tol(dtype, 1e-5, 8e-3, 1e-3)


def test_loss_gate_and_augmentation_kernels_are_contained(cuda):
    """madm_masked_l1, madm_tanh_gate_bwd, madm_bn_fold_stats, madm_mic_minmax + madm_block_mask, madm_gray_sum +
    madm_color_jitter_step, madm_blur_axis_f32, madm_groupnorm_stats / _finalize: f32 work on dense tensors whose sizes are
    no multiple of 4, every output (and accumulator) behind canaries.  Expressions and bounds of
    test_masked_l1_and_tanh_gate_backward (test_train_gpu.py:159-188), test_batchnorm_train_is_groupnorm_over_the_batch
    (:61-63), test_block_mask_kernel_is_bit_exact (test_mic_gpu.py:34-45), test_color_augmentation_kernels
    (test_train_gpu.py:469-488) and test_groupnorm_finalize_utility (test_ops_gpu.py:934-952)."""
    import numpy as np
    from madm_amd import augment, ops
    from madm_amd._lib import lib
    from oracle import augment as OA
    from test_mic_gpu import _gen as mic_gen
    g = torch.Generator().manual_seed(7)
    B, C, h, w = 2, 3, 7, 9
    pred = torch.randn((B, C, h, w), generator=g, requires_grad=True)
    gt = torch.randn((B, C, h, w), generator=g)
    mask = torch.rand((B, 1, 37, 41), generator=g)
    for l2 in (False, True):
        pred.grad = None
        d = F.mse_loss(pred, gt, reduction='none') if l2 else F.l1_loss(pred, gt, reduction='none')
        m = F.interpolate(mask, size=(h, w), mode='nearest').repeat(1, C, 1, 1)
        loss = torch.sum(d * m) / d.numel() * 0.7
        loss.backward()
        gs = {}
        gs["pred"], pv = _vec(pred.detach())
        gs["gt"], gv = _vec(gt)
        gs["mask"], mv = _vec(mask)
        gs["loss"], ls = _vec(torch.zeros(1, dtype=torch.float64))
        gs["gscale"], sc = _vec(torch.tensor([3.0]))
        gs["dpred"], dp = _flat_out((B, C, h, w), F32)
        _call("madm_masked_l1", _p(pv), _p(gv), _p(mv), B, C, h, w, 37, 41, 1 if l2 else 0, _p(ls), _p(sc), 0.7 / d.numel(), _p(dp))
        _check_all(gs, "masked_l1")
        assert abs(ls.item() * 0.7 / d.numel() - loss.item()) < 1e-6 * abs(loss.item())
        assert rel_err(dp.cpu(), 3.0 * pred.grad)[0] < 1e-6
    n, R = 77 * 768 + 1, 2
    a1, x1, a2, x2 = [torch.randn(n, generator=g).requires_grad_(True) for _ in range(4)]
    out = (torch.tanh(a1) * x1 + torch.tanh(a2) * x2)[None].repeat(R, 1)
    do = torch.randn((R, n), generator=g)
    out.backward(do)
    gs, ins, bufs = {}, [], []
    for nm, t in (("a1", a1), ("x1", x1), ("a2", a2), ("x2", x2)):
        gs[nm], v = _vec(t.detach(), post=1024)
        ins.append(v)
        gs["d" + nm], b_ = _flat_out((n,), F32)
        b_.zero_()
        bufs.append(b_)
    gs["dout"], dov = _vec(do, post=1024)
    _call("madm_tanh_gate_bwd", _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(dov), _p(bufs[0]), _p(bufs[1]), _p(bufs[2]),
          _p(bufs[3]), n, R)
    _check_all(gs, "tanh_gate_bwd")
    for b_, r_ in zip(bufs, (a1, x1, a2, x2)):
        assert rel_err(b_.cpu(), r_.grad)[0] < 1e-5
    # GroupNorm statistics of a two-source concat + the stand-alone finalize; BatchNorm bookkeeping on the same sums
    Bn, cins, H, W = 2, [1280, 640], 4, 6
    xs = [_gen((Bn, c, H, W), 30 + i) * (1.0 + i) + 0.5 * i for i, c in enumerate(cins)]
    Ct = sum(cins)
    gamma, beta = 1.0 + 0.2 * _gen((Ct,), 2), 0.3 * _gen((Ct,), 3)
    ref = F.group_norm(torch.cat(xs, 1), 32, gamma, beta, eps=1e-5)
    gs, sts = {}, []
    for i, x in enumerate(xs):
        gs[f"x{i}"], xv = _vec(to_tokens(x, F32), post=1024)
        gs[f"sums{i}"], st = _vec(torch.zeros((Bn, cins[i], 2), dtype=torch.float64))
        _call("madm_groupnorm_stats", _code(F32), _p(xv), Bn, H * W, cins[i], _p(st))
        sts.append(st)
    gs["gamma"], gv = _vec(gamma)
    gs["beta"], bv = _vec(beta)
    gs["scale"], scale = _flat_out((Bn, Ct), F32)
    gs["shift"], shift = _flat_out((Bn, Ct), F32)
    _call("madm_groupnorm_finalize", Bn, H * W, Ct, 32, _p(sts[0]), cins[0], _p(sts[1]), _p(gv), _p(bv), 1e-5, _p(scale), _p(shift))
    bn = torch.nn.BatchNorm2d(cins[1])
    with torch.no_grad():
        bn.running_mean.copy_(_gen((cins[1],), 8)); bn.running_var.copy_(0.5 + torch.rand(cins[1], generator=g))
    gs["rm"], rm = _vec(bn.running_mean.clone())
    gs["rv"], rv = _vec(bn.running_var.clone())
    gs["st"], stb = _flat_out((1, cins[1], 2), torch.float64)
    _call("madm_bn_fold_stats", _p(sts[1]), Bn, cins[1], float(Bn * H * W), 0.1, _p(stb), _p(rm), _p(rv))
    _check_all(gs, "groupnorm_stats / groupnorm_finalize / bn_fold_stats")
    got = torch.cat(xs, 1) * scale.cpu()[:, :, None, None] + shift.cpu()[:, :, None, None]
    assert rel_err(got, ref)[0] < 1e-5
    bn.train()(xs[1])
    assert rel_err(rm.cpu(), bn.running_mean)[0] < 1e-6 and rel_err(rv.cpu(), bn.running_var)[0] < 1e-6
    assert rel_err(stb.cpu()[0, :, 0], xs[1].double().sum((0, 2, 3)))[0] < 1e-6
    # block mask: 80 x 50 (the ragged case of its dense test), B = 3
    gm = mic_gen()
    Bm, Hm, Wm = 3, 80, 50
    xm = torch.rand((Bm, 3, Hm, Wm), generator=g)
    gh, gw = augment.mask_grid_shape(Hm, Wm)
    u = torch.rand((Bm, 1, gh, gw), generator=g)
    nn_ = xm.numel()
    nparts = lib.madm_mic_minmax_parts(nn_)
    gs = {}
    gs["x"], xv = _vec(xm, post=1024)
    gs["u"], uv = _vec(u)
    gs["parts"], parts = _flat_out((nparts, 2), F32)
    gs["flag"], flag = _vec(torch.zeros(1, dtype=torch.int32).view(torch.uint8))
    gs["out"], mo = _flat_out((Bm, 3, Hm, Wm), F32)
    _call("madm_mic_minmax", _p(xv), nn_, _p(parts), nparts)
    sy, sx = float(np.float32(gh) / np.float32(Hm)), float(np.float32(gw) / np.float32(Wm))
    _call("madm_block_mask", _p(xv), _p(mo), Bm, 3, Hm, Wm, _p(uv), gh, gw, sy, sx, 0.7, _p(parts), nparts, _p(flag))
    _check_all(gs, "mic_minmax / block_mask")
    assert torch.equal(mo.cpu(), gm.restated_mask_image(xm, 0.7, u=u)) and int(flag.view(torch.int32).item()) == 0
    # colour jitter steps (contrast reads the grey sum) and the two blur passes, odd sizes
    img = torch.rand((3, 47, 81), generator=g)
    img[:, 5, 5] = 0.3
    img[:, 6, 6] = torch.tensor([1.0, 0.0, 0.0])
    HW = 47 * 81
    fb, fc, fh, fs, order = augment.jitter_params(0.2, generator=g)
    factors = (fb, fc, fs, 2 * math.pi * fh)
    gs = {}
    gs["a"], cur = _vec(img, post=1024)
    for step, idx in enumerate(order):
        gsum = None
        if idx == 1:
            gs[f"gray{step}"], gsum = _vec(torch.zeros(1, dtype=torch.float64))
            _call("madm_gray_sum", _p(cur), HW, _p(gsum))
        gs[f"o{step}"], nxt = _flat_out((3, 47, 81), F32)
        _call("madm_color_jitter_step", _p(cur), _p(nxt), HW, int(idx), float(factors[idx]), _p(gsum))
        cur = nxt
    _check_all(gs, "gray_sum / color_jitter_step")
    assert (cur.cpu() - OA.color_jitter_image(img, fb, fc, fh, fs, order)).abs().max() < 2e-5
    data = torch.rand((2, 3, 63, 97), generator=g)
    ky, kx = augment.blur_kernel_size(63), augment.blur_kernel_size(97)
    gs = {}
    gs["data"], dv = _vec(data, post=1024)
    gs["wx"], wx = _vec(augment.gaussian_kernel1d(kx, 0.7, "cpu"))
    gs["wy"], wy = _vec(augment.gaussian_kernel1d(ky, 0.7, "cpu"))
    gs["tmp"], tmp = _flat_out((2, 3, 63, 97), F32)
    gs["out"], bo = _flat_out((2, 3, 63, 97), F32)
    _call("madm_blur_axis_f32", _p(dv), _p(tmp), 6, 63, 97, 1, kx, _p(wx))
    _call("madm_blur_axis_f32", _p(tmp), _p(bo), 6, 63, 97, 0, ky, _p(wy))
    _check_all(gs, "blur_axis_f32")
    assert (bo.cpu() - OA.gaussian_blur(data, ky, kx, 0.7)).abs().max() < 1e-6


# ----------------------------------------------------------------------------- labels, flat optimizer buffers, pictures
def test_label_kernels_are_contained(cuda):
    """madm_label_to_rgb, madm_pseudo_label, madm_label_presence, madm_class_mix on a 17 x 33 map (HW = 561, odd): every
    output behind canaries, bit for bit against oracle/labels.py (prob: 2e-6, test_labels_gpu.py:52,76)."""
    from oracle import labels as L
    g = torch.Generator().manual_seed(9)
    B, H, W, K = 2, 17, 33, 7
    HW = H * W
    lab = torch.randint(0, 1000, (B, 1, H, W), generator=g)
    pal = [int(v) for v in torch.randint(0, 256, (768,), generator=g)]
    gs = {}
    gs["label"], lv = _vec(lab)
    gs["palette"], pv = _vec(torch.tensor(pal, dtype=torch.uint8))
    gs["rgb"], rgb = _flat_out((B, 3, H, W), F32)
    gs["valid"], valid = _flat_out((B, 1, H, W), F32)
    _call("madm_label_to_rgb", _p(lv), _p(pv), _p(rgb), _p(valid), B, HW)
    logits = torch.randn((B, K, H, W), generator=g)
    logits[0, 1, 3, 3] = logits[0, 4, 3, 3] = 9.0
    gs["logits"], xv = _vec(logits, post=1024)
    gs["prob"], prob = _flat_out((B, H, W), F32)
    gs["plabel"], pl = _flat_out((B, H, W), torch.int64)
    gs["count"], cnt = _vec(torch.zeros(1, dtype=torch.int64))
    _call("madm_pseudo_label", _p(xv), _p(prob), _p(pl), _p(cnt), B, K, HW, 0.3)
    lab2 = torch.randint(0, K, (B, H, W), generator=g)
    gs["lab2"], l2v = _vec(lab2)
    gs["presence"], pres = _vec(torch.zeros(256, dtype=torch.int32).view(torch.uint8))
    _call("madm_label_presence", _p(l2v), B * HW, _p(pres))
    chosen = torch.tensor([1, 4, 5])
    sel = torch.zeros(256, dtype=torch.uint8)
    sel[chosen] = 1
    imgs = torch.randn((2, 3, H, W), generator=g)
    gs["sel"], sv = _vec(sel)
    gs["imgs"], iv = _vec(imgs, post=1024)
    gs["mask"], mk = _flat_out((1, H, W), F32)
    gs["mixed"], mi = _flat_out((3, H, W), F32)
    gs["mixed_label"], ml = _flat_out((H, W), torch.int64)
    _call("madm_class_mix", _p(l2v[0]), _p(l2v[1]), _p(sv), _p(iv[0]), _p(iv[1]), 3, HW, _p(mk), _p(mi), _p(ml))
    _check_all(gs, "label kernels")
    r0, v0 = L.convert_label_to_rgb(lab, pal)
    assert torch.equal(rgb.cpu(), r0) and torch.equal(valid.cpu(), v0)
    p0, l0, _ = L.pseudo_labels(logits, (H, W), 0.3)
    assert torch.equal(pl.cpu(), l0) and (prob.cpu() - p0).abs().max() < 2e-6 and pl[0, 3, 3].item() == 1
    borderline = int(((p0 - 0.3).abs() < 2e-6).sum())
    assert abs(int(cnt.item()) - int((p0 >= 0.3).sum())) <= borderline
    assert torch.equal(torch.nonzero(pres.view(torch.int32).cpu()).flatten(), torch.unique(lab2))
    mref = L.generate_class_mask(lab2[0], chosen).float()
    assert torch.equal(mk.cpu()[0], mref.reshape(H, W))
    assert torch.equal(mi.cpu(), mref.reshape(1, H, W) * imgs[0] + (1 - mref.reshape(1, H, W)) * imgs[1])
    assert torch.equal(ml.cpu(), torch.where(mref.reshape(H, W) > 0, lab2[0], lab2[1]))


def test_flat_optimizer_kernels_are_contained(cuda):
    """madm_sumsq_f32, madm_adamw_step, madm_adamw_step_table, madm_ema_update, madm_snapshot_f32 on flat f32 buffers with
    n = 4099 (n % 4 == 3; the table step needs whole 1024-element chunks), the canary starting at element n of every
    buffer.  torch.optim.AdamW, the EMA formula and the bounds of test_flat_adamw_ema_clip (2e-6, 1e-6 for the norm,
    test_eval_gpu.py:452-465) and test_table_adamw_matches_torch_adamw_with_groups (2e-6, test_train_gpu.py:553); the
    fingerprint is the integer sum include/madm_hip.h states."""
    g = torch.Generator().manual_seed(12)
    n = 4099
    lr, b1, b2, eps, wd, scale = 5e-3, 0.9, 0.999, 1e-8, 0.05, 128.0
    p0 = torch.randn(n, generator=g)
    ref_p = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    gs = {}
    gs["p"], p = _vec(p0, post=1024)
    gs["m"], m = _vec(torch.zeros(n), post=1024)
    gs["v"], v = _vec(torch.zeros(n), post=1024)
    for step in (1, 2):
        gr = torch.randn(n, generator=g)
        gs[f"g{step}"], gv = _vec(gr * scale, post=1024)
        ref_p.grad = gr.clone()
        opt.step()
        _call("madm_adamw_step", _p(p), _p(gv), _p(m), _p(v), n, lr, b1, b2, eps, wd, step, 1.0 / scale)
    gs["sumsq"], ss = _vec(torch.zeros(1, dtype=torch.float64))
    _call("madm_sumsq_f32", _p(gv), n, _p(ss))
    ema0 = torch.randn(n, generator=g)
    gs["ema"], ema = _vec(ema0, post=1024)
    _call("madm_ema_update", _p(ema), _p(p), n, 0.9)
    gs["copy"], cp = _flat_out((n,), F32)
    gs["fp"], fp = _vec(torch.zeros(1, dtype=torch.int64))
    _call("madm_snapshot_f32", _p(p), _p(cp), n, 5, _p(fp))
    _check_all(gs, "flat optimizer kernels")
    assert rel_err(p.cpu(), ref_p.detach())[0] < 2e-6
    want = ((gr * scale).double() ** 2).sum().item()
    assert abs(ss.item() - want) < 1e-6 * want
    assert rel_err(ema.cpu(), 0.9 * ema0 + (1 - 0.9) * p.cpu())[0] < 2e-6
    assert torch.equal(cp, p)
    bits = p.cpu().view(torch.int32).tolist()
    mask64, acc = (1 << 64) - 1, 0
    for i, wbits in enumerate(bits):
        hsh = ((((5 + i) << 32) | (wbits & 0xFFFFFFFF)) * 0x9E3779B97F4A7C15) & mask64
        hsh ^= hsh >> 32
        hsh = (hsh * 0xD6E8FEB86659FD93) & mask64
        hsh ^= hsh >> 32
        acc = (acc + hsh) & mask64
    assert (int(fp.item()) & mask64) == acc
    # per-tensor hyper-parameters: three chunks, two tensors, the second without a gradient this step (skipped)
    nt = 3 * 1024
    pt0 = torch.randn(nt, generator=g)
    grt = torch.randn(nt, generator=g)
    refs = [pt0[:2048].clone().requires_grad_(True), pt0[2048:].clone().requires_grad_(True)]
    ropt = torch.optim.AdamW([{"params": [refs[0]], "lr": 3e-3, "weight_decay": 0.05},
                              {"params": [refs[1]], "lr": 7e-4, "weight_decay": 0.0}], betas=(b1, b2), eps=eps)
    refs[0].grad = grt[:2048].clone()
    ropt.step()
    gs = {}
    gs["p"], pt = _vec(pt0, post=1024)
    gs["g"], gt_ = _vec(grt * scale, post=1024)
    gs["m"], mt = _vec(torch.zeros(nt), post=1024)
    gs["v"], vt = _vec(torch.zeros(nt), post=1024)
    gs["chunk_tensor"], ct = _vec(torch.tensor([0, 0, 1], dtype=torch.int32).view(torch.uint8))
    hyper = torch.tensor([[3e-3, 0.05, 1 - b1, math.sqrt(1 - b2)], [7e-4, 0.0, 0.0, 0.0]])
    gs["hyper"], hv = _vec(hyper)
    _call("madm_adamw_step_table", _p(pt), _p(gt_), _p(mt), _p(vt), nt, _p(ct), _p(hv), b1, b2, eps, 1.0 / scale)
    _check_all(gs, "adamw_step_table")
    assert (pt.cpu()[:2048] - refs[0].detach()).abs().max().item() < 2e-6
    assert torch.equal(pt.cpu()[2048:], pt0[2048:]) and float(mt[2048:].abs().max()) == 0.0


def test_picture_kernels_are_contained(cuda):
    """madm_vis_compose (every byte of the canvas, none beyond: 48 x 50 tiles, row pitch no multiple of 4, a ragged last
    sheet row) and madm_eval_export_pack (97 x 131 at an odd byte offset), byte for byte against the restatements of
    test_vis_gpu.py and eval_export_util.py."""
    import numpy as np
    from madm_amd import ops, vis, labels
    from eval_export_util import pack_ref
    from test_vis_gpu import make_tiles, on_device, palette_for, ref_sheet
    from test_eval_export_gpu import _pack_case, PALETTE19, K19
    H, W, K = 48, 50, 9
    pal = palette_for(K)
    tiles = make_tiles(2, H, W, K, seed=H * W + K)
    rows, cols, _ = vis.layout(len(tiles), 2, 5)
    g_c = guarded_flat(rows * H * cols * W * 3, torch.uint8, pre=61, post=1024)
    canvas = g_c.flat.view(rows * H, cols * W, 3)
    got = vis.compose(on_device(tiles), 5, pal, out=canvas)
    torch.cuda.synchronize()
    g_c.check("vis_compose canvas")
    assert got.data_ptr() == canvas.data_ptr()
    assert np.array_equal(canvas.cpu().numpy(), ref_sheet(tiles, 5, pal, H, W))
    image, pred, gt = _pack_case(97, 131, 7, False)
    n = ops.eval_export_pack_bytes(97, 131)
    g_o = guarded_flat(n, torch.uint8, pre=61, post=1024)
    ops.eval_export_pack(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(image).cuda(),
                         labels._device_palette(list(PALETTE19), g_o.flat.device), K19, 255, out=g_o.flat)
    torch.cuda.synchronize()
    g_o.check("eval_export_pack out")
    assert np.array_equal(g_o.flat.cpu().numpy(), pack_ref(image, pred, gt, PALETTE19, K19, 255))


# ----------------------------------------------------------------------------- which test covers which entry point
# Every madm_* function of include/madm_hip.h is in exactly one of the two tables (tests/test_windows_host.py checks it): a new
# entry point fails the suite until someone decides whether it gets a window / containment test or needs none.
COVERED = {
    "madm_conv2d_fwd": "test_conv2d_windows",
    "madm_conv2d_wgrad": "test_conv2d_wgrad_windows",
    "madm_pack_dgrad_weights": "test_conv2d_dgrad_windows",
    "madm_pack_weight": "test_weight_packing_windows",
    "madm_fold_layernorm_pack": "test_weight_packing_windows",
    "madm_attention_fwd": "test_attention_windows",
    "madm_causal_attention_fwd": "test_causal_attention_windows",
    "madm_attention_bwd": "test_attention_backward_windows",
    "madm_groupnorm_apply": "test_groupnorm_apply_windows",
    "madm_groupnorm_apply_cat": "test_groupnorm_apply_windows",
    "madm_groupnorm_bwd_sums": "test_groupnorm_backward_windows",
    "madm_groupnorm_bwd_apply": "test_groupnorm_backward_windows",
    "madm_layernorm_fwd": "test_row_kernels_windows",
    "madm_layernorm_bwd": "test_row_kernels_windows",
    "madm_softmax_rows": "test_row_kernels_windows",
    "madm_geglu_bwd": "test_row_kernels_windows",
    "madm_silu_bwd": "test_row_kernels_windows",
    "madm_add": "test_row_kernels_windows",
    "madm_colsum": "test_row_kernels_windows",
    "madm_zero_insert2x": "test_gradient_reshaping_kernels_are_contained",
    "madm_sumpool2x2": "test_gradient_reshaping_kernels_are_contained",
    "madm_stem_conv3x3": "test_stem_conv3x3_windows",
    "madm_image_to_nhwc": "test_glue_kernels_windows",
    "madm_image_to_im2col3x3": "test_glue_kernels_windows",
    "madm_nchw_f32_to_nhwc": "test_glue_kernels_windows",
    "madm_nhwc_to_nchw_f32": "test_glue_kernels_windows",
    "madm_copy_columns": "test_glue_kernels_windows",
    "madm_latents_add_noise": "test_glue_kernels_windows",
    "madm_timestep_embedding": "test_glue_kernels_windows",
    "madm_silu": "test_glue_kernels_windows",
    "madm_rows_to_f32": "test_glue_kernels_windows",
    "madm_cast_from_f32": "test_glue_kernels_windows",
    "madm_clamp_f32": "test_glue_kernels_windows",
    "madm_token_embedding": "test_clip_kernels_are_contained",
    "madm_quick_gelu": "test_clip_kernels_are_contained",
    "madm_resize_bilinear": "test_spatial_kernels_windows",
    "madm_resize_bilinear_nchw_f32": "test_spatial_kernels_windows",
    "madm_scale_pad_crop_nchw_f32": "test_spatial_kernels_windows",
    "madm_slide_merge": "test_spatial_kernels_windows",
    "madm_tanh_gate": "test_spatial_kernels_windows",
    "madm_argmax_nchw_f32": "test_spatial_kernels_windows",
    "madm_confusion_matrix": "test_spatial_kernels_windows",
    "madm_dwconv3x3": "test_dwconv3x3_windows",
    "madm_scale_channels": "test_train_kernels_windows",
    "madm_relu_bwd": "test_train_kernels_windows",
    "madm_dwconv3x3_wgrad": "test_train_kernels_windows",
    "madm_resize_bilinear_bwd": "test_train_kernels_windows",
    "madm_softmax_ce": "test_train_kernels_windows",
    "madm_masked_l1": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_tanh_gate_bwd": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_groupnorm_stats": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_groupnorm_finalize": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_bn_fold_stats": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_mic_minmax": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_block_mask": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_gray_sum": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_color_jitter_step": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_blur_axis_f32": "test_loss_gate_and_augmentation_kernels_are_contained",
    "madm_label_to_rgb": "test_label_kernels_are_contained",
    "madm_pseudo_label": "test_label_kernels_are_contained",
    "madm_label_presence": "test_label_kernels_are_contained",
    "madm_class_mix": "test_label_kernels_are_contained",
    "madm_sumsq_f32": "test_flat_optimizer_kernels_are_contained",
    "madm_adamw_step": "test_flat_optimizer_kernels_are_contained",
    "madm_adamw_step_table": "test_flat_optimizer_kernels_are_contained",
    "madm_ema_update": "test_flat_optimizer_kernels_are_contained",
    "madm_snapshot_f32": "test_flat_optimizer_kernels_are_contained",
    "madm_vis_compose": "test_picture_kernels_are_contained",
    "madm_eval_export_pack": "test_picture_kernels_are_contained",
}
EXEMPT = {
    "madm_abi_version": "host query, no device memory",
    "madm_last_error": "host query, no device memory",
    "madm_conv2d_make_plan": "host planner: touches no tensor",
    "madm_dwconv3x3_plan": "host planner: touches no tensor",
    "madm_conv2d_can_fuse_groupnorm": "host predicate: touches no tensor",
    "madm_conv2d_tile_name": "host table lookup, no device memory",
    "madm_set_tuning_profile": "host process state, no device memory",
    "madm_get_tuning_profile": "host process state, no device memory",
    "madm_debug_set_conv_tile": "host process state (the tests here use it to force tiles)",
    "madm_debug_poison_lds": "test aid: writes LDS only, its global sink is never written",
    "madm_calib_mfma_loop": "measurement loop on registers: its global sink is never written",
    "madm_attention_bwd_workspace_bytes": "host size query, no device memory",
    "madm_resize_bilinear_bwd_workspace_bytes": "host size query, no device memory",
    "madm_mic_minmax_parts": "host size query, no device memory",
}
