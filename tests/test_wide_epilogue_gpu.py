"""The LDS-DMA igemm kernels (tiles 7, 8, 11, 14 .. 17) and the 8 x 16 LDS-DMA halo conv (tiles 9, 10) under the permuted
channel mapping: a lane owns 4 * NI consecutive output channels and stores them in wide pieces (csrc/igemm.hip igemm_tile_epilogue PERM, csrc/igemm_common.hpp epilogue_tile).
Every epilogue form, on the smallest shapes at which the mapping or the choice of the store width can go wrong:

* M = one tile + 5 rows over B images (64-row tiles: 3 x 23 rows, 128-row tiles: 7 x 19), so the first tile straddles images (time
  row per row, element-wise statistics) and the second lies in one image (stashed time row, per-tile statistics);
* N cuts a lane's span in its middle (tile - 4, tile + 4, 36: N % 8 == 4, per-chunk pieces) into a window with ldo = columns + 4
  whose first element sits 4 elements into the buffer (8-byte, not 16-byte aligned, canaries before, after and in the row gaps;
  the residual likewise), and N = tile + 8 (GEGLU: 2 tile + 16) dense and aligned, where the wide pieces are taken;
* K = 64 and 320.

Reference and tolerances: the torch-CPU fp32 op on the rounded operands, as in test_ops_gpu.py (TOL for conv2d / linear, the
folded-LayerNorm and the statistics bounds of the tests of those there)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from util import to_tokens, from_tokens, rel_err
from window_util import Guarded
from test_ops_gpu import TOL as _TOL, _q, _gen

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
TOL = {torch.float32: _TOL[torch.float32], torch.bfloat16: _TOL[torch.bfloat16], torch.float16: 2.5e-3}   # test_ops_gpu.py:15, :360
LN_TOL = {torch.float32: 3e-5, torch.bfloat16: 1.5e-2, torch.float16: 2.5e-3}                              # test_ops_gpu.py:363
STAT_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 3e-3}                                # test_ops_gpu.py:207, :427

GLDS_TILES = {7: (64, 64), 8: (128, 64), 11: (64, 64), 14: (128, 128), 15: (128, 128), 16: (64, 64), 17: (128, 64)}
REG_TILES = {3: (64, 64), 2: (128, 64), 1: (128, 128)}     # register-staged kernels of the same tile shapes (plain mapping)
ROWS = {64: (3, 23), 128: (7, 19)}     # BM -> (images, rows per image): M = BM + 5
NMAX, MMAX = 288, 133


@functools.lru_cache(maxsize=None)
def _operands(dtype, K):
    """x [MMAX, K], w [NMAX, K] rounded to dtype, and x w^T (f64 accumulation), shared by every case of that dtype and K."""
    x = _q(_gen((MMAX, K), 1), dtype)
    w = _q(_gen((NMAX, K), 2) / math.sqrt(K), dtype)
    return x, w, (x.double() @ w.double().t()).float()


@functools.lru_cache(maxsize=None)
def _extras():
    return dict(bias=_gen((NMAX,), 3), rowvec=_gen((7, NMAX), 4), res=_gen((MMAX, NMAX), 5),
                gamma=1.0 + 0.3 * _gen((320,), 6), beta=0.2 * _gen((320,), 7))


def _configs(bn, feature):
    """(N, K, layout): layout 'tight' = ld = columns + 4, window 4 elements into the buffer; 'dense' = aligned, ld = columns."""
    if "geglu" in feature:
        cut, fit = [2 * bn - 8, 72], 2 * bn + 16
    else:
        cut, fit = [bn - 4, bn + 4, 36], bn + 8
    if "splitk" in feature:     # K = 64 is a single K step in the 16-bit modes: nothing to split
        return [(cut[0], 320, "tight"), (cut[-1], 320, "tight"), (fit, 320, "dense")]
    return [(n, 64, "tight") for n in cut] + [(cut[1], 320, "tight"), (fit, 64, "dense"), (fit, 320, "dense")]


def _window(rows, cols, dtype, kind):
    return Guarded(rows, cols, dtype, ld=cols + 4, c0=4) if kind == "tight" else Guarded(rows, cols, dtype)


def _launch(dtype, tile, feature, N, K, kind):
    """One launch of the linear layer [M, K] x [N, K]^T with ``feature``; returns (output f32 CPU, reference, statistics or None)."""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    bm, _ = (GLDS_TILES.get(tile) or REG_TILES[tile])
    B, HW = ROWS[bm]
    M = B * HW
    kt = ops.k_tile(dtype)
    x, w, xw = _operands(dtype, K)
    ex = _extras()
    x, w, ref = x[:M], w[:N], xw[:M, :N].clone()
    geglu = "geglu" in feature
    ocols = N // 2 if geglu else N
    kw = {}
    if feature == "ln":
        gamma, beta = ex["gamma"][:K], ex["beta"][:K]
        w32 = _gen((NMAX, K), 8)[:N] / math.sqrt(K)
        b = ex["bias"][:N]
        ref = F.linear(F.layer_norm(x, (K,), gamma, beta, 1e-5), w32, b)
        wp, bp, cs = packing.fold_layernorm(w32, b, gamma, beta, dtype, kt)
        kw.update(bias=bp.cuda(), ln=(cs.cuda(), 1e-5))
    else:
        wp = packing.pack_linear_weight(w, dtype, kt)
    if feature in ("bias", "geglu", "geglu_res", "stats"):
        ref = ref + ex["bias"][:N]
        kw["bias"] = ex["bias"][:N].contiguous().cuda()
    if feature == "rowvec":
        rv = ex["rowvec"][:B, :N].contiguous()
        ref = ref + rv.repeat_interleave(HW, 0)
        kw["rowvec"] = rv.cuda()
    if geglu:
        ref = ref[:, 0::2] * F.gelu(ref[:, 1::2])       # packed rows are (value_j, gate_j) pairs
        kw["epilogue"] = ops.EPI_GEGLU
    guards = []
    if feature in ("residual", "geglu_res"):
        res = _q(ex["res"][:M, :ocols], dtype)
        ref = ref + res
        g = _window(M, ocols, dtype, kind)
        kw["residual"] = g.load(res)
        guards.append((g, "residual"))
    if feature == "relu":
        ref = F.relu(ref)
        kw["epilogue"] = ops.EPI_RELU
    if feature == "out_f32":
        kw["out_f32"] = True
    st = None
    if feature == "stats":
        st = torch.zeros((B, N, 2), device="cuda", dtype=torch.float64)
        kw["stats"] = st
    if "splitk" in feature:
        kw["splitk"] = int(feature[-1])
    go = _window(M, ocols, torch.float32 if feature == "out_f32" else dtype, kind)
    guards.append((go, "out"))
    lib.madm_debug_set_conv_tile(tile)
    ops.PROFILE = []
    try:
        ops.conv2d(x.to(dtype).cuda(), wp.cuda(), B, HW, 1, N=N, out=go.view, **kw)
        torch.cuda.synchronize()
        kernel = ops.PROFILE[0][0]
    finally:
        ops.PROFILE = None
        lib.madm_debug_set_conv_tile(0)
    assert kernel.startswith(lib.madm_conv2d_tile_name(tile).decode()), kernel
    for g, what in guards:
        g.check(f"{feature} tile {tile} N{N} K{K} {kind}: {what}")
    return go.view.float().cpu(), ref, (None if st is None else (st.float().cpu(), B, HW))


FEATURES = ["bias", "rowvec", "residual", "relu", "geglu", "geglu_res", "out_f32", "ln", "stats", "splitk2", "splitk3"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("feature", FEATURES)
@pytest.mark.parametrize("tile", sorted(GLDS_TILES))
def test_glds_epilogue_forms(cuda, tile, feature, dtype):
    _, bn = GLDS_TILES[tile]
    tol = (LN_TOL if feature == "ln" else TOL)[dtype]
    for N, K, kind in _configs(bn, feature):
        got, ref, st = _launch(dtype, tile, feature, N, K, kind)
        assert not torch.isnan(got).any(), f"N{N} K{K} {kind}: canary left in the window"
        e, l2 = rel_err(got, ref)
        assert e < tol, f"N{N} K{K} {kind}: max rel err {e:.3e} l2 {l2:.3e}"
        if st is not None:
            sums, B, HW = st
            r = ref.reshape(B, HW, N)
            assert rel_err(sums[..., 0], r.sum(1))[0] < STAT_TOL[dtype], f"N{N} K{K} {kind}: sums"
            assert rel_err(sums[..., 1], (r ** 2).sum(1))[0] < STAT_TOL[dtype], f"N{N} K{K} {kind}: sums of squares"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("splitk", [2, 3])
@pytest.mark.parametrize("tile", sorted(GLDS_TILES))
def test_glds_splitk_slabs_feed_the_post_groupnorm(cuda, tile, splitk, dtype):
    """The slabs written under the permuted mapping are read by (m, n): the split-K reduction that carries the consumer's
    GroupNorm + SiLU (16 x 16 map, 64 channels) equals the torch composition."""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    B, Cin, H, W, Cout = 2, 64, 16, 16, 64
    kt = ops.k_tile(dtype)
    x = _q(_gen((B, Cin, H, W), 1), dtype)
    w = _q(_gen((Cout, Cin, 3, 3), 2) / math.sqrt(Cin * 9), dtype)
    bias, row = _gen((Cout,), 3), 0.5 * _gen((B, Cout), 6)
    gamma, beta = 1.0 + 0.2 * _gen((Cout,), 4), 0.3 * _gen((Cout,), 5)
    wp = packing.pack_conv_weight(w, dtype, kt).cuda()
    lib.madm_debug_set_conv_tile(tile)
    try:
        out, applied = ops.conv2d(to_tokens(x, dtype), wp, B, H, W, N=Cout, KH=3, KW=3, pad_t=1, pad_l=1, bias=bias.cuda(),
                                  rowvec=row.cuda(), splitk=splitk, post_gn=(gamma.cuda(), beta.cuda(), 32, 1e-5, True))
        torch.cuda.synchronize()
    finally:
        lib.madm_debug_set_conv_tile(0)
    assert applied
    ref = F.silu(F.group_norm(F.conv2d(x, w, bias, padding=1) + row[:, :, None, None], 32, gamma, beta, eps=1e-5))
    e, l2 = rel_err(from_tokens(out, B, H, W), ref)
    assert e < (3e-5 if dtype == torch.float32 else 2e-2), f"{e:.3e} {l2:.3e}"      # test_ops_gpu.py:566


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_glds_tiles_equal_the_register_staged_tiles_bit_for_bit(cuda, dtype):
    """The register-staged kernels keep the plain mapping and walk K in the same steps (64-element tiles, two MFMA halves each) as
    the LDS-DMA kernel of the same tile shape: per output element the same MFMAs and the same epilogue operations in the same
    order, so the two must agree in every bit -- cut N with per-chunk pieces and aligned N with wide pieces alike."""
    for glds, reg in ((7, 3), (8, 2), (14, 1)):
        _, bn = GLDS_TILES[glds]
        for feature in ("bias", "residual", "relu", "geglu", "rowvec"):
            geglu = feature == "geglu"
            for N, kind in (((2 * bn + 16) if geglu else bn + 8, "dense"), ((2 * bn - 8) if geglu else bn + 4, "tight")):
                a, _, _ = _launch(dtype, glds, feature, N, 320, kind)
                b, _, _ = _launch(dtype, reg, feature, N, 320, kind)
                assert torch.equal(a, b), f"tile {glds} vs {reg}, {feature}, N{N} {kind}: {(a != b).sum().item()} elements differ"


HALO_DMA_TILES = {9: 128, 10: 64}      # conv3x3_halo_dma_x128 / _x64: 8 x 16-pixel patches, the same channel mapping


@functools.lru_cache(maxsize=None)
def _conv_operands(dtype, B, H, W):
    Cin = 64
    x = _q(_gen((B, Cin, H, W), 11), dtype)
    w = _q(_gen((NMAX, Cin, 3, 3), 12) / math.sqrt(Cin * 9), dtype)
    return x, w, F.conv2d(x.double(), w.double(), None, padding=1).float()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("feature", ["bias_rowvec_residual", "relu", "out_f32", "stats", "splitk2", "splitk3"])
@pytest.mark.parametrize("tile", sorted(HALO_DMA_TILES))
def test_halo_dma_epilogue_forms(cuda, tile, feature, dtype):
    """The 8 x 16 LDS-DMA halo conv shares the mapping and the epilogue: a ragged one-image map (13 x 21: patches cut on both
    sides) and two full patches in two images, N cut inside a lane's span into the 8-byte-aligned window and N aligned and dense."""
    from madm_amd import ops, packing
    from madm_amd._lib import lib
    bn = HALO_DMA_TILES[tile]
    kt = ops.k_tile(dtype)
    ex = _extras()
    for (B, H, W), N, kind in [((1, 13, 21), bn - 4, "tight"), ((2, 8, 16), bn + 4, "tight"), ((2, 8, 16), 36, "tight"),
                               ((1, 13, 21), bn + 8, "dense")]:
        x, w, conv = _conv_operands(dtype, B, H, W)
        w, ref, M = w[:N], conv[:, :N].clone(), B * H * W
        kw, guards, st = {}, [], None
        if feature == "bias_rowvec_residual":
            rv = ex["rowvec"][:B, :N].contiguous()
            res = _q(_gen((B, N, H, W), 13), dtype)
            ref = ref + ex["bias"][:N][None, :, None, None] + rv[:, :, None, None] + res
            g = _window(M, N, dtype, kind)
            kw.update(bias=ex["bias"][:N].contiguous().cuda(), rowvec=rv.cuda(), residual=g.load(to_tokens(res, dtype)))
            guards.append((g, "residual"))
        if feature == "relu":
            ref = F.relu(ref)
            kw["epilogue"] = ops.EPI_RELU
        if feature == "out_f32":
            kw["out_f32"] = True
        if feature == "stats":
            st = torch.zeros((B, N, 2), device="cuda", dtype=torch.float64)
            kw["stats"] = st
        if "splitk" in feature:
            kw["splitk"] = int(feature[-1])
        go = _window(M, N, torch.float32 if feature == "out_f32" else dtype, kind)
        guards.append((go, "out"))
        wp = packing.pack_conv_weight(w, dtype, kt).cuda()
        lib.madm_debug_set_conv_tile(tile)
        ops.PROFILE = []
        try:
            ops.conv2d(to_tokens(x, dtype), wp, B, H, W, N=N, KH=3, KW=3, pad_t=1, pad_l=1, out=go.view, **kw)
            torch.cuda.synchronize()
            kernel = ops.PROFILE[0][0]
        finally:
            ops.PROFILE = None
            lib.madm_debug_set_conv_tile(0)
        what = f"{B}x{H}x{W} N{N} {kind}"
        assert kernel.startswith(lib.madm_conv2d_tile_name(tile).decode()), kernel
        for g, name in guards:
            g.check(f"{what}: {name}")
        got = from_tokens(go.view, B, H, W)
        assert not torch.isnan(got).any(), f"{what}: canary left in the window"
        e, l2 = rel_err(got, ref)
        assert e < TOL[dtype], f"{what}: max rel err {e:.3e} l2 {l2:.3e}"
        if st is not None:
            sums = st.float().cpu()
            assert rel_err(sums[..., 0], ref.sum((2, 3)))[0] < STAT_TOL[dtype], f"{what}: sums"
            assert rel_err(sums[..., 1], (ref ** 2).sum((2, 3)))[0] < STAT_TOL[dtype], f"{what}: sums of squares"
