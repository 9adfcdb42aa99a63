"""Data, references, bounds and mutants for the kernels between the UNet features and the loss (host-only torch code): the
depthwise dilated conv and its weight gradient, the bilinear resize and its adjoint, the sliding-window merge, the pixel-weighted
cross entropy and the masked L1.  Shared by tests/test_spatial_exact_host.py (the conditions, the plan, the negative controls)
and tests/test_spatial_exact_gpu.py.  The layers are those of norm_util.py.

Layer 1 -- exact.  Inputs on which the f32 arithmetic of a kernel has ONE bit pattern, whatever the order and whether or not
the compiler fuses a product into the following sum; the stored value is that result rounded once to the dtype.
  depthwise conv   x integer |x| <= 8, w integer 1 <= |w| <= 3, scale in {1/2, 1, 2}, integer shift: every f32 intermediate is
                   an integer or a half-integer below 2^24 (``dw_forward`` asserts it).  Six non-zero values cannot make the
                   nine taps of one channel pairwise distinct; instead ``dw_case`` asserts that every pair of taps differs in
                   some channel of every 32-channel block, that neighbouring channels carry different tap patterns and that
                   neighbouring slabs do.
  weight gradient  x, dy integer |.| <= 2 (det_util's term tensor); the magnitudes per (tap, channel) add up to less than
                   2^24 / 4, so f32 atomics give the integer sum in any order, also on top of an integer-filled dw.
  resize           power-of-two ratios per axis: the f32 source coordinate, both lambdas and the four weight products are
                   dyadic and exact, the data are integers, every partial sum has fewer than 2^24 quanta.
  softmax_ce       equal logits (softmax exactly 1 / K, K a power of two) and one-hot logits (0 against -200: exp underflows
                   to zero), dyadic weight / coef / gscale.
  masked_l1        dyadic pred, gt, mask and coefficients: d, |d| m, d^2 m and the f64 sum are exact.
  slide_merge      integer windows; counts 0, 1, 2, 4 divide exactly.

Layer 2 -- a tolerance per element against float64 on random inputs quantised to the dtype:  half an ulp of the output type at
the reference value, plus u = 2^-24 (half an ulp of f32, relative) times the COUNTED roundings of the kernel's expression times
the magnitude of the element's terms.  The counts (each is stated as if no product were fused; fusing only removes roundings):
  DW_ROUNDINGS = 20       nine taps of acc += x w (a product and a sum each), acc scale (1), + shift (1); then SiLU through
                          norm_util.silu_error
  wgrad                   (n - 1) u sum |dy x| for the n = B H W terms of a (tap, channel), norm_util.stat_errors' rule (the
                          products of 16-bit operands are exact in f32)
  RESIZE_ROUNDINGS = 7    1 - ly, 1 - lx, their product, the product with the pixel, three sums (the NCHW kernel's nested form
                          has six).  lambda = src - floor(src) is exact.  The source coordinate fl(fl(o + 1/2) fl(I / O)) - 1/2
                          carries the rounding of the ratio, of the product and of the difference: at most 3 u (src + 1) <
                          2^-22 (src + 1); the interpolant is piecewise linear in src, so the result moves by at most that
                          times the largest slope among the three cells around the element's, per axis.
  adjoint                 per axis (k + 3) roundings, k = the most outputs that touch one input: 1 - lambda, the sum of the
                          two weight halves, the product, and k sums; the coordinate term is the same shift of weight
                          (|dw / dsrc| = 1) between the inputs of the three cells around an output's.
  softmax_ce              expf and logf are ASSUMED accurate to 2 ulp = 4 u each (no accuracy table of the device library is
                          installed next to the compiler); the rest is counted in ``ce_bounds``.
  slide_merge, count 3    2: fl(1 / 3) and the product (the sum of three integers is exact).

Layer 3 -- mutants of the references (a tap dropped at a border, a seam read from the clamped column, a tile of the walk
skipped, align_corners coordinates, ...): the host test shows that each differs from its reference on every row it applies to,
so equality with the reference excludes it."""
import ctypes
import functools
import math
import os
from fractions import Fraction
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import det_util as D
import norm_util as N
from norm_util import F32, BF16, F16, DT3, ID3, U32, ACC_MAX, epc, half_ulp, need, quantum_exp, assert_within  # noqa: F401

DTYPE_CODE = D.DTYPE_CODE
DW_ROUNDINGS = 20
RESIZE_ROUNDINGS = 7
LIBM_ULP = 2          # assumed accuracy of expf / logf, in ulp


# ---- 0. the plan of a depthwise launch ------------------------------------------------------------------------------------------
def dw_plan(dtype, B, H, W, C, d, wgrad=False, force=None):
    """(variant, ny, nx, th, tw, blocks) of madm_dwconv3x3_plan, which both launchers call.  ``force``: the value of
    MADM_DWCONV_KERNEL for this one query (None: the process environment as it stands)."""
    from madm_amd._lib import lib
    old = os.environ.get("MADM_DWCONV_KERNEL")
    if force is not None:
        os.environ["MADM_DWCONV_KERNEL"] = str(force)
    try:
        out = (ctypes.c_int * 6)()
        rc = lib.madm_dwconv3x3_plan(DTYPE_CODE[dtype], B, H, W, C, d, out, 1 if wgrad else 0)
        assert rc == 0, lib.madm_last_error().decode()
        return tuple(out)
    finally:
        if force is not None:
            if old is None:
                del os.environ["MADM_DWCONV_KERNEL"]
            else:
                os.environ["MADM_DWCONV_KERNEL"] = old


FORCES = [1, 2, 3, 4, 0]          # MADM_DWCONV_KERNEL: plain, comb, comb with per-XCD slabs, lattice, unforced
# name, B, H, W, d, width, the lattice tile (ny, nx, th, tw) the name promises (None: the lattice kernel does not fit),
# {MADM_DWCONV_KERNEL: the variant that launch reaches}.  Widths: "c128" = 128 channels (4 slabs in f32, 2 in 16 bit), "slab" = 8
# chunks, "chunk" = one 16-byte chunk, "big" = 1024 channels in 16 bit and 512 in f32
DW_ROWS = [
    ("full_tile", 1, 30, 30, 2, "c128", (1, 1, 15, 15), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),
    ("full_tile_seams", 2, 57, 61, 2, "c128", (2, 3, 15, 11), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),   # last tiles: 14 rows, 9 columns
    ("full_tile_d6", 1, 85, 29, 6, "c128", (1, 1, 15, 5), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),       # 36 residue classes
    ("half_idle", 1, 32, 16, 2, "c128", (2, 1, 8, 8), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),
    ("half_one_col", 1, 33, 18, 2, "c128", (2, 1, 9, 9), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),        # last tile 8 rows
    # only the centre tap is inside; classes with rx >= W are empty; W < 4 d: variants 2 and 3 fall back to the plain kernel
    ("smaller_than_dilation", 2, 5, 4, 6, "c128", (1, 1, 1, 1), {0: 1, 1: 1, 2: 1, 3: 1, 4: 4}),
    ("prime_map", 1, 31, 47, 3, "c128", (1, 2, 11, 8), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),
    ("narrow_slab", 1, 19, 23, 2, "slab", (1, 1, 10, 12), {0: 2, 1: 1, 2: 2, 3: 3, 4: 4}),
    ("narrow_chunk", 1, 19, 23, 2, "chunk", None, {0: 2, 1: 1, 2: 2, 3: 2, 4: 2}),               # plain and comb only
    ("auto_lattice", 1, 128, 128, 6, "big", (2, 2, 11, 11), {0: 4, 1: 1, 2: 2, 3: 3, 4: 4}),
    ("auto_comb_xcd", 1, 128, 128, 1, "big", None, {0: 3, 1: 1, 2: 2, 3: 3, 4: 2}),
]
DW_SMALL = [r[0] for r in DW_ROWS if r[5] != "big"]
DW_REAL_ROWS = ["full_tile_seams", "prime_map"]
WINDOW_ROW = "prime_map"          # y into a column window of a wider zero buffer, every variant
# the weight gradient: the lattice-capable rows, and one whose UNFORCED launch walks 25 tiles per class on the lattice
WG_ROWS = [(r[0],) + r[1:7] + ({0: 1, 1: 1, 4: 4},) for r in DW_ROWS if r[6] is not None] + \
          [("auto_wgrad_lattice", 1, 128, 128, 2, "big", (5, 5, 13, 13), {0: 4, 1: 1, 4: 4})]
WG_FORCES = [1, 4, 0]
WG_SMALL = [r[0] for r in WG_ROWS if r[5] != "big"]
WG_STRIDED_ROW = "half_one_col"   # dy in a row-strided window


def dw_row(name, rows=None):
    return next(r for r in (rows or DW_ROWS + WG_ROWS[-1:]) if r[0] == name)


def dw_width(kind, dtype):
    return {"c128": 128, "slab": 8 * epc(dtype), "chunk": epc(dtype), "big": 512 if dtype == F32 else 1024}[kind]


def _randint(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int32)


def _taps(C, seed):
    """w [9, C] with 1 <= |w| <= 3 such that every pair of taps differs in some channel of every 32-channel block (of the whole
    width where it is narrower), neighbouring channels differ and neighbouring 32- / 64-channel slabs differ."""
    vals = torch.tensor([1, -1, 2, -2, 3, -3], dtype=torch.int32)
    blk = min(C, 32)
    for k in range(256):
        w = vals[_randint((9, C), seed + 1000 * k, 0, 5).long()]
        wb = w.view(9, C // blk, blk)
        pairs = (wb.unsqueeze(0) != wb.unsqueeze(1)).any(-1).all(-1)          # [9, 9]: tap i differs from tap j in every block
        ok = bool((pairs | torch.eye(9, dtype=torch.bool)).all())
        ok = ok and (C == 1 or bool((w[:, 1:] != w[:, :-1]).any(0).all()))
        for chs in (32, 64):
            if C >= 2 * chs:
                s = w.view(9, C // chs, chs)
                ok = ok and bool((s[:, 1:] != s[:, :-1]).any(2).any(0).all())
        if ok:
            return w
    raise AssertionError("no tap table with the stated properties")


@functools.lru_cache(maxsize=None)
def dw_case(name, C):
    """Layer-1 data of a depthwise row at width C, as int32: x [B, H, W, C], w [9, C], scale2 = 2 scale, shift [C]"""
    _n, B, H, W, d, _k, tile, variants = dw_row(name)
    seed = 4100 + 17 * [r[0] for r in DW_ROWS + WG_ROWS[-1:]].index(name) + C
    c = torch.arange(C)
    ns = SimpleNamespace(name=name, B=B, H=H, W=W, d=d, C=C, tile=tile, variants=variants)
    ns.x = _randint((B, H, W, C), seed, -8, 8)
    ns.w = _taps(C, seed + 1)
    ns.scale2 = torch.tensor([1, 2, 4], dtype=torch.int32)[((c + c // 32) % 3).long()]        # scale 1/2, 1, 2
    ns.shift = ((5 * c + c // 32) % 9 - 3).to(torch.int32)
    assert bool((ns.scale2[1:] != ns.scale2[:-1]).any()) and int(ns.w.abs().min()) >= 1 and int(ns.w.abs().max()) <= 3
    return ns


DW_MUTANTS = ["border_tap_dropped", "taps_transposed", "dilation_x_plus_one", "seam_clamped", "slab_offset_zero", "image_zero",
              "row14_dropped", "half_row_dropped"]


def dw_mutant_applies(mut, ns, chs):
    """Where a mutant changes the statement at all (a geometry condition, not an outcome)"""
    ny, nx, th, tw = ns.tile or (0, 0, 0, 0)
    return {"border_tap_dropped": ns.W > ns.d, "taps_transposed": ns.W > ns.d or ns.H > ns.d,
            "dilation_x_plus_one": ns.W > ns.d, "seam_clamped": nx > 1, "slab_offset_zero": ns.C > chs, "image_zero": ns.B > 1,
            "row14_dropped": th == 15, "half_row_dropped": tw > 8}[mut]


def dw_accumulate(x, w, d, mut=None, tile=None, chs=32):
    """acc[b][y][x][c] = sum over the taps inside the image of w[r * 3 + s][c] x[b][y + (r - 1) d][x + (s - 1) d][c], in the
    type of x (int32 or float64).  Mutants of the statement: see DW_MUTANTS."""
    B, H, W, C = x.shape
    oy, ox = torch.arange(H), torch.arange(W)
    dx_ = d + 1 if mut == "dilation_x_plus_one" else d
    if mut == "slab_offset_zero":
        x = x[..., torch.arange(C) % chs]
    if mut == "image_zero":
        x = x[torch.zeros(B, dtype=torch.long)]
    if mut == "taps_transposed":
        w = w.view(3, 3, C).transpose(0, 1).reshape(9, C)
    acc = torch.zeros_like(x)
    for r in range(3):
        iy = oy + (r - 1) * d
        vy = (iy >= 0) & (iy < H)
        rows = x.index_select(1, iy.clamp(0, H - 1))
        for s in range(3):
            ix = ox + (s - 1) * dx_
            vx = (ix >= 0) & (ix < W)
            if mut == "border_tap_dropped" and s == 2:
                vx = vx & (ix != W - 1)                          # the right tap never reaches the last column
            if mut == "seam_clamped" and s == 2:
                _ny, nx, _th, tw = tile
                sx = ox // d
                seam = (sx % tw == tw - 1) & (sx // tw < nx - 1) & vx
                ix = torch.where(seam, ox, ix)                   # the column right of the tile: the clamped one, not the neighbour's
            g = rows.index_select(2, ix.clamp(0, W - 1))
            m = (vy.view(H, 1) & vx.view(1, W)).view(1, H, W, 1).to(x.dtype)
            acc += g * m * w[r * 3 + s]
    return acc


def dw_forward(ns, act, mut=None, chs=32):
    """The exact output [B, H, W, C] as float32 (every value a half-integer below 2^24): act(acc scale + shift)"""
    acc = dw_accumulate(ns.x, ns.w, ns.d, mut, ns.tile, chs)
    assert 9 * 8 * 3 * 4 + 2 * 5 < ACC_MAX                       # |acc| <= 216, |acc scale + shift| <= 437, in halves
    v2 = acc * ns.scale2 + 2 * ns.shift                          # 2 (acc scale + shift): an integer
    assert int(v2.abs().max()) < 1 << 24
    if act == "relu":
        v2 = v2.clamp_min(0)
    if mut in ("row14_dropped", "half_row_dropped"):             # outputs the thread never writes keep the buffer's zero
        _ny, _nx, th, tw = ns.tile
        sy, sx = torch.arange(ns.H) // ns.d, torch.arange(ns.W) // ns.d
        dead = (sy % th == 14).view(ns.H, 1) | torch.zeros(1, ns.W, dtype=torch.bool) if mut == "row14_dropped" else \
            torch.zeros(ns.H, 1, dtype=torch.bool) | (sx % tw >= 8).view(1, ns.W)
        v2 = v2 * (~dead).view(1, ns.H, ns.W, 1).to(v2.dtype)
    if act == "relu" and mut is None:
        frac = float((v2 != 0).double().mean())
        assert frac > 0.25, f"{ns.name}: only {frac:.2f} of the outputs survive the ReLU"
    return v2.float() / 2


@functools.lru_cache(maxsize=None)
def dw_expected(name, C, act):
    """``dw_forward`` of the unmutated row as tokens [B * H * W, C], computed once (the big rows are shared by bf16 and f16)"""
    return dw_forward(dw_case(name, C), act).view(-1, C)


@functools.lru_cache(maxsize=None)
def dw_real_case(name, dtype):
    """Layer 2: x quantised to the dtype, f32 w / scale / shift (all held as float64), SiLU: reference z, y and the tolerance"""
    _n, B, H, W, d, kind, _t, _v = dw_row(name)
    C = dw_width(kind, dtype)
    seed = 4500 + DW_REAL_ROWS.index(name)
    x = N.quantised((B, H, W, C), seed, dtype)
    w = N.quantised((9, C), seed + 10, F32, 1 / 3)
    scale = N.quantised((C,), seed + 20, F32, 0.1, 1.0)
    shift = N.quantised((C,), seed + 30, F32, 0.1)
    acc = dw_accumulate(x, w, d)
    mag = dw_accumulate(x.abs(), w.abs(), d)
    z = acc * scale + shift
    dz = U32 * DW_ROUNDINGS * (mag * scale.abs() + shift.abs())
    y = F.silu(z)
    return SimpleNamespace(B=B, H=H, W=W, d=d, C=C, x=x, w=w, scale=scale, shift=shift, z=z, y=y,
                           tol=half_ulp(y, dtype) + N.silu_error(z, dz))


# ---- 2. the depthwise weight gradient ----------------------------------------------------------------------------------------------
def _tap_grids(H, W, d):
    oy, ox = torch.arange(H).view(H, 1).expand(H, W), torch.arange(W).view(1, W).expand(H, W)
    return [(oy + (r - 1) * d, ox + (s - 1) * d) for r in range(3) for s in range(3)]


def wgrad_sum(x, dy, d, weight=None, stale_halo=None):
    """dw [9, C] (int64 or float64) = sum over pixels of weight[y][x] dy[p] x[p + offset_t]; x, dy [B, H, W, C].
    ``stale_halo`` (ny, nx, th, tw): every tile but the first of a class's walk multiplies with the PREVIOUS tile's halo."""
    B, H, W, C = x.shape
    out = []
    sy, sx = torch.arange(H).view(H, 1) // d, torch.arange(W).view(1, W) // d
    for iy, ix in _tap_grids(H, W, d):
        if stale_halo is not None:
            _ny, nx, th, tw = stale_halo
            ty, tx = (sy // th).expand(H, W), (sx // tw).expand(H, W)
            iy = torch.where(tx > 0, iy, torch.where(ty > 0, iy - th * d, iy))
            ix = torch.where(tx > 0, ix - tw * d, torch.where(ty > 0, ix + (nx - 1) * tw * d, ix))
        valid = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        g = x[:, iy.clamp(0, H - 1), ix.clamp(0, W - 1)] * valid.view(1, H, W, 1).to(x.dtype)
        t = dy * g
        if weight is not None:
            t = t * weight.view(1, H, W, 1).to(x.dtype)
        out.append(t.sum((0, 1, 2), dtype=torch.float64 if x.dtype == torch.float64 else torch.int64))
    return torch.stack(out)


def wgrad_sum_sliced(x, dy, d):
    """The same sum with slices instead of gathers (the 16 M-element rows): int64 [9, C]"""
    B, H, W, C = x.shape
    out = []
    for r in range(3):
        for s in range(3):
            oy0, oy1 = max(0, -(r - 1) * d), min(H, H - (r - 1) * d)
            ox0, ox1 = max(0, -(s - 1) * d), min(W, W - (s - 1) * d)
            if oy1 <= oy0 or ox1 <= ox0:
                out.append(torch.zeros(C, dtype=torch.int64))
                continue
            a = dy[:, oy0:oy1, ox0:ox1]
            b = x[:, oy0 + (r - 1) * d:oy1 + (r - 1) * d, ox0 + (s - 1) * d:ox1 + (s - 1) * d]
            out.append((a * b).sum((0, 1, 2), dtype=torch.int64))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def wgrad_case(name, C):
    """Layer 1: x, dy integers of magnitude <= 2 (tokens, float64), the exact integer sum ``dw`` [9, C] (float64) and an
    integer-valued old content ``old`` of the accumulated-into buffer.  Small rows: det_util's case with its term tensor (``det``);
    the 16 M-element rows: int32 data of their own, summed with slices."""
    _n, B, H, W, d, kind, tile, variants = dw_row(name, WG_ROWS)
    seed = 5100 + [r[0] for r in WG_ROWS].index(name)
    ns = SimpleNamespace(name=name, B=B, H=H, W=W, d=d, C=C, tile=tile, variants=variants, det=None)
    if kind == "big":
        assert B * H * W * 4 < ACC_MAX / 4                       # every term is at most 4 in magnitude
        ns.x4, ns.dy4 = _randint((B, H, W, C), seed, -2, 2), _randint((B, H, W, C), seed + 50, -2, 2)
        ns.dw = wgrad_sum_sliced(ns.x4, ns.dy4, d).double()
    else:
        ns.det = D.check_exact(D.dw_geometry_case(B, H, W, d, C, seed))
        ns.x4, ns.dy4 = ns.det.x.view(B, H, W, C), ns.det.dy.view(B, H, W, C)
        ns.dw = D.reduce(ns.det)[:, 0, :]
    ns.old = N.ints((9, C), seed + 90, 1 << 20)
    assert float(ns.old.abs().max()) + float(ns.dw.abs().max()) < ACC_MAX
    return ns


WG_MUTANTS = ["tile_skipped", "sums_reset", "stale_halo", "taps_swapped"]


def wgrad_mutant_applies(mut, ns):
    """A geometry condition: swapped taps need an off-centre tap inside the image, the walk's mutants more than one tile"""
    ny, nx, _th, _tw = ns.tile
    if mut == "taps_swapped":
        return ns.W > ns.d and ns.H > ns.d
    return ny * nx > 1 if mut in ("sums_reset", "stale_halo") else True


def wgrad_mutant(ns, mut):
    """dw [9, C] float64 of a mutated walk over the lattice tiles of every residue class (small rows only)"""
    ny, nx, th, tw = ns.tile
    H, W, d = ns.H, ns.W, ns.d
    sy, sx = torch.arange(H).view(H, 1) // d, torch.arange(W).view(1, W) // d
    tile_of = ((sy // th) * nx + sx // tw).expand(H, W)
    x, dy = ns.x4.double(), ns.dy4.double()
    if mut == "tile_skipped":                                    # the last tile of the walk, in every class
        return wgrad_sum(x, dy, d, weight=(tile_of != ny * nx - 1))
    if mut == "sums_reset":                                      # only the last tile's products survive
        return wgrad_sum(x, dy, d, weight=(tile_of == ny * nx - 1))
    if mut == "stale_halo":
        return wgrad_sum(x, dy, d, stale_halo=ns.tile)
    if mut == "taps_swapped":
        return ns.dw.view(3, 3, -1).transpose(0, 1).reshape(9, -1)
    raise KeyError(mut)


@functools.lru_cache(maxsize=None)
def wgrad_real_case(name, dtype):
    """Layer 2: random quantised x, dy; reference and (n - 1) u sum |dy x| per (tap, channel), + half an ulp of the f32 output"""
    _n, B, H, W, d, kind, _t, _v = dw_row(name)
    C = dw_width(kind, dtype)
    seed = 5500 + DW_REAL_ROWS.index(name)
    x, dy = N.quantised((B, H, W, C), seed, dtype), N.quantised((B, H, W, C), seed + 1, dtype)
    ref = wgrad_sum(x, dy, d)
    mag = wgrad_sum(x.abs(), dy.abs(), d)
    return SimpleNamespace(B=B, H=H, W=W, d=d, C=C, x=x, dy=dy, ref=ref, tol=half_ulp(ref, F32) + (B * H * W - 1) * U32 * mag)


# ---- 3. bilinear resize and its adjoint --------------------------------------------------------------------------------------------
RS_EXACT = [((5, 7), (20, 28)), ((3, 3), (24, 24)), ((8, 6), (4, 3)), ((7, 5), (7, 5)), ((1, 1), (8, 8)), ((16, 16), (1, 1)),
            ((4, 8), (16, 4)), ((16, 16), (64, 64)), ((2, 3), (16, 24))]
RS_REAL = [((5, 7), (3, 4)), ((5, 7), (16, 9)), ((9, 30), (17, 11)), ((30, 50), (61, 67))]
RS_NCHW_REAL = ((30, 50), (61, 67))
RS_WINDOW_ROW = ((4, 8), (16, 4))         # ldi / ldo / lddo windows
RS_B = 2
RS_MUTANTS = ["align_corners", "no_clamp0", "upper_not_clamped", "lambda_swapped", "scales_swapped"]
RS_ADJ_MUTANTS = ["window_lo_short", "window_hi_short"]


def rs_id(row):
    (ih, iw), (oh, ow) = row
    return f"{ih}x{iw}_to_{oh}x{ow}"


def rs_widths(dtype):
    """12 in f32 (the logits' own width: three chunks per pixel); 24 and 64 in 16 bit"""
    return [12] if dtype == F32 else [24, 64]


def _coords(I, O, mut=None, ratio=None):
    """Per output o: (i0, i1, lambda as a Fraction, the clamped source coordinate) of F.interpolate(bilinear,
    align_corners=False), from the definition with the ratio I / O as an exact fraction"""
    ratio = Fraction(I, O) if ratio is None else ratio
    out = []
    for o in range(O):
        src = (Fraction(o) + Fraction(1, 2)) * ratio - Fraction(1, 2)
        if mut == "align_corners":
            src = Fraction(o * (I - 1), O - 1) if O > 1 else Fraction(0)
        if src < 0 and mut != "no_clamp0":
            src = Fraction(0)
        i0 = min(int(src), I - 1)                      # int() truncates towards zero, as the kernel's cast does
        i1 = min(i0 + 1, I - 1)
        out.append((i0, i1, src - i0, src))
    return out


def resize_matrix(I, O, mut=None, ratio=None):
    """M [O, I] float64 with out = M in along one axis"""
    M = torch.zeros((O, I), dtype=torch.float64)
    for o, (i0, i1, lam, _s) in enumerate(_coords(I, O, mut, ratio)):
        a, b = (lam, 1 - lam) if mut == "lambda_swapped" else (1 - lam, lam)
        M[o, i0] += float(a)
        if mut == "upper_not_clamped" and i0 + 1 > I - 1:
            continue                                   # the row behind the last one: not the last one again
        M[o, i1] += float(b)
    return M


def rs_axis_mutant_applies(mut, I, O):
    if mut == "align_corners":
        return I > 1 and O != I
    if mut in ("no_clamp0", "upper_not_clamped"):
        return O > I > 1
    if mut == "lambda_swapped":                        # lambda = 1/2 everywhere at an even integer ratio
        return I > 1 and not (I % O == 0 and (I // O) % 2 == 0)
    raise KeyError(mut)


def rs_mutant_applies(mut, row):
    (ih, iw), (oh, ow) = row
    if mut == "scales_swapped":
        return Fraction(ih, oh) != Fraction(iw, ow) and (ih > 1 or iw > 1)
    if mut in RS_ADJ_MUTANTS:
        return True
    return rs_axis_mutant_applies(mut, ih, oh) or rs_axis_mutant_applies(mut, iw, ow)


def rs_matrices(row, mut=None):
    (ih, iw), (oh, ow) = row
    if mut == "scales_swapped":
        return resize_matrix(ih, oh, ratio=Fraction(iw, ow)), resize_matrix(iw, ow, ratio=Fraction(ih, oh))
    if mut in RS_ADJ_MUTANTS:                          # the gather window [lo, hi] of every input one output short
        My, Mx = resize_matrix(ih, oh), resize_matrix(iw, ow)
        for M in (My, Mx):
            for i in range(M.shape[1]):
                nz = M[:, i].nonzero().view(-1)
                if len(nz):
                    M[nz[0] if mut == "window_lo_short" else nz[-1], i] = 0.0
        return My, Mx
    return resize_matrix(ih, oh, mut), resize_matrix(iw, ow, mut)


def rs_apply(My, Mx, x):
    """x [B, IH, IW, C] -> [B, OH, OW, C]"""
    return torch.einsum("oy,byxc,px->bopc", My, x, Mx).contiguous()


def rs_adjoint(My, Mx, dy):
    """dy [B, OH, OW, C] -> [B, IH, IW, C]"""
    return torch.einsum("oy,bopc,px->byxc", My, dy, Mx).contiguous()


@functools.lru_cache(maxsize=None)
def rs_exact_case(row, C):
    """Layer 1: integer x (|x| <= 64) and dy (|dy| <= 8), dyadic weight matrices, every partial sum below 2^24 quanta"""
    (ih, iw), (oh, ow) = row
    seed = 6100 + 31 * RS_EXACT.index(row) + C
    My, Mx = rs_matrices(row)
    jy, jx = quantum_exp(My), quantum_exp(Mx)
    x, dy = N.ints((RS_B, ih, iw, C), seed, 64), N.ints((RS_B, oh, ow, C), seed + 1, 8)
    y, dx = rs_apply(My, Mx, x).contiguous(), rs_adjoint(My, Mx, dy).contiguous()
    assert float(rs_apply(My.abs(), Mx.abs(), x.abs()).max()) * 2.0 ** (jy + jx) < ACC_MAX
    assert float(rs_adjoint(My.abs(), Mx.abs(), dy.abs()).max()) * 2.0 ** (jy + jx) < ACC_MAX
    need(y, F32, "resize output")
    need(dx, F32, "resize adjoint")
    return SimpleNamespace(row=row, C=C, My=My, Mx=Mx, x=x, dy=dy, y=y, dx=dx)


def _axis_terms(I, O):
    """(i0 [O] long, delta [O] = 2^-22 (src + 1), A [O, I] = 1 where input i belongs to the three cells around output o's, k =
    the most outputs that touch one input)"""
    co = _coords(I, O)
    i0 = torch.tensor([c[0] for c in co])
    delta = torch.tensor([2.0 ** -22 * (float(c[3]) + 1) for c in co], dtype=torch.float64)
    i = torch.arange(I).view(1, I)
    A = ((i >= i0.view(O, 1) - 1) & (i <= i0.view(O, 1) + 2)).double()
    k = int((resize_matrix(I, O) != 0).sum(0).max())
    return i0, delta, A, k


def _slope_max(x, axis):
    """[B, IH, IW, C]: the largest |difference of neighbours along ``axis``| among the 3 x 3 cells around (y, x)"""
    B, IH, IW, C = x.shape
    s = torch.zeros_like(x)
    if axis == 1 and IH > 1:
        s[:, :-1] = (x[:, 1:] - x[:, :-1]).abs()
    if axis == 2 and IW > 1:
        s[:, :, :-1] = (x[:, :, 1:] - x[:, :, :-1]).abs()
    return F.max_pool2d(s.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)


def resize_bound(row, x, dtype):
    """(reference, tolerance) [B, OH, OW, C] of the resize of x [B, IH, IW, C] (float64), see the module docstring"""
    (ih, iw), (oh, ow) = row
    My, Mx = rs_matrices(row)
    ref = rs_apply(My, Mx, x)
    mag = rs_apply(My.abs(), Mx.abs(), x.abs())
    y0, dy_, _A, _k = _axis_terms(ih, oh)
    x0, dx_, _A, _k = _axis_terms(iw, ow)
    coord = dy_.view(1, oh, 1, 1) * _slope_max(x, 1)[:, y0][:, :, x0] + dx_.view(1, 1, ow, 1) * _slope_max(x, 2)[:, y0][:, :, x0]
    return ref, half_ulp(ref, dtype) + U32 * RESIZE_ROUNDINGS * mag + coord


def resize_bwd_bound(row, dy, dtype):
    """(reference, tolerance) [B, IH, IW, C] of the adjoint on dy [B, OH, OW, C] (float64)"""
    (ih, iw), (oh, ow) = row
    My, Mx = rs_matrices(row)
    ref = rs_adjoint(My, Mx, dy)
    mag = rs_adjoint(My.abs(), Mx.abs(), dy.abs())
    _y0, dly, Ay, ky = _axis_terms(ih, oh)
    _x0, dlx, Ax, kx = _axis_terms(iw, ow)
    coord = rs_adjoint(Ay * dly.view(-1, 1), Mx.abs(), dy.abs()) + rs_adjoint(My.abs(), Ax * dlx.view(-1, 1), dy.abs())
    return ref, half_ulp(ref, dtype) + U32 * (ky + 3 + kx + 3) * mag + coord


def rs_real_input(row, C, dtype, adjoint=False):
    (ih, iw), (oh, ow) = row
    shape = (RS_B, oh, ow, C) if adjoint else (RS_B, ih, iw, C)
    return N.quantised(shape, 6500 + 3 * RS_REAL.index(row) + (1 if adjoint else 0), dtype)


# ---- 4. softmax_ce -----------------------------------------------------------------------------------------------------------------
IGNORE = 255
CE_MUTANTS = ["weight_of_previous_pixel", "ignore_not_honoured", "mean_over_valid", "max_not_subtracted", "gscale_twice"]


def ce_reference(x, K, labels, weight, coef, g, mut=None):
    """(loss_sum, dlogits [M, K]) in float64 of the header's statement on logits x [M, >= K] (float64): labels equal to IGNORE or
    outside [0, K) contribute nothing."""
    M = x.shape[0]
    x = x[:, :K]
    valid = (labels != IGNORE) & (labels >= 0) & (labels < K)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    if mut == "ignore_not_honoured":                   # an ignored pixel counts as class 0
        valid = (labels == IGNORE) | valid
    w = torch.ones(M, dtype=torch.float64) if weight is None else weight.double()
    if mut == "weight_of_previous_pixel":
        w = w.roll(1)
    w = w * valid
    if mut == "mean_over_valid":
        coef = coef * M / max(int(valid.sum()), 1)
    if mut == "gscale_twice":
        g = g * g
    if mut == "max_not_subtracted":                    # f32, as a kernel would: exp overflows on the offset rows
        e = torch.exp(x.float())
        p, lsm = (e / e.sum(1, keepdim=True)).double(), (x.float() - torch.log(e.sum(1, keepdim=True))).double()
    else:
        lsm = torch.log_softmax(x, 1)
        p = lsm.exp()
    onehot = F.one_hot(lab, K).double()
    loss = -(w * lsm.gather(1, lab.view(-1, 1)).view(-1))
    loss = torch.where(w != 0, loss, torch.zeros_like(loss))
    grad = coef * g * w.view(-1, 1) * (p - onehot)
    return float(loss.sum()), grad


def ce_labels(M, K, seed):
    """Random labels in [0, K) with every eighth pixel IGNORE and a few outside [0, K) that are not the ignore index"""
    g = torch.Generator().manual_seed(int(seed))
    lab = torch.randint(0, K, (M,), generator=g)
    i = torch.arange(M)
    lab[i % 8 == 3] = IGNORE
    lab[i % 16 == 5] = -1
    lab[i % 16 == 9] = K
    lab[i % 16 == 13] = 254
    return lab


def ce_dyadic_weight(M, seed):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randint(0, 9, (M,), generator=g).double() / 4).float()          # 0, 1/4, .. 2


CE_EXACT_K = [1, 2, 8]
CE_EXACT_M = 300                  # two blocks of 256 pixels
CE_COEF, CE_G = 2.0 ** -3, 2.0 ** 4


@functools.lru_cache(maxsize=None)
def ce_exact_case(kind, K):
    """(a) "equal": the K logits of a pixel are equal (another value per pixel); (b) "onehot": 0 at the label, -200 elsewhere
    (at the pixels whose label is no class: 0 at class 0)"""
    M, ldx = CE_EXACT_M, K + 3
    lab = ce_labels(M, K, 7000 + K)
    w = ce_dyadic_weight(M, 7100 + K)
    g = torch.Generator().manual_seed(7200 + K)
    x = torch.randn((M, ldx), generator=g).float() * 50          # the columns behind K: never read into a result
    valid = (lab >= 0) & (lab < K)
    if kind == "equal":
        x[:, :K] = (torch.randn((M, 1), generator=g) * 30).float()
        grad = CE_COEF * CE_G * (w.double() * valid).view(-1, 1) * (1.0 / K - F.one_hot(lab.clamp(0, K - 1), K).double())
        loss = float((w.double() * valid).sum()) * math.log(K)
    else:
        hot = torch.where(valid, lab, torch.zeros_like(lab))
        x[:, :K] = -200.0
        x[torch.arange(M), hot] = 0.0
        grad = torch.zeros((M, K), dtype=torch.float64)
        loss = 0.0
    assert K & (K - 1) == 0 and float(torch.tensor(-200.0).exp()) == 0.0
    need(grad, BF16, "gradient")                                  # (so no rounding hides a wrong one)
    return SimpleNamespace(M=M, K=K, ldx=ldx, x=x, labels=lab, weight=w, grad=grad, loss=loss, n_weight=float((w.double() * valid).sum()))


# name, K, ldx, M, weight ("none" / "given" / "zero"), per-pixel logit offsets, gscale given
CE_REAL_ROWS = [("k11_one_pixel", 11, 12, 1, "given", False, True),
                ("k11_m257", 11, 12, 257, "none", False, False),
                ("k19_m257_weighted", 19, 20, 257, "given", False, True),
                ("k12_dense_rows", 12, 12, 257, "given", True, True),
                ("k19_offsets", 19, 20, 257, "given", True, False),
                ("k11_zero_weight", 11, 12, 257, "zero", True, True)]
CE_BIG_ROW = ("k11_second_trip", 11, 12, 4096 * 256 + 3, "given", False, True)       # f32 gradient only
CE_SUBNORMAL = 2.0 ** -16         # coef gscale of the f16 rows: with weights up to 2 no gradient exceeds 2^-15 (f16 is subnormal below 2^-14)
CE_PREFILL = 1234.5


@functools.lru_cache(maxsize=None)
def ce_real_case(name):
    _n, K, ldx, M, wkind, offsets, with_g = next(r for r in CE_REAL_ROWS + [CE_BIG_ROW] if r[0] == name)
    seed = 7500 + 13 * ([r[0] for r in CE_REAL_ROWS] + [CE_BIG_ROW[0]]).index(name)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, ldx), generator=g).float() * 3
    if offsets:
        x = (x.double() + (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1) * 1e4).float()
    w = {"none": None, "zero": torch.zeros(M), "given": torch.rand(M, generator=g) * 2}[wkind]
    return SimpleNamespace(name=name, K=K, ldx=ldx, M=M, x=x, labels=ce_labels(M, K, seed + 1), weight=w,
                           coef=0.7 / M, g=512.0 if with_g else None)


def ce_bounds(ns, coef, g, dtype):
    """(loss, loss tolerance, grad [M, K], grad tolerance).  With t_k = x_k - mx (one rounding, |t_k| u relative in the
    exponential) and expf to LIBM_ULP ulp, e_k is off by (|t_k| + 2 LIBM_ULP) u relative; the sum of K of them adds K - 1
    roundings to the weighted mean of those; g w / se: the product coef gscale, the product with w, the quotient (3), then the
    product with e_k (1) and the difference with the label's g w (1, of the result).  The loss: logf (2 LIBM_ULP u of |log se|
    plus the sum's relative error), the sum with mx and the difference with x_label (u of the intermediate each), the product
    with w; the f64 sum over pixels adds nothing on this scale."""
    K = ns.K
    x = ns.x.double()[:, :K]
    gg = 1.0 if g is None else g
    loss, grad = ce_reference(ns.x.double(), K, ns.labels, ns.weight, coef, gg)
    valid = (ns.labels >= 0) & (ns.labels < K) & (ns.labels != IGNORE)
    w = (torch.ones(ns.M, dtype=torch.float64) if ns.weight is None else ns.weight.double()) * valid
    mx = x.max(1, keepdim=True).values
    t = (x - mx).abs()
    p = torch.softmax(x, 1)
    rel_e = t + 2 * LIBM_ULP
    rel_se = (p * rel_e).sum(1, keepdim=True) + (K - 1)
    lab = torch.where(valid, ns.labels, torch.zeros_like(ns.labels))
    onehot = F.one_hot(lab, K).double()
    cgw = (abs(coef * gg) * w).view(-1, 1)
    tol_g = half_ulp(grad, dtype) + U32 * cgw * (p * (rel_e + rel_se + 4) + 2 * onehot + (p - onehot).abs())
    lse = torch.log(torch.exp(x - mx).sum(1))
    li = lse + mx.view(-1) - x.gather(1, lab.view(-1, 1)).view(-1)
    tol_l = U32 * w * (2 * LIBM_ULP * lse.abs() + rel_se.view(-1) + (lse + mx.view(-1)).abs() + 2 * li.abs())
    return loss, float(tol_l.sum()) + 1e-13 * abs(loss), grad, tol_g


# ---- 5. masked_l1 and slide_merge --------------------------------------------------------------------------------------------------
# mask (Hm, Wm) -> (h, w); None = no mask; the last row makes a second trip of the grid-stride loop (1024 blocks of 256)
ML_ROWS = [((64, 64), (8, 8), 2, 4), ((10, 7), (3, 5), 2, 4), ((7, 10), (16, 24), 2, 4), ((1, 1), (4, 4), 2, 4), (None, (5, 9), 2, 4),
           ((24, 24), (192, 192), 2, 4)]
ML_COEF, ML_G = 2.0 ** -5, 2.0 ** 3


def ml_id(row):
    return ("nomask" if row[0] is None else f"{row[0][0]}x{row[0][1]}") + f"_to_{row[1][0]}x{row[1][1]}"


@functools.lru_cache(maxsize=None)
def ml_case(row):
    """Dyadic pred, gt (multiples of 1/8, |.| <= 4, a fifth of the differences zero) and mask (multiples of 1/4 in [0, 1]); the
    nearest-neighbour index map is F.interpolate(mode='nearest') in float32 applied to the mask itself."""
    mshape, (h, w), B, C = row
    seed = 8000 + ML_ROWS.index(row)
    pred, gt = N.ints((B, C, h, w), seed, 32, 8), N.ints((B, C, h, w), seed + 1, 32, 8)
    same = N.ints((B, C, h, w), seed + 2, 2) == 0
    gt = torch.where(same, pred, gt)
    mask = N.ints((B, 1) + mshape, seed + 3, 2).abs() / 2 if mshape is not None else None      # 0, 1/2, 1
    if mask is not None:
        mask = (mask + N.ints((B, 1) + mshape, seed + 4, 1).abs() / 4).clamp(0, 1)             # + 0 or 1/4
    m = F.interpolate(mask.float(), size=(h, w), mode="nearest").double() if mask is not None else torch.ones((B, 1, h, w)).double()
    d = pred - gt
    out = {}
    for l2 in (False, True):
        terms = (d * d if l2 else d.abs()) * m
        need(terms, F32, "|d| m")
        assert float(terms.sum()) * 256 < 2.0 ** 52
        grad = ML_COEF * ML_G * m * (2 * d if l2 else torch.sign(d))
        out[l2] = (float(terms.sum()), need(grad, F32, "gradient"))
    assert bool((d == 0).any()) and bool((d > 0).any()) and bool((d < 0).any())
    return SimpleNamespace(B=B, C=C, h=h, w=w, pred=pred, gt=gt, mask=mask, m=m, d=d, out=out)


# name, nW, window width w, canvas width Wc, x1 (unsorted), B, h
SM_ROWS = [("one_window_gaps", 1, 5, 12, (3,), 2, 3),
           ("two_unsorted", 2, 6, 12, (6, 2), 2, 3),                      # counts 0, 1, 2
           ("three_disjoint_gap", 3, 4, 14, (8, 0, 4), 2, 3),             # count 1, a gap behind
           ("four_overlapping", 4, 8, 12, (4, 0, 2, 1), 2, 3),            # counts 1, 2, 3, 4
           ("production", 3, 64, 128, (0, 32, 64), 2, 4)]                 # counts 1, 2, 3, 2, 1


def sm_widths(dtype):
    return [epc(dtype), 64]


@functools.lru_cache(maxsize=None)
def sm_case(name, C):
    """Integer windows [nW, B, h, w, C] (|.| <= 60), the exact canvas [B, h, Wc, C], the count per column and the tolerance
    where the count is 3 (zero elsewhere)"""
    _n, nW, w, Wc, x1, B, h = next(r for r in SM_ROWS if r[0] == name)
    win = N.ints((nW, B, h, w, C), 9000 + [r[0] for r in SM_ROWS].index(name) + C, 60)
    total = torch.zeros((B, h, Wc, C), dtype=torch.float64)
    cnt = torch.zeros(Wc, dtype=torch.float64)
    for k, xo in enumerate(x1):
        total[:, :, xo:xo + w] += win[k]
        cnt[xo:xo + w] += 1
    c4 = cnt.view(1, 1, Wc, 1)
    ref = torch.where(c4 > 0, total / c4.clamp_min(1), torch.zeros_like(total))
    return SimpleNamespace(nW=nW, B=B, h=h, w=w, Wc=Wc, x1=x1, C=C, win=win, ref=ref, cnt=cnt, total=total)


def sm_tolerance(ns, dtype):
    """Zero where the count divides exactly; at count 3 half an ulp of the dtype plus the two roundings of sum * fl(1 / 3)"""
    three = (ns.cnt == 3).view(1, 1, ns.Wc, 1)
    return torch.where(three, half_ulp(ns.ref, dtype) + 2 * U32 * ns.ref.abs(), torch.zeros_like(ns.ref))
