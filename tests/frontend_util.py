"""Data, float64 references, bounds and mutants for the kernels through which an image enters the model (host-only torch / numpy
code): the stem conv and the image layout entries, the range probe, the other glue kernels of csrc/misc.hip and the colour
augmentation kernels of csrc/train.hip.  Shared by tests/test_frontend_exact_host.py (the conditions, the negative controls, the
bounds held by plain f32 arithmetic) and tests/test_frontend_exact_gpu.py.  The layers are those of norm_util.py.

Layer 1 -- exact.  Inputs on which the f32 arithmetic of a kernel has ONE bit pattern, in any order, fused or not.
  stem / im2col / nhwc   normalised values n in {-1, -1/2, 0, 1/2, 1}; the image x = n std + mean for (mean, std) = (1/2, 1/2) and
                         (0, 1) is dyadic and (x - mean) fl(1 / std) gives n back exactly.  Integer weights |w| <= 2, integer
                         bias 1 <= |b| <= 3: every output is a half-integer below 64, which bf16 holds; the sums of the outputs
                         and of their squares over a whole image stay below 2^24 quanta, so every f32 partial of the fused
                         statistics is exact and the f64 statistics are.  The 27 weight rows are pairwise distinct inside every
                         16-channel tile, neighbouring channels and neighbouring tiles differ.
  latents_add_noise      moments and noise multiples of 1/4, scaling 1/2, table entries multiples of 1/8: sa lat + sn noise is a
                         multiple of 1/64 below 4.
  gray_sum               one non-zero channel holding powers of two: coefficient x value is exact, the other terms are zero and
                         the f64 sum of at most 2^17 such terms is exact.
  color_jitter           dyadic x and f (op 0), f = 1 (ops 1, 2: x 1 + m 0 and 0 + 1 x), grey pixels (op 3: s = 0, so p = q = t = v).
  blur                   integer image, dyadic weights (not symmetric) summing to 1.
  casts, clamp, copies, rows_to_f32, nhwc_to_nchw: a single rounding or none -- torch's result is the bit pattern.

Layer 2 -- a tolerance per element against float64 on random inputs: half an ulp of the output type at the reference value plus
u = 2^-24 times the COUNTED roundings times the magnitude of the element's terms (counted unfused; fusing removes roundings).
  normalisation          (x - mean) * fl(1 / std) cannot be fused (the sum comes first): it has one f32 bit pattern and is computed
                         in f32 on the CPU (``normalise32``); the image entries store THAT value rounded once.
  stem, matrix pipe      operands rounded to the dtype (exact 16-bit products), 27 products summed in f32 on top of the bias: 28
                         additions, each granted a whole ulp 2^-23 of S = sum |x w| + |b| (the 16-bit MFMA's inner adder is not
                         documented to round to nearest: head_fuse_util.classify_bound's rule).
  stem, FMA              unrounded operands, 27 fused multiply-adds: 27 u S.
  stem statistics        f64 sums of the f32 values BEFORE rounding: what the values are off by, summed, plus norm_util.stat_errors'
                         rule for an f32 partial of n terms ((n - 1) u sum |v|, n u sum v^2), n = 1024 pixels of a block.
  latents_add_noise      4: lat = m scaling, sa lat, sn noise, the sum (3 if the last product is fused).
  timestep_embedding     LIBM_ULP ulp of f32 for cosf / sinf, u |arg| for the rounded product t f_i (|cos'|, |sin'| <= 1).
  silu                   norm_util.silu_error.
  gray_sum               5 per pixel: three products, two sums, of sum |terms|.
  color_jitter 0 / 1 / 2 1 / 5 / 9: x f | (float) mean, 1 - f, their product, x f, the sum | grey (5), 1 - f, their product, f x,
                         the sum.
  color_jitter 3 (hue)   the hue in turns is off by at most E_H = (12 + |f| / 2 pi) u: mx - r, mx - g, mx - b are off by u dc each
                         (they are at most dc), so the numerator by 10 u dc, the quotient by dc and by 6 by 20 / 6 + 1 u, the
                         wrap h - floor(h) by u, 2 pi h by u, + f by (1 + |f| / 2 pi) u, h / 2 pi * 6 by 2 u, the fraction by u.
                         The output is piecewise linear in the hue with slope at most 6 v s per turn, and the map is CONTINUOUS
                         across ties of the maximum, the h - floor(h) wrap, fmod's wrap and the sector borders: a branch taken
                         differently in f32 and in f64 therefore stays inside  6 v s E_H.  Direct roundings of p, q, t:
                         s (3: dc, mx + eps, the quotient), (1 - f) (1), its product with s (1), 1 - . (1), the product with v (1):
                         u v (5 s + 3).
  blur                   ks products and ks sums of sum |w x|.

Layer 3 -- mutants of the references; the host test shows that each differs from its reference on every row it applies to.  One
listed mutant is EQUIVALENT and the host test shows that instead: "last maximum wins" gives the same hue at every tie (r = g = max:
both branches give exactly dc / dc = 1; all equal: s = 0), because HSV is continuous there."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import norm_util as N
from norm_util import F32, BF16, F16, DT3, ID3, U32, ACC_MAX, epc, half_ulp, assert_within, silu_error, need, rounded  # noqa: F401
from spatial_util import LIBM_ULP

F64 = torch.float64
GRID_CAP = 2048 * 256            # elements of one trip of the flat kernels' grid
PAST_CAP = GRID_CAP + 77         # a ragged second trip
FLAT_SIZES = [1, 255, 257, PAST_CAP]


def bits(t):
    """The bit patterns of a tensor (int32 / int16 / int64 view)"""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def inv_std32(std):
    """1.0f / std as the entry points compute it"""
    return float(np.float32(1.0) / np.float32(std))


def normalise32(img, mean, std):
    """(x - mean) * fl(1 / std) in float32, two separate operations: the one bit pattern of the kernels' normalisation"""
    return (img.float() - torch.tensor(float(mean), dtype=F32)) * torch.tensor(inv_std32(std), dtype=F32)


def gen(shape, seed, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(int(seed))) * scale


def uniform(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(tuple(shape), generator=torch.Generator().manual_seed(int(seed))) * (hi - lo) + lo


# ---- A. stem, im2col, image_to_nhwc ------------------------------------------------------------------------------------------------
STEM_N = 128
STEM_B = 2
STEM_H = [1, 5, 9, 17]                       # partial band, band border of the 4-row FMA and of the 8-row MFMA kernel
STEM_W = [1, 17, 127, 128, 129, 145]         # lone last pixel of a pair, partial 16-pixel tiles, one-pixel second segment
NORMS = [(0.5, 0.5), (0.0, 1.0)]
STEM_LDO_ODD = 132                           # a multiple of 4, not of 8: the 16-bit launch falls back to the FMA kernel
STEM_MUTANTS = ["pad_before_norm", "rs_transposed", "k_channel_major", "last_column_dropped", "halo_zero", "stats_phantom_bias",
                "stats_image0_into_1"]
STEM_REAL = [(5, 17), (9, 145), (17, 129)]
STEM_BLOCK_PIXELS = 1024                     # 8 rows x 128 pixels (the FMA kernel's block has 512)


def weight_rows_ok(wT):
    """wT [27, 128]: rows pairwise distinct inside every 16-channel tile; neighbouring channels and neighbouring tiles differ"""
    t = wT.view(27, STEM_N // 16, 16)
    pair = (t.unsqueeze(0) != t.unsqueeze(1)).any(-1).all(-1)                    # [27, 27]
    ok = bool((pair | torch.eye(27, dtype=torch.bool)).all())
    ok = ok and bool((wT[:, 1:] != wT[:, :-1]).any(0).all())
    return ok and bool((t[:, 1:] != t[:, :-1]).any(2).any(0).all())


def to_wT(w):
    """[128, 3, 3, 3] (n, c, r, s) -> [27, 128], k = (r * 3 + s) * 3 + c"""
    return w.permute(2, 3, 1, 0).reshape(27, -1).contiguous()


@functools.lru_cache(maxsize=None)
def stem_weights():
    """(w [128, 3, 3, 3] integers |w| <= 2, bias [128] integers 1 <= |b| <= 3), float64"""
    for k in range(64):
        w = N.ints((STEM_N, 3, 3, 3), 100 + k, 2)
        if weight_rows_ok(to_wT(w)):
            return w, N.signs((STEM_N,), 99, 3)
    raise AssertionError("no weight table with the stated properties")


def stem_reference(n, w, bias, mut=None, border=0.0):
    """(out [B, 128, H, W], stats [B, 128, 2]) in float64 from the NORMALISED image n [B, 3, H, W]: conv3x3 / pad 1 + bias with
    zero padding after the normalisation, and the sums of the outputs and of their squares.  ``border`` = (0 - mean) / std is what
    "pad_before_norm" puts around the image.  Mutants: STEM_MUTANTS."""
    B, _c, H, W = n.shape
    if mut == "rs_transposed":
        w = w.transpose(2, 3)
    if mut == "k_channel_major":                 # the table read at k = c * 9 + tap
        k = torch.arange(27)
        w = to_wT(w)[(k % 3) * 9 + k // 3].view(3, 3, 3, -1).permute(3, 2, 0, 1)
    xp = F.pad(n, (1, 1, 1, 1), value=border if mut == "pad_before_norm" else 0.0)
    out = F.conv2d(xp, w, bias)
    if mut == "halo_zero":                       # column x0 - 1 is missing from the window of segment x0 / 128 > 0
        w0 = w.clone()
        w0[..., 1:] = 0.0
        for x0 in range(128, W, 128):
            col = torch.zeros_like(xp)
            col[..., x0] = xp[..., x0]           # (padded index of column x0 - 1)
            out = out - F.conv2d(col, w0)
    if mut == "last_column_dropped" and W % 128:
        out = out.clone()
        out[..., W - 1] = 0.0                    # never written: the buffer's zero
    st = torch.stack([out.sum((2, 3)), (out * out).sum((2, 3))], -1)
    if mut == "stats_phantom_bias":
        cnt = (-(-H // 4) * 4) * (-(-W // 128) * 128) - H * W
        st = st + cnt * torch.stack([bias, bias * bias], -1)
    if mut == "stats_image0_into_1":
        st = st.clone()
        st[1:] += st[0]
    return out, st


def stem_mutant_applies(mut, H, W, mean):
    """A geometry condition, not an outcome"""
    return {"pad_before_norm": mean != 0.0, "rs_transposed": H > 1 or W > 1, "k_channel_major": True,
            "last_column_dropped": W % 128 != 0, "halo_zero": W > 128, "stats_phantom_bias": H % 4 != 0 or W % 128 != 0,
            "stats_image0_into_1": True}[mut]


def tokens(x):
    """[B, C, H, W] -> [B * H * W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def lattice_image(B, C, H, W, norm, seed):
    """(img f32, n float64): n in {-1, -1/2, 0, 1/2, 1}, img = n std + mean; normalise32(img) is n"""
    mean, std = norm
    n = N.ints((B, C, H, W), seed, 2, 2)
    img = need(n * std + mean, F32, "image").float()
    assert torch.equal(normalise32(img, mean, std).double(), n), "the normalisation does not give the lattice back"
    return img, n


@functools.lru_cache(maxsize=None)
def stem_case(H, W, ni):
    """Layer-1 data of one stem row: img (f32), n, the exact tokens [B * H * W, 128] and statistics, the probe's (min, max)"""
    mean, std = NORMS[ni]
    w, bias = stem_weights()
    img, n = lattice_image(STEM_B, 3, H, W, NORMS[ni], 1000 + 37 * H + W + 5000 * ni)
    out, st = stem_reference(n, w, bias)
    for dt in DT3:
        need(out, dt, "stem output")
    # every f32 partial of the statistics (per-lane, per-block: sub-sums of one image's) is exact: quanta of 1/2 and 1/4
    assert float(out.abs().sum((2, 3)).max()) * 2 < ACC_MAX and float((out * out).sum((2, 3)).max()) * 4 < ACC_MAX
    return SimpleNamespace(H=H, W=W, mean=mean, std=std, img=img, n=n, w=w, bias=bias, out=out, tok=tokens(out), stats=st,
                           lo=float(n.min()), hi=float(n.max()))


@functools.lru_cache(maxsize=None)
def stem_real_case(H, W, dtype, route):
    """Layer 2 of the stem; route "mfma" (operands rounded to the dtype) or "fma" (unrounded)"""
    mean, std = NORMS[0]
    seed = 2000 + 31 * H + W
    img = uniform((STEM_B, 3, H, W), seed)
    w, bias = (gen((STEM_N, 3, 3, 3), seed + 1) / math.sqrt(27.0)).float(), gen((STEM_N,), seed + 2).float()
    n32 = normalise32(img, mean, std)
    if route == "mfma":
        assert dtype != F32
        a, ww, unit = rounded(n32, dtype).double(), rounded(w, dtype).double(), 28 * 2.0 ** -23
    else:
        a, ww, unit = n32.double(), w.double(), 27 * U32
    ref = F.conv2d(a, ww, bias.double(), padding=1)
    S = F.conv2d(a.abs(), ww.abs(), bias.double().abs(), padding=1)
    acc = unit * S
    nb = STEM_BLOCK_PIXELS
    mag = ref.abs() + acc
    tiny = 2.0 ** -48
    tol_sum = acc.sum((2, 3)) + ((nb - 1) * U32 + tiny) * mag.sum((2, 3))
    tol_sq = (2 * ref.abs() * acc + acc * acc).sum((2, 3)) + (nb * U32 + tiny) * (mag * mag).sum((2, 3))
    return SimpleNamespace(H=H, W=W, mean=mean, std=std, img=img, w=w, bias=bias, n32=n32, a=a, ww=ww, ref=ref, tok=tokens(ref),
                           tol=tokens(half_ulp(ref, dtype) + acc), stats=torch.stack([ref.sum((2, 3)), (ref * ref).sum((2, 3))], -1),
                           tol_stats=torch.stack([tol_sum, tol_sq], -1))


def stem_emulate(ns, route):
    """The kernel's expression in plain f32 on the CPU, in its order: the bias first, then the 27 terms (c, r, s).  "fma": each
    step is round(x w + acc) (the exact product and sum taken in float64, rounded once more to f32); "mfma": exact 16-bit products
    added one at a time in f32."""
    B, _c, H, W = ns.a.shape
    xp = F.pad(ns.a, (1, 1, 1, 1))
    acc = ns.bias.view(1, -1, 1, 1).expand(B, STEM_N, H, W).clone()          # f32
    for c in range(3):
        for r in range(3):
            for s in range(3):
                p = xp[:, c, r:r + H, s:s + W].unsqueeze(1) * ns.ww[:, c, r, s].view(1, -1, 1, 1)      # float64, exact
                acc = (acc.double() + p).float() if route == "fma" else acc + p.float()
    return acc


def im2col_reference(n, Kpad, mut=None):
    """[B * H * W, Kpad] float64: k = (r * 3 + s) * 3 + c of the zero-padded normalised image, zeros from k = 27 on"""
    B, _c, H, W = n.shape
    unf = F.unfold(n, 3, padding=1).view(B, 3, 9, H * W)                     # [B, c, tap, pixel]
    rows = unf.permute(0, 3, 2, 1) if mut != "k_channel_major" else unf.permute(0, 3, 1, 2)
    return F.pad(rows.reshape(B * H * W, 27), (0, Kpad - 27))


def nhwc_reference(n, Cpad):
    return F.pad(tokens(n), (0, Cpad - n.shape[1]))


IM2COL_W = [1, 63, 64, 65]
IM2COL_H = 3
IM2COL_KPAD = [32, 64]
NHWC_C = [1, 3, 4]
NHWC_HW = (3, 5)
NHWC_BIG_W = GRID_CAP + 37                   # B = 1, C = 1, H = 1: a ragged second trip of the pixel loop


# ---- B. range probe ----------------------------------------------------------------------------------------------------------------
PROBE_TRIP = 64 * 256 * 8                    # float4 of one unrolled trip of the full grid
# n: tail only (1, 2, 3); one float4 and n & 3 = 1, 2, 3; just below one unrolled trip of a one-block grid (7 x 256 float4: only
# the remainder loop runs); two blocks; just over one unrolled trip of the full grid (1 x 3 x 419 x 419: both loops run)
PROBE_SIZES = [1, 2, 3, 5, 6, 7, 4 * 1791 + 3, 4 * 2049 + 2, 3 * 419 * 419]
PROBE_SIGNS = ["positive", "negative", "mixed", "negative_std", "neg_zero_max", "neg_zero_min"]
PROBE_POSITIONS = ["first", "body_last", "tail", "other_block"]
assert 3 * 419 * 419 // 4 > PROBE_TRIP and 3 * 419 * 419 % 4 == 3


def probe_blocks(n):
    return max(1, min(64, -(-(n // 4) // 2048)))


def probe_position(n, where):
    """The flat index of a named position, or None where the size has none"""
    n4 = n // 4
    if where == "first":
        return 0
    if where == "body_last":
        return 4 * n4 - 1 if n4 > 0 else None
    if where == "tail":
        return n - 1 if n % 4 else None
    if where == "other_block":                   # float4 number 256 + 5 belongs to thread 5 of block 1
        return 4 * (256 + 5) + 2 if probe_blocks(n) > 1 and n4 > 261 else None
    raise KeyError(where)


def probe_norm(sign):
    return (0.125, -1.25) if sign == "negative_std" else (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def probe_base(n, sign):
    """raw f32 values strictly inside the band of the sign case (the placed extremes lie outside it)"""
    lo, hi = {"positive": (0.2, 0.8), "negative": (-0.8, -0.2), "mixed": (-0.8, 0.8), "negative_std": (-0.8, 0.8),
              "neg_zero_max": (-0.8, -0.2), "neg_zero_min": (0.2, 0.8)}[sign]
    return uniform((n,), 300 + n % 1000 + PROBE_SIGNS.index(sign), lo, hi)


def probe_extremes(sign):
    """(value placed as the minimum, value placed as the maximum) of the raw data"""
    return {"positive": (0.0625, 0.9375), "negative": (-0.9375, -0.0625), "mixed": (-0.9375, 0.9375),
            "negative_std": (-0.9375, 0.9375), "neg_zero_max": (-0.9375, -0.0), "neg_zero_min": (-0.0, 0.9375)}[sign]


def probe_rows(n, sign):
    """[(what, raw data)]: the minimum at every named position with the maximum in the middle, and the other way round"""
    base = probe_base(n, sign)
    vmin, vmax = probe_extremes(sign)
    rows = []
    for which, v, other in (("min", vmin, vmax), ("max", vmax, vmin)):
        for where in PROBE_POSITIONS:
            i = probe_position(n, where)
            if i is None:
                continue
            x = base.clone()
            j = n // 2 if n // 2 != i else (n // 2 + 1) % n
            if j != i:
                x[j] = other
            x[i] = v
            rows.append((f"{which}_{where}", x))
    return rows


def probe_expected(x, mean, std):
    n32 = normalise32(x, mean, std)
    return float(n32.min()), float(n32.max())


def in_range(lo, hi):
    """The Python-side check of the probe's pair, as LdmRocm's forward and DeferredRangeCheck make it"""
    return bool(-1 <= lo and hi <= 1)


PROBE_NAN_SIZES = [3, 4 * 1791 + 3, 3 * 419 * 419]
PROBE_NAN_WHERE = ["first", "tail", "middle", "all"]


def probe_nan_row(n, where):
    x = uniform((n,), 400 + n % 1000, -0.8, 0.8)
    if where == "all":
        x[:] = float("nan")
    else:
        x[{"first": 0, "tail": n - 1, "middle": 4 * ((n // 4) // 2) + 1 if n >= 8 else n // 2}[where]] = float("nan")
    return x


# ---- C. the rest of misc.hip -------------------------------------------------------------------------------------------------------
NCHW_ROWS = [(1, 1), (3, 33), (33, 31), (64, 32), (40, 1025)]        # (C, HW)
NCHW_PREFILL = 777.25


def nchw_case(C, HW, dtype):
    """x [B * HW, ld] in the dtype (ld = C + 3), c_off = 2, Ctot = C + 3; the expected f32 [B, Ctot, HW] with the prefill elsewhere"""
    B, ld, c_off, Ctot = 2, C + 3, 2, C + 3
    x = rounded(gen((B * HW, ld), 600 + C + HW).double(), dtype)
    want = torch.full((B, Ctot, HW), NCHW_PREFILL, dtype=F32)
    want[:, c_off:c_off + C] = x[:, :C].float().view(B, HW, C).permute(0, 2, 1)
    return SimpleNamespace(B=B, C=C, HW=HW, ld=ld, c_off=c_off, Ctot=Ctot, x=x, want=want)


LAN_B, LAN_HW, LAN_LDM = 2, 37, 8
LAN_T = [0, 999]
LAN_MUTANTS = ["timestep_of_batch0", "noise_per_batch", "logvar_columns"]
LAN_ROUNDINGS = 4


def lan_reference(m, scaling, noise, sa, sn, ts, mut=None):
    """(latents [B, 4, HW], noisy [B * HW, 4], |sa lat| + |sn noise|) float64; m [B * HW, ldm], noise [4, HW], tables [1000], ts [B]"""
    B, HW = len(ts), noise.shape[1]
    cols = m[:, 4:8] if mut == "logvar_columns" else m[:, :4]
    lat = (cols * scaling).view(B, HW, 4)
    t = ts if mut != "timestep_of_batch0" else ts[torch.zeros(B, dtype=torch.long)]
    nz = noise.t().unsqueeze(0).expand(B, HW, 4)
    if mut == "noise_per_batch":                 # image b reads what lies b * 4 * HW further on: here the channels rolled by b
        nz = torch.stack([noise.roll(b, 0).t() for b in range(B)])
    a, b_ = sa[t].view(B, 1, 1) * lat, sn[t].view(B, 1, 1) * nz
    return lat.permute(0, 2, 1).contiguous(), (a + b_).view(B * HW, 4), (a.abs() + b_.abs()).view(B * HW, 4)


@functools.lru_cache(maxsize=None)
def lan_case(kind, dtype):
    """kind "lattice": see the module docstring; "real": scaling 0.18215, the scaled-linear DDPM schedule"""
    ts = torch.tensor(LAN_T)
    if kind == "lattice":
        m, noise = N.ints((LAN_B * LAN_HW, LAN_LDM), 700, 8, 4), N.ints((4, LAN_HW), 701, 8, 4)
        t = torch.arange(1000)
        sa, sn, scaling = ((t * 7) % 8 + 1).double() / 8, ((t * 3 + 2) % 8 + 1).double() / 8, 0.5
        assert float(sa[0]) != float(sa[999]) and float(sn[0]) != float(sn[999])
    else:
        m = rounded(gen((LAN_B * LAN_HW, LAN_LDM), 710, 4.0).double(), dtype).double()
        noise = gen((4, LAN_HW), 711).float().double()
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=F64) ** 2
        ac = torch.cumprod(1 - betas, 0)
        sa, sn, scaling = ac.sqrt().float().double(), (1 - ac).sqrt().float().double(), float(np.float32(0.18215))
    lat, noisy, mag = lan_reference(m, scaling, noise, sa, sn, ts)
    if kind == "lattice":
        for dt in DT3:
            need(noisy, dt, "noisy latents")
            need(m, dt, "moments")
        need(lat, F32, "latents")
    lat32 = (m[:, :4].float() * torch.tensor(scaling, dtype=F32)).view(LAN_B, LAN_HW, 4).permute(0, 2, 1).contiguous()
    return SimpleNamespace(m=m, noise=noise, sa=sa, sn=sn, scaling=scaling, ts=ts, lat=lat, lat32=lat32, noisy=noisy,
                           tol=half_ulp(noisy, dtype) + LAN_ROUNDINGS * U32 * mag)


def lan_emulate(ns):
    """plain f32, unfused: lat = m scaling; sa lat + sn noise"""
    f = lambda t: t.float()  # noqa: E731
    lat = f(ns.m[:, :4]) * torch.tensor(ns.scaling, dtype=F32)
    b = torch.arange(LAN_B).repeat_interleave(LAN_HW)
    sa, sn = f(ns.sa)[ns.ts][b].view(-1, 1), f(ns.sn)[ns.ts][b].view(-1, 1)
    return sa * lat + sn * f(ns.noise).t().repeat(LAN_B, 1)


TE_T = [0, 1, 60, 999]
TE_DIMS = [2, 320]
TE_MUTANTS = ["sin_first", "freq_of_next"]


def te_freqs(dim):
    half = dim // 2
    return torch.exp(-math.log(10000) * torch.arange(half, dtype=F32) / half)


def te_reference(ts, freqs, dtype, mut=None):
    """(embedding [B, dim] float64, tolerance): cos | sin of t f_i"""
    f = freqs.double()
    if mut == "freq_of_next":
        f = f.roll(-1)
    arg = ts.double().view(-1, 1) * f.view(1, -1)
    c, s = torch.cos(arg), torch.sin(arg)
    ref = torch.cat([s, c] if mut == "sin_first" else [c, s], 1)
    tol = half_ulp(ref, dtype) + 2 * LIBM_ULP * half_ulp(ref, F32) + U32 * torch.cat([arg, arg], 1).abs()
    return ref, tol


def silu_case(n, dtype):
    x = rounded(gen((n,), 800 + n % 999, 3.0).double(), dtype)
    z = x.double()
    y = F.silu(z)
    return x, y, half_ulp(y, dtype) + silu_error(z, torch.zeros_like(z))


CAST_SPECIALS = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65520.0, 1e-8, -3e-6,
                 2.0 ** -24, 2.0 ** -25, 1e30, -1e30, 2.0 ** -130]       # ties of bf16 and f16, f16's overflow and subnormals


def cast_input(n):
    x = gen((n,), 810 + n % 999, 10.0)
    k = min(n, len(CAST_SPECIALS))
    x[:k] = torch.tensor(CAST_SPECIALS[:k])
    return x


CLAMP_BOUNDS = [(-1.0, 1.0), (0.25, 0.25), (float("-inf"), float("inf")), (-0.5, float("inf")), (float("-inf"), -0.0), (0.0, 2.0)]


def clamp_input(n):
    x = gen((n,), 820 + n % 999, 1.5)
    sp = [float("inf"), float("-inf"), -0.0, 0.0, 0.25, -1.0, 1.0]
    k = min(n, len(sp))
    x[n - k:] = torch.tensor(sp[:k])
    return x


# ---- D. colour augmentation --------------------------------------------------------------------------------------------------------
GRAY = [float(np.float32(c)) for c in (0.299, 0.587, 0.114)]      # the kernels' coefficients, as float64
TWO_PI32 = float(np.float32(6.283185307179586))
EPS_HSV = float(np.float32(1e-8))
GRAY_HW = [1, 255, 257, 65536 + 257]         # the last: a second trip past the 256-block cap
GRAY_ROUNDINGS = 5
JIT_HW = [1, 257, GRID_CAP + 91]
JIT_ROUNDINGS = {0: 1, 1: 5, 2: 9}
JIT_HUE_F = [-0.2, 0.0, 0.2, 1.3]            # radians; 1.3 > 2 pi / 6
JIT_MUTANTS = ["gray_rb_swapped", "contrast_mean_per_channel", "clamp_missing", "hue_in_turns"]
JIT_EQUIVALENT = ["last_max_wins"]


def gray_exact_case(HW, ch):
    """[3, HW] f32 with channel ``ch`` holding 2^-k (k = 0 .. 3) and zeros elsewhere; the exact sum"""
    k = torch.randint(0, 4, (HW,), generator=torch.Generator().manual_seed(900 + HW % 999 + ch))
    img = torch.zeros((3, HW), dtype=F32)
    img[ch] = 2.0 ** -k.float()
    want = GRAY[ch] * float(img[ch].double().sum())
    assert HW * 8 < 2 ** 28          # a 24-bit coefficient times at most 2^28 eighths: every partial sum fits 52 bits
    return img, want


def gray_of64(x, mut=None):
    c = GRAY[::-1] if mut == "gray_rb_swapped" else GRAY
    return c[0] * x[0] + c[1] * x[1] + c[2] * x[2]


def gray_sum_bound(img):
    x = img.double()
    return float(gray_of64(x).sum()), float(GRAY_ROUNDINGS * U32 * gray_of64(x.abs()).sum() * (1 + 2.0 ** -20))


def jitter_reference(x, op, f, gs=None, mut=None):
    """One step on x [3, HW] float64 with the factor f (the f32 value the kernel is handed; op 3: radians) -- oracle/augment.py's
    formulas with the kernel's f32 constants; ``gs``: the grey sum handed to op 1.  Returns (out, tolerance)."""
    HW = x.shape[1]
    clamp = (lambda t: t) if mut == "clamp_missing" else (lambda t: t.clamp(0.0, 1.0))
    if op == 0:
        y = x * f
        return clamp(y), half_ulp(clamp(y), F32) + JIT_ROUNDINGS[0] * U32 * y.abs()
    if op == 1:
        mean = float(np.float32(gs / HW))
        m = torch.full((3, 1), mean * (1.0 - f), dtype=F64)
        if mut == "contrast_mean_per_channel":
            m = x.mean(1, keepdim=True) * (1.0 - f)
        if mut == "gray_rb_swapped":
            m = torch.full((3, 1), float(gray_of64(x, mut).mean()) * (1.0 - f), dtype=F64)
        y = x * f + m
        return clamp(y), half_ulp(clamp(y), F32) + JIT_ROUNDINGS[1] * U32 * ((x * f).abs() + m.abs())
    if op == 2:
        g = (1.0 - f) * gray_of64(x, mut)
        y = g + f * x
        return clamp(y), half_ulp(clamp(y), F32) + JIT_ROUNDINGS[2] * U32 * (g.abs() + (f * x).abs())
    r, g, b = x[0], x[1], x[2]
    mx, mn = x.max(0).values, x.min(0).values
    dc = mx - mn
    v, s = mx, dc / (mx + EPS_HSV)
    dc = torch.where(dc == 0, torch.ones_like(dc), dc)
    rc, gc, bc = mx - r, mx - g, mx - b
    hr, hg, hb = bc - gc, (rc - bc) + 2.0 * dc, (gc - rc) + 4.0 * dc
    if mut == "last_max_wins":
        h = torch.where(b == mx, hb, torch.where(g == mx, hg, hr))
    else:
        h = torch.where(r == mx, hr, torch.where(g == mx, hg, hb))
    h = h / dc / 6.0
    h = h - torch.floor(h)
    if mut == "hue_in_turns":
        h = torch.fmod(TWO_PI32 * (h + f), TWO_PI32)
    else:
        h = torch.fmod(TWO_PI32 * h + f, TWO_PI32)
    h6 = h / TWO_PI32 * 6.0
    hi = torch.floor(h6)
    hi = hi - 6.0 * torch.floor(hi / 6.0)
    ff = h6 - 6.0 * torch.floor(h6 / 6.0) - hi
    p, q, t = v * (1.0 - s), v * (1.0 - ff * s), v * (1.0 - (1.0 - ff) * s)
    k = hi.long() % 6
    sel = lambda tab: torch.stack(tab, 0).gather(0, k.unsqueeze(0)).squeeze(0)  # noqa: E731
    out = torch.stack([sel([v, q, p, p, t, v]), sel([t, v, v, q, p, p]), sel([p, p, t, v, v, q])], 0)
    e_h = (12.0 + abs(f) / TWO_PI32) * U32
    tol = half_ulp(out, F32) + (U32 * v * (5.0 * s + 3.0) + 6.0 * v * s * e_h).unsqueeze(0)
    return out, tol


def hsv_to_rgb64(h_turns, s, v):
    """float64 tensors -> [3, n] (the construction of the hand-placed pixels)"""
    h6 = (h_turns % 1.0) * 6.0
    k = torch.floor(h6).long() % 6
    ff = h6 - torch.floor(h6)
    p, q, t = v * (1 - s), v * (1 - ff * s), v * (1 - (1 - ff) * s)
    sel = lambda tab: torch.stack(tab, 0).gather(0, k.unsqueeze(0)).squeeze(0)  # noqa: E731
    return torch.stack([sel([v, q, p, p, t, v]), sel([t, v, v, q, p, p]), sel([p, p, t, v, v, q])], 0)


def jitter_hand_pixels(f_hue):
    """[3, n] f32: ties of the maximum, primaries and secondaries, black, greys, and for the hue shift ``f_hue`` (radians) two
    pixels within 1e-6 of a turn of each sector border after the shift"""
    px = [(0.75, 0.75, 0.25), (0.5, 0.5, 0.0), (0.25, 0.75, 0.75), (0.0, 0.625, 0.625), (0.75, 0.25, 0.75), (0.6, 0.6, 0.6),
          (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0, 0, 0), (1, 1, 1), (0.3, 0.3, 0.3),
          (0.2, 0.7, 0.7000001), (0.9, 0.9000001, 0.1), (1e-6, 0.0, 0.0), (0.5, 0.5 - 2.0 ** -24, 0.5)]
    hand = torch.tensor(px, dtype=F64).t()
    k = torch.arange(6, dtype=F64).repeat_interleave(2)
    d = torch.tensor([-5e-7, 5e-7], dtype=F64).repeat(6)
    h0 = k / 6.0 - f_hue / TWO_PI32 + d
    border = hsv_to_rgb64(h0, torch.full_like(h0, 0.5), torch.full_like(h0, 0.8))
    return torch.cat([hand, border], 1).float()


@functools.lru_cache(maxsize=None)
def jitter_image(HW, f_hue=0.0):
    """[3, HW] f32 in [0, 1]: the hand-placed pixels (as many as fit) at the END of the image -- in the last trip of the big row --
    and noise"""
    img = uniform((3, HW), 950 + HW % 999)
    hand = jitter_hand_pixels(f_hue)
    k = min(HW, hand.shape[1])
    img[:, HW - k:] = hand[:, :k]
    return img


def jitter_emulate(x, op, f, gs=None):
    """The kernel's expression in plain f32 torch operations, unfused, in its order; x [3, HW] f32"""
    f32 = lambda v: torch.tensor(float(v), dtype=F32)  # noqa: E731
    HW = x.shape[1]
    fv = f32(f)
    one = f32(1.0)
    gray = lambda t: f32(0.299) * t[0] + f32(0.587) * t[1] + f32(0.114) * t[2]  # noqa: E731
    if op == 0:
        return (x * fv).clamp(0, 1)
    if op == 1:
        m = f32(np.float32(gs / HW)) * (one - fv)
        return (x * fv + m).clamp(0, 1)
    if op == 2:
        y = (one - fv) * gray(x)
        return (y + fv * x).clamp(0, 1)
    two_pi, six = f32(TWO_PI32), f32(6.0)
    r, g, b = x[0], x[1], x[2]
    mx, mn = x.max(0).values, x.min(0).values
    dc = mx - mn
    v, s = mx, dc / (mx + f32(1e-8))
    dc = torch.where(dc == 0, torch.ones_like(dc), dc)
    rc, gc, bc = mx - r, mx - g, mx - b
    h = torch.where(r == mx, bc - gc, torch.where(g == mx, (rc - bc) + f32(2.0) * dc, (gc - rc) + f32(4.0) * dc))
    h = h / dc / six
    h = h - torch.floor(h)
    h = torch.fmod(two_pi * h + fv, two_pi)
    h6 = h / two_pi * six
    hi = torch.floor(h6)
    hi = hi - six * torch.floor(hi / six)
    ff = h6 - six * torch.floor(h6 / six) - hi
    p, q, t = v * (one - s), v * (one - ff * s), v * (one - (one - ff) * s)
    k = hi.long().clamp(0, 5)
    sel = lambda tab: torch.stack(tab, 0).gather(0, k.unsqueeze(0)).squeeze(0)  # noqa: E731
    return torch.stack([sel([v, q, p, p, t, v]), sel([t, v, v, q, p, p]), sel([p, p, t, v, v, q])], 0)


# blur: (planes, H, W, axis, ks).  L = ks / 2 + 1 on both axes (a reflection reaches the far edge), L = 2 with ks = 3, ks = 1, even
# ks, planes = 1 and 6 with H != W
BLUR_ROWS = [(1, 5, 4, 1, 7), (1, 4, 5, 0, 7), (6, 3, 2, 1, 3), (6, 2, 3, 0, 3), (1, 4, 6, 1, 1), (6, 4, 6, 0, 1), (6, 7, 3, 1, 4),
             (6, 3, 7, 0, 4), (6, 9, 13, 1, 5), (6, 9, 13, 0, 5), (1, 40, 27, 1, 9), (1, 40, 27, 0, 9)]
BLUR_MUTANTS = ["replicate", "reflect_with_edge", "axis_swapped", "plane_stride_ww"]


def blur_id(row):
    return "p{}_{}x{}_axis{}_ks{}".format(*row)


def dyadic_weights(ks):
    """ks positive multiples of a power of two that add up to 1, not symmetric (float64)"""
    a = [k + 1 for k in range(ks - 1)]
    total = 1
    while total <= sum(a) + 1:
        total *= 2
    a.append(total - sum(a))
    w = torch.tensor(a, dtype=F64) / total
    assert float(w.sum()) == 1.0 and (ks < 2 or a != a[::-1])
    return w


def blur_reference(x, axis, w, mut=None):
    """(out, sum |w x|) float64 for x [planes, H, W]: correlation along x (axis 1) or y (axis 0), reflect border without the edge"""
    P, H, W = x.shape
    ks = len(w)
    half = ks // 2
    if mut == "axis_swapped":
        axis = 1 - axis
    L = W if axis else H
    src = x
    if mut == "plane_stride_ww":                 # plane p starts at p W W of the flat buffer (wrapped into it)
        flat = x.reshape(-1)
        idx = (torch.arange(P).view(P, 1) * W * W + torch.arange(H * W).view(1, H * W)) % flat.numel()
        src = flat[idx].view(P, H, W)
    out, mag = torch.zeros_like(x), torch.zeros_like(x)
    c0 = torch.arange(L)
    for k in range(ks):
        c = c0 + k - half
        if mut == "replicate":
            c = c.clamp(0, L - 1)
        elif mut == "reflect_with_edge":
            c = torch.where(c < 0, -c - 1, c)
            c = torch.where(c >= L, 2 * L - 1 - c, c)
        else:
            c = torch.where(c < 0, -c, c)
            c = torch.where(c >= L, 2 * (L - 1) - c, c)
        c = c.clamp(0, L - 1)                    # (only a mutant on a short axis gets here out of range)
        t = float(w[k]) * (src[:, :, c] if axis else src[:, c, :])
        out, mag = out + t, mag + t.abs()
    return out, mag


def blur_mutant_applies(mut, row):
    P, H, W, axis, ks = row
    L = W if axis else H
    return {"replicate": ks > 2, "reflect_with_edge": ks > 1, "axis_swapped": ks > 1 and H > 1 and W > 1,
            "plane_stride_ww": P > 1 and H != W}[mut] and L > 1


def blur_case(row, kind):
    """kind "lattice": integer image |x| <= 255 and dyadic weights; "real": random image and a normalised Gaussian in f32"""
    P, H, W, axis, ks = row
    seed = 1100 + BLUR_ROWS.index(row)
    if kind == "lattice":
        x, w = N.ints((P, H, W), seed, 255), dyadic_weights(ks)
        assert 255 * 2.0 ** ks < ACC_MAX
    else:
        x = uniform((P, H, W), seed).double()
        g = torch.exp(-((torch.arange(ks, dtype=F32) - ks // 2 + (0.5 if ks % 2 == 0 else 0.0)) ** 2) / (2 * 0.7 ** 2))
        w = (g / g.sum()).double()
    out, mag = blur_reference(x, axis, w)
    if kind == "lattice":
        need(out, F32, "blur output")
    return SimpleNamespace(x=x, w=w, out=out, tol=half_ulp(out, F32) + 2 * ks * U32 * mag)


def blur_emulate(x, axis, w):
    """acc += w[k] * x in plain f32, unfused, k ascending"""
    P, H, W = x.shape
    ks, L = len(w), (W if axis else H)
    x32, w32 = x.float(), w.float()
    acc = torch.zeros_like(x32)
    c0 = torch.arange(L)
    for k in range(ks):
        c = c0 + k - ks // 2
        c = torch.where(c < 0, -c, c)
        c = torch.where(c >= L, 2 * (L - 1) - c, c)
        acc = acc + w32[k] * (x32[:, :, c] if axis else x32[:, c, :])
    return acc
