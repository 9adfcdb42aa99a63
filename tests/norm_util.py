"""Data, float64 references and bound functions for the normalisation kernels of the default library (host-only torch code),
shared by tests/test_norm_exact_host.py (the conditions, the negative controls) and tests/test_norm_exact_gpu.py.

Layer 1 -- exact.  The apply-type kernels and the halo convs use whatever channel sums they are handed, so the rows hand them
sums: per (image, group) a lattice mean m and a variance v with v + eps a power of four (eps = 2^-10, a dyadic, so that v is
one too).  The channel sums are s = HW (m + d_c) and q = HW (v + m^2 + d_c) with a per-channel wobble d_c that adds up to zero
over a group (a fold that misses or repeats a channel then lands on another mean); folded in f64 they give m and v up to
2^-52, which the cast to f32 removes, and rsq(v + eps) is a power of two.  With x, the residual and dy on a dyadic lattice and
small-integer gamma / beta every f32 intermediate of  x (rstd gamma) + (beta - m rstd gamma)  and of  (x - m) rstd gamma + beta
is exactly representable (the builders assert it on every intermediate, in f16 where the 16 x 16-patch conv runs the affine in
packed f16): the f32 result has ONE bit pattern and the stored value is that result rounded once to the dtype.  Every
(image, group) has its own (m, rstd), so a mix-up of group, image, source or channel offset changes bits.

The backward's group terms A_g / cnt and B_g / cnt are exact only where cnt = HW cpg is a power of two; the other rows pair
channels j and j + cpg / 2 of a group (equal x, gamma, beta, opposite dy; cpg = 1: pixels 2 i and 2 i + 1), which makes
A_g = B_g = 0 with non-zero per-channel sums.

Layer 2 -- a tolerance per element against float64 on random inputs quantised to the dtype:  half an ulp of the output type at
the reference value, plus 2^-24 (half an ulp of f32, relative) times the number of f32 roundings of the formula in
include/madm_hip.h times the magnitude of the element's terms, plus what the f32 partial sums of the statistics can be off by
(``stat_errors``: a sum of n f32 terms in any order is within (n - 1) 2^-24 sum |t| of the exact one).  v_rsq, v_rcp and v_exp
are 1 ulp = two such units each.

Layer 3 -- conditioning: max |y - y64| of stats -> apply next to F.group_norm in float32 on the same inputs."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import lattice_util as L
from det_util import ln_width_is_exact

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT3, ID3 = [F32, BF16, F16], ["f32", "bf16", "f16"]
ACC_MAX = float(1 << 24)
U32 = 2.0 ** -24                 # half an ulp of float32, relative
EPS_LATTICE = 2.0 ** -10         # the eps of every handed-statistics row
RSQ_PROBE_K = list(range(-4, 5))  # var + eps = 4^k of the first test
ACTS = ["none", "relu"]


def epc(dtype):
    return 4 if dtype == F32 else 8


# ---- exactness helpers ------------------------------------------------------------------------------------------------------------
def representable(t, dtype):
    return bool(torch.equal(t.to(dtype).double(), t))


def need(t, dtype, what):
    assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()), what
    assert representable(t, dtype), f"{what}: not representable in {dtype}"
    return t


def quantum_exp(t):
    """Smallest j >= 0 with t 2^j integer-valued everywhere."""
    for j in range(0, 41):
        s = t * 2.0 ** j
        if torch.equal(s, s.round()):
            return j
    raise AssertionError("not on a dyadic lattice of 2^-40")


def need_exact_sums(terms, dim, what, room=1.0):
    """Every partial sum over ``dim``, in any order, is exact in f32: the sum of the magnitudes, in units of the terms' common
    quantum, stays below 2^24 / room."""
    j = quantum_exp(terms)
    worst = float(terms.abs().sum(dim).max()) * 2.0 ** j
    assert worst * room < ACC_MAX, f"{what}: {worst} quanta of 2^-{j}"


def rounded(t, dtype):
    """The exact value rounded once (round-to-nearest-even) to the dtype, as a tensor of that dtype"""
    return t.float() if dtype == F32 else t.to(dtype)


def ints(shape, seed, amp, den=1):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).double() / den


def signs(shape, seed, amp=2):
    """Integers of magnitude 1 .. amp, never zero (gamma, beta: a zero would hide its neighbour)."""
    g = torch.Generator().manual_seed(int(seed))
    mag = torch.randint(1, amp + 1, tuple(shape), generator=g)
    return (mag * (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1)).double()


def act_f(z, act):
    return F.relu(z) if act == "relu" else (F.silu(z) if act == "silu" else z)


def act_grad(z, act):
    if act == "relu":
        return (z > 0).double()
    if act == "silu":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    return torch.ones_like(z)


# ---- the launchers' grids, restated (test_norm_exact_host.py holds the rows against them) -----------------------------------------
def stats_blocks(B, HW):
    """(blocks per image, rows per block) of madm_groupnorm_stats"""
    splits = max(1, min(-(-HW // 64), -(-1024 // B)))
    rpb = -(-HW // splits)
    return -(-HW // rpb), rpb


def apply_strips(B, HW, chunks):
    """(strips per image, 16-byte chunks of an image) of madm_groupnorm_apply; a thread's first four chunks are prefetched"""
    total = HW * chunks
    return max(1, min(-(-total // 1024), -(-2048 // B))), total


# ---- 1. statistics ----------------------------------------------------------------------------------------------------------------
# name, B, HW, column chunks (C = chunks * elements per 16 bytes)
STATS_ROWS = [("one_block_one_chunk", 1, 9, 1), ("ragged_b3", 3, 37, 5), ("two_column_trips", 1, 130, 257), ("ten_blocks", 2, 601, 3)]


@functools.lru_cache(maxsize=None)
def stats_case(name, C):
    _n, B, HW, _c = next(r for r in STATS_ROWS if r[0] == name)
    x = ints((B, HW, C), 11 + [r[0] for r in STATS_ROWS].index(name), 16, 8)
    terms = torch.stack([x, x * x], -1)                      # [B, HW, C, 2]
    need_exact_sums(terms[..., 0], 1, "sum x", room=2)       # (room for the accumulating second call)
    need_exact_sums(terms[..., 1], 1, "sum x^2", room=2)
    need(x, BF16, "x")
    # the kernel's f32 sums run over x - p with a pivot p that is the mean of four lattice values: differences are multiples of 1/32
    # below 4, their squares multiples of 1/1024 below 16, and a block adds at most rows-per-block of them
    assert stats_blocks(B, HW)[1] * 16 * 1024 < ACC_MAX
    return SimpleNamespace(B=B, HW=HW, C=C, x=x, terms=terms)


def stats_sums(ns, weight=None):
    """f64 [B, C, 2]; ``weight`` [B, HW] (None = ones): a row dropped is a zero in it"""
    t = ns.terms if weight is None else ns.terms * weight.view(ns.B, ns.HW, 1, 1)
    return t.sum(1)


# ---- handed statistics ------------------------------------------------------------------------------------------------------------
def handed_stats(B, HW, cins, G, coarse):
    """Per-source channel sums [B, C_i, 2] (f64) whose groups fold to a lattice mean and a power-of-two rstd, both [B, G]."""
    Ctot = sum(cins)
    assert Ctot % G == 0
    cpg = Ctot // G
    b, g = torch.arange(B).view(B, 1), torch.arange(G).view(1, G)
    if coarse:       # integer means, rstd in {1, 1/2}: leaves bits for the A_g / cnt, B_g / cnt terms of the backward
        mean, k = ((b + 2 * g) % 3 - 1).double(), ((b + g) % 2).double()
    else:
        mean, k = ((3 * b + 5 * g) % 9 - 4).double() / 8, ((b + g) % 3 - 1).double()
    rstd = 2.0 ** -k
    var = 4.0 ** k - EPS_LATTICE
    j = (torch.arange(Ctot) % cpg).double()
    d = ((2 * j - (cpg - 1)) / 8).view(1, Ctot)              # adds up to zero over a group
    mc, vc = mean.repeat_interleave(cpg, 1), var.repeat_interleave(cpg, 1)
    sums = torch.stack([HW * (mc + d), HW * (vc + mc * mc + d)], -1)
    return list(torch.split(sums, list(cins), 1)), mean, rstd


def fold_sums(sums, HW, G, eps, mut=None):
    """(mean, rstd) [B, G] of the header's statement, in float64: group sums of the concatenated channel sums / count.
    Mutations: "second_source_offset" (channels of source 2 read source 1's sums at their own index), "count_from_c1" (the
    count taken from the first source's channels instead of Ctot), "no_eps"."""
    sums = [s.clone() for s in sums]
    C1 = sums[0].shape[1]
    if mut == "second_source_offset" and len(sums) > 1:
        C2 = sums[1].shape[1]
        sums[1] = sums[0][:, torch.arange(C2) % C1]
    cat = torch.cat(sums, 1)
    B, Ctot, _ = cat.shape
    cpg = Ctot // G
    cnt = float(HW) * (C1 // G if mut == "count_from_c1" else cpg)
    gs = cat.view(B, G, cpg, 2).sum(2)
    mean = gs[..., 0] / cnt
    var = (gs[..., 1] / cnt - mean * mean).clamp_min(0.0)
    return mean, (var + (0.0 if mut == "no_eps" else eps)) ** -0.5


def _per_channel(stat, cpg, mut=None):
    """[B, G] -> [B, 1, Ctot]; "group_off_by_one": channel c takes the group of channel c + 1; "next_image": image b takes b + 1's"""
    c = stat.repeat_interleave(cpg, 1)
    if mut == "group_off_by_one":
        c = torch.cat([c[:, 1:], c[:, -1:]], 1)
    if mut == "next_image":
        c = c.roll(-1, 0)
    return c.unsqueeze(1)


def gn_forward(x, mean, rstd, gamma, beta, act="none", res=None, mut=None, exact=None, C1=None):
    """y [B, HW, Ctot] = act((x - mean_g) rstd_g gamma + beta + res), float64.  ``exact``: a dtype in which every intermediate of
    both orders of evaluation must be representable (asserted).  Mutations: those of ``_per_channel``, "c_off_ignored" (the second
    source takes gamma / beta from index 0), "res_after_act"."""
    B, HW, Ctot = x.shape
    cpg = Ctot // mean.shape[1]
    mc, rc = _per_channel(mean, cpg, mut), _per_channel(rstd, cpg, mut)
    if mut == "c_off_ignored":
        gamma, beta = (torch.cat([v[:C1], v[:Ctot - C1]]) for v in (gamma, beta))
    sc = rc * gamma
    sh = beta - mc * sc
    z = x * sc + sh
    if exact is not None:
        for name, t in (("scale", sc), ("mean * scale", mc * sc), ("shift", sh), ("x * scale", x * sc), ("z", z),
                        ("x - mean", x - mc), ("(x - mean) rstd", (x - mc) * rc), ("(x - mean) rstd gamma", (x - mc) * sc)):
            need(t, exact, name)
    if res is not None and mut != "res_after_act":
        z = z + res
        if exact is not None:
            need(z, exact, "z + residual")
    y = act_f(z, act)
    return y + res if (res is not None and mut == "res_after_act") else y


def gn_backward(x, dy, mean, rstd, gamma, beta, act="none", dres=None, mut=None, exact=False, weight=None):
    """Backward of ``gn_forward`` without its residual, float64: namespace of dx [B, HW, Ctot], bsums [B, Ctot, 2] (S1 = sum dz,
    S2 = sum dz xh), dgamma, dbeta [Ctot].  ``exact``: assert every f32 intermediate and partial sum.  ``weight`` [B, HW]: row
    weights of the sums (a dropped row).  Mutations: "A_dropped", "B_dropped", "dgamma_dbeta_swapped"."""
    B, HW, Ctot = x.shape
    G = mean.shape[1]
    cpg = Ctot // G
    cnt = float(HW * cpg)
    mc, rc = _per_channel(mean, cpg), _per_channel(rstd, cpg)
    mr = -mc * rc
    xh = x * rc + mr
    z = xh * gamma + beta
    dz = dy * act_grad(z, act)
    t2 = dz * xh
    w = 1.0 if weight is None else weight.view(B, HW, 1)
    S1, S2 = (dz * w).sum(1), (t2 * w).sum(1)
    kA = _per_channel((gamma * S1).view(B, G, cpg).sum(2) / cnt, cpg)
    kB = _per_channel((gamma * S2).view(B, G, cpg).sum(2) / cnt, cpg)
    if mut == "A_dropped":
        kA = torch.zeros_like(kA)
    if mut == "B_dropped":
        kB = torch.zeros_like(kB)
    inner = gamma * dz - kA - xh * kB
    dx = rc * inner
    if exact:
        for name, t in (("-mean rstd", mr), ("x rstd", x * rc), ("xh", xh), ("xh gamma", xh * gamma), ("z", z), ("dz xh", t2),
                        ("A / cnt", kA), ("B / cnt", kB), ("gamma dz - A / cnt", gamma * dz - kA), ("xh B / cnt", xh * kB),
                        ("inner", inner), ("dx", dx)):
            need(t, F32, name)
        need_exact_sums(dz, 1, "S1")
        need_exact_sums(t2, 1, "S2")
        need_exact_sums(S1, 0, "dbeta", room=2)           # (room for the non-zero buffers it is accumulated into)
        need_exact_sums(S2, 0, "dgamma", room=2)
    if dres is not None:
        dx = dx + dres
        if exact:
            need(dx, F32, "dx + dres")
    dgamma, dbeta = S2.sum(0), S1.sum(0)
    if mut == "dgamma_dbeta_swapped":
        dgamma, dbeta = dbeta, dgamma
    return SimpleNamespace(dx=dx, bsums=torch.stack([S1, S2], -1), dgamma=dgamma, dbeta=dbeta, kA=kA, kB=kB, z=z, xh=xh, dz=dz)


# ---- 2. / 3. the GroupNorm rows ---------------------------------------------------------------------------------------------------
# name, B, HW, sources, G
GN_ROWS = [("c64", 2, 35, (64,), 32),
           ("cpg10", 2, 35, (320,), 32),                  # a 16-byte chunk straddles groups
           ("one_group_tail", 1, 16, (128,), 1),          # 128 channels per group: the fold's tail past 80; cnt = 2048
           ("straddle4", 2, 7, (64, 128), 4),             # group 1 straddles the sources
           ("wide_concat", 1, 5, (1280, 640), 32),
           ("g64_per_channel", 2, 9, (64,), 64),          # a second pass of the g0 += 32 loop, G = C
           ("pow2_count", 2, 16, (64,), 32)]              # cnt = 32: non-zero A_g / cnt, B_g / cnt with two channels per group
BIG_ROW = ("prefetch_overrun", 256, 130, 64, 32)          # B, HW, chunks per row, G: 8320 chunks per image > 8 strips x 1024


def gn_row(name, dtype=None):
    if name == BIG_ROW[0]:
        return BIG_ROW[1], BIG_ROW[2], (BIG_ROW[3] * epc(dtype),), BIG_ROW[4]
    return next(r for r in GN_ROWS if r[0] == name)[1:]


def is_pow2(n):
    return n & (n - 1) == 0


@functools.lru_cache(maxsize=None)
def gn_case(name, C_big=None, paired=False):
    """The data of one row: x, res, dy, dres [B, HW, Ctot], gamma, beta, the handed sums and the (mean, rstd) they fold to.
    ``paired`` (the backward's rows whose count is no power of two): see the module docstring."""
    if name == BIG_ROW[0]:
        B, HW, cins, G = BIG_ROW[1], BIG_ROW[2], (C_big,), BIG_ROW[4]
    else:
        B, HW, cins, G = gn_row(name)
    Ctot = sum(cins)
    cpg = Ctot // G
    coarse = is_pow2(HW * cpg)
    seed = 700 + 10 * ([r[0] for r in GN_ROWS] + [BIG_ROW[0]]).index(name)
    den = 1 if coarse else 8
    ns = SimpleNamespace(name=name, B=B, HW=HW, cins=cins, G=G, Ctot=Ctot, cpg=cpg, coarse=coarse, paired=paired and not coarse,
                         eps=EPS_LATTICE)
    ns.x = ints((B, HW, Ctot), seed, 4 if coarse else 16, den)
    ns.res = ints((B, HW, Ctot), seed + 1, 8, 8)
    ns.dy = ints((B, HW, Ctot), seed + 2, 3)
    ns.dres = ints((B, HW, Ctot), seed + 3, 8, 8)
    ns.gamma, ns.beta = signs((Ctot,), seed + 4), signs((Ctot,), seed + 5)
    if ns.paired and cpg % 2 == 0:
        c = torch.arange(Ctot)
        src = c - torch.where(c % cpg >= cpg // 2, cpg // 2, 0)
        sign = torch.where(c % cpg >= cpg // 2, -1.0, 1.0).double()
        ns.x, ns.gamma, ns.beta = ns.x[..., src], ns.gamma[src], ns.beta[src]
        ns.dy = ns.dy[..., src] * sign
    elif ns.paired:
        p = torch.arange(HW)
        src = p - p % 2
        sign = torch.where(p % 2 == 1, -1.0, 1.0).double()
        if HW % 2:
            src[-1], sign[-1] = HW - 1, 0.0
        ns.x = ns.x[:, src]
        ns.dy = ns.dy[:, src] * sign.view(1, HW, 1)
    ns.sums, ns.mean, ns.rstd = handed_stats(B, HW, cins, G, coarse)
    return ns


def check_handed(ns):
    """The handed sums fold (float64, the header's statement) to the designed mean and rstd up to f64 rounding, and exactly
    after the casts to f32 that the kernels make; mean and rstd differ between neighbouring groups and images."""
    mean, rstd = fold_sums(ns.sums, ns.HW, ns.G, ns.eps)
    assert torch.equal(mean.float().double(), ns.mean) and float((mean - ns.mean).abs().max()) < 1e-13
    assert float((rstd / ns.rstd - 1).abs().max()) < 1e-12
    cat = torch.cat(ns.sums, 1).view(ns.B, ns.G, ns.cpg, 2).sum(2)
    var32 = (cat[..., 1] / (ns.HW * ns.cpg) - mean * mean).float()
    total = (var32 + torch.tensor(ns.eps, dtype=F32)).double()
    assert torch.equal(total, ns.rstd ** -2), "var + eps is not the power of four in f32"
    if ns.G > 1:
        assert bool((ns.mean[:, 1:] != ns.mean[:, :-1]).all()) and bool((ns.rstd[:, 1:] != ns.rstd[:, :-1]).all())
    if ns.B > 1:
        assert bool((ns.mean[1:] != ns.mean[:-1]).all())
    for s in ns.sums:
        need(s, torch.float64, "sums")
        assert quantum_exp(s) <= 13


def gn_forward_case(ns, act, with_res, mut=None, exact=True):
    return gn_forward(ns.x, ns.mean, ns.rstd, ns.gamma, ns.beta, act, ns.res if with_res else None, mut,
                      F16 if exact else None, ns.cins[0])


def finalize_reference(ns):
    """(scale, shift) [B, Ctot] of madm_groupnorm_finalize"""
    sc = _per_channel(ns.rstd, ns.cpg)[:, 0] * ns.gamma
    return sc, ns.beta - _per_channel(ns.mean, ns.cpg)[:, 0] * sc


def gn_backward_case(ns, act, with_dres, mut=None, weight=None):
    assert ns.coarse or ns.paired
    return gn_backward(ns.x, ns.dy, ns.mean, ns.rstd, ns.gamma, ns.beta, act, ns.dres if with_dres else None, mut,
                       exact=mut is None and weight is None, weight=weight)


# ---- 4. the fused GroupNorm input of the halo convs -------------------------------------------------------------------------------
HALO_NAMES = {4: "conv3x3_halo_x128", 5: "conv3x3_halo_x64", 9: "conv3x3_halo_dma_x128", 10: "conv3x3_halo_dma_x64",
              12: "conv3x3_h16_x128"}
# name, B, sources, H, W, Cout, tile codes: the shapes of test_conv_fused_groupnorm_input with Cout <= 128, and of the fused rows
# of H16_CASES for the 16 x 16-patch kernel (which the planner replaces on maps under 16 x 16)
CONV_GN_ROWS = [("x128", 2, (128,), 16, 32, 128, (4, 9, 12)),
                ("c320", 2, (320,), 16, 16, 64, (5, 10, 12)),
                ("ragged", 1, (64,), 11, 19, 64, (5, 9)),
                ("ragged_h16", 1, (64,), 19, 23, 64, (12,)),
                ("concat", 2, (128, 64), 8, 16, 128, (5,)),             # six channels per group; group 21 straddles
                ("concat_straddle", 2, (1280, 640), 8, 16, 64, (5, 10)),
                ("concat_straddle_h16", 2, (1280, 640), 16, 16, 64, (12,))]
CONV_GN_G = 32


@functools.lru_cache(maxsize=None)
def conv_gn_reference(name, act, mut=None):
    """conv3x3(act(GroupNorm([x | skip]))) + bias with handed statistics, in the manner of lattice_util.conv_reference: the
    normalised input y is a multiple of 1/8 that bf16 holds, the weights are +-1 at lattice_util's density, and
    Kred amp_a amp_b < 2^24 in units of y's quantum, so the f32 accumulator is exact in any order.  ``out`` NCHW float64; the
    kernel's output is ``out`` rounded once to its dtype.  mut "pad_before_act": the zero padding goes through the affine
    and the activation like a pixel."""
    _n, B, cins, H, W, Cout, _t = next(r for r in CONV_GN_ROWS if r[0] == name)
    Ctot, G = sum(cins), CONV_GN_G
    seed = 900 + [r[0] for r in CONV_GN_ROWS].index(name)
    x = ints((B, H * W, Ctot), seed, 8, 4)
    gamma, beta = signs((Ctot,), seed + 20), signs((Ctot,), seed + 40)
    sums, mean, rstd = handed_stats(B, H * W, cins, G, False)
    kred = 9 * Ctot
    w = L.lattice((Cout, Ctot, 3, 3), seed + 60, 1, L.exact_density(kred))
    bias = L.small_dense((Cout,), seed + 80)
    if mut == "pad_before_act":
        xp = F.pad(x.view(B, H, W, Ctot), (0, 0, 1, 1, 1, 1)).view(B, (H + 2) * (W + 2), Ctot)
        y = gn_forward(xp, mean, rstd, gamma, beta, act).view(B, H + 2, W + 2, Ctot).permute(0, 3, 1, 2)
        out = F.conv2d(y, w, bias)
    else:
        y = gn_forward(x, mean, rstd, gamma, beta, act, exact=F16)
        need(y, BF16, "the normalised input")
        y = y.view(B, H, W, Ctot).permute(0, 3, 1, 2)
        out = F.conv2d(y, w, bias, padding=1)
    j = quantum_exp(y)
    amp_a = float(y.abs().max()) * 2.0 ** j
    assert j <= 4 and kred * amp_a * 1.0 < ACC_MAX, (kred, amp_a, j)
    need(out, F32, "conv output")
    return SimpleNamespace(B=B, cins=cins, H=H, W=W, Cout=Cout, G=G, x=x, gamma=gamma, beta=beta, sums=sums, mean=mean, rstd=rstd,
                           w=w, bias=bias, y=y, out=out, eps=EPS_LATTICE, HW=H * W, cpg=Ctot // G, kred=kred)


# ---- 5. LayerNorm -----------------------------------------------------------------------------------------------------------------
LN_M = [1, 5, 9]


def ln_widths(dtype):
    """one chunk; 65 chunks (lane 0 owns a second one); 320; 512 (a power of two: non-zero row means of the backward); 1280 (the
    f32 limit of 5 chunks per lane); 2560 (16-bit only)"""
    e = epc(dtype)
    return [e, 65 * e, 320, 512, 1280] + ([2560] if dtype != F32 else [])


LN_STRIDE_ROW = 517              # rows of two chunks: the backward's 128-block grid strides over them


@functools.lru_cache(maxsize=None)
def ln_case(M, C):
    """Rows of +-2^k in equal numbers (k = row % 5 - 2) with eps = 0: mean 0, rstd 2^-k.  C a power of two: dy free, the row
    means m1 = sum gamma dy / C and m2 are exact; otherwise channels c and c + C / 2 carry equal x and gamma and opposite dy,
    so m1 = m2 = 0 and dx = rstd gamma dy (+ dres)."""
    assert C % 4 == 0 and ln_width_is_exact(C)
    seed = 1300 + 7 * M + C
    g = torch.Generator().manual_seed(seed)
    pow2 = is_pow2(C)
    n = C if pow2 else C // 2
    half = torch.cat([torch.ones(n // 2), -torch.ones(n // 2)]).double()
    k = (torch.arange(M) % 5 - 2).double()
    x = torch.stack([half[torch.randperm(n, generator=g)] for _ in range(M)])
    gamma, beta = signs((n,), seed + 1), signs((C,), seed + 2)
    dy = ints((M, n), seed + 3, 3)
    if not pow2:
        x, gamma, dy = torch.cat([x, x], 1), torch.cat([gamma, gamma]), torch.cat([dy, -dy], 1)
    x = x * (2.0 ** k).view(M, 1)
    dres = ints((M, C), seed + 4, 8, 8)
    ns = SimpleNamespace(M=M, C=C, x=x, gamma=gamma, beta=beta, dy=dy, dres=dres, rstd=(2.0 ** -k).view(M, 1), pow2=pow2)
    assert float(x.sum(1).abs().max()) == 0.0
    need_exact_sums(x, 1, "row sum")
    need_exact_sums(x * x, 1, "row sum of squares")
    assert torch.equal((x * x).sum(1) / C, (4.0 ** k))
    return ns


def ln_forward(x, gamma, beta, eps, mean=None, rstd=None):
    if mean is None:
        mean = x.mean(1, keepdim=True)
        rstd = (((x - mean) ** 2).mean(1, keepdim=True) + eps) ** -0.5
    return (x - mean) * rstd * gamma + beta


def ln_backward(x, dy, gamma, eps, dres=None, mean=None, rstd=None, mut=None, exact=False):
    C = x.shape[1]
    if mean is None:
        mean = x.mean(1, keepdim=True)
        rstd = (((x - mean) ** 2).mean(1, keepdim=True) + eps) ** -0.5
    xh = (x - mean) * rstd
    gd = gamma * dy
    m1, m2 = gd.sum(1, keepdim=True) / C, (gd * xh).sum(1, keepdim=True) / C
    if mut == "A_dropped":
        m1 = torch.zeros_like(m1)
    if mut == "B_dropped":
        m2 = torch.zeros_like(m2)
    inner = gd - m1 - xh * m2
    dx = rstd * inner
    if exact:
        for name, t in (("xh", xh), ("gamma dy", gd), ("gamma dy xh", gd * xh), ("m1", m1), ("m2", m2), ("xh m2", xh * m2),
                        ("gamma dy - m1", gd - m1), ("inner", inner), ("dx", dx)):
            need(t, F32, name)
        need_exact_sums(gd, 1, "m1")
        need_exact_sums(gd * xh, 1, "m2")
        need_exact_sums(dy * xh, 0, "dgamma", room=2)
        need_exact_sums(dy, 0, "dbeta", room=2)
    if dres is not None:
        dx = dx + dres
        if exact:
            need(dx, F32, "dx + dres")
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    if mut == "dgamma_dbeta_swapped":
        dgamma, dbeta = dbeta, dgamma
    return SimpleNamespace(dx=dx, dgamma=dgamma, dbeta=dbeta, xh=xh, m1=m1, m2=m2, rstd=rstd)


def ln_exact(ns, with_dres=True, mut=None):
    zero = torch.zeros((ns.M, 1), dtype=torch.float64)
    y = need(ln_forward(ns.x, ns.gamma, ns.beta, 0.0, zero, ns.rstd), BF16, "LayerNorm output")
    bw = ln_backward(ns.x, ns.dy, ns.gamma, 0.0, ns.dres if with_dres else None, zero, ns.rstd, mut, exact=mut is None)
    return y, bw


# the LayerNorm-folded linear on rows of +-1 (mean 0, variance 1): M, C, N, tile codes (13 = the A-stationary kernel, 3 = 64 x 64)
LN_FOLD_ROW = (70, 320, 128, (13, 3))
LN_FOLD_EPS = 2.0 ** -30         # the entry point wants eps > 0; 1 + 2^-30 is 1.0f


@functools.lru_cache(maxsize=None)
def ln_fold_reference():
    """out = LN(x) W^T + b = x (W gamma)^T + (W beta + b) on rows of +-1: the plain exact linear of lattice_util's kind (weights
    +-1 at its density, integer gamma / beta / bias), all integers below 2^24 in any order."""
    M, C, N, _t = LN_FOLD_ROW
    g = torch.Generator().manual_seed(77)
    half = torch.cat([torch.ones(C // 2), -torch.ones(C // 2)]).double()
    x = torch.stack([half[torch.randperm(C, generator=g)] for _ in range(M)])
    w = L.lattice((N, C), 78, 1, L.exact_density(C))
    gamma, beta, b = signs((C,), 79), signs((C,), 80), L.small_dense((N,), 81)
    out = F.linear(ln_forward(x, gamma, beta, 0.0, torch.zeros(M, 1).double(), torch.ones(M, 1).double()), w, b)
    assert torch.equal(out, F.linear(x, w * gamma, F.linear(beta, w) + b))
    assert torch.equal(out, out.round()) and C * 1.0 * 2.0 < ACC_MAX and float(out.abs().max()) <= L.EXACT_OUT_MAX[BF16]
    assert ln_width_is_exact(C) and float(torch.tensor(1.0, dtype=F32) + torch.tensor(LN_FOLD_EPS, dtype=F32)) == 1.0
    return SimpleNamespace(M=M, C=C, N=N, x=x, w=w, gamma=gamma, beta=beta, b=b, out=out)


# ---- layer 2: data, float64 references from the stored inputs, bounds --------------------------------------------------------------
def quantised(shape, seed, dtype, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(tuple(shape), generator=g) * scale + shift).to(dtype).double()


def half_ulp(ref, dtype):
    """Half an ulp of ``dtype`` at |ref| (the subnormal spacing below the smallest normal), float64"""
    p, emin = {F32: (24, -126), BF16: (8, -126), F16: (11, -14)}[dtype]
    _m, e = torch.frexp(ref.abs().double())            # |ref| = m 2^e, m in [0.5, 1): the binade starts at 2^(e - 1)
    e = torch.where(ref == 0, torch.full_like(e, emin + 1), e).clamp_min(emin + 1)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - p - 1)


def real_stats(x, G, eps):
    """float64 (mean, var, rstd) [B, G] of x [B, HW, Ctot]"""
    B, HW, Ctot = x.shape
    xg = x.view(B, HW, G, Ctot // G)
    mean = xg.mean((1, 3))
    var = (xg * xg).mean((1, 3)) - mean * mean
    return mean, var, (var + eps) ** -0.5


def stat_errors(x, G, eps, n_terms):
    """What f32 partial sums of ``n_terms`` terms (in any order; f64 across partials) can move the group mean and the relative
    rstd by: |d sum x| <= (n - 1) u sum |x|, |d sum x^2| <= n u sum x^2 (one more for the square), u = 2^-24; then
    var = E x^2 - mean^2 and rstd = (var + eps)^-1/2 to first order, plus the casts of mean and var + eps to f32 and the
    1-ulp v_rsq (4 u)."""
    B, HW, Ctot = x.shape
    cnt = HW * (Ctot // G)
    xg = x.view(B, HW, G, Ctot // G)
    mean, var, _r = real_stats(x, G, eps)
    dm = (n_terms - 1) * U32 * xg.abs().sum((1, 3)) / cnt
    dv = n_terms * U32 * (xg * xg).sum((1, 3)) / cnt + 2 * mean.abs() * dm + dm * dm
    drel = dv / (2 * (var + eps)) + 4 * U32
    return dm + U32 * mean.abs(), drel


N_FWD = 6     # x - mean, * rstd, * gamma, + beta, + residual, and the product rstd gamma of the scale / shift form


def silu_error(z, dz):
    """|silu(z') - silu(z)| for |z' - z| <= dz plus the f32 evaluation z / (1 + exp(-z)): |silu'| <= 1.1; exp's argument is a
    rounded product (relative error |z| u in exp(-z), twice for the rounded constant), v_exp and v_rcp 1 ulp each (2 u), the add
    and the final product (u each)"""
    s = torch.sigmoid(z)
    return 1.1 * dz + U32 * (8 * (z * s).abs() + 2 * z * z * s * (1 - s))


def gn_forward_bound(x, gamma, beta, G, eps, act, res, dtype, n_terms):
    """Per-element tolerance [B, HW, Ctot] of act(GroupNorm(x) + res) computed from statistics with f32 partial sums"""
    B, HW, Ctot = x.shape
    cpg = Ctot // G
    mean, _v, rstd = real_stats(x, G, eps)
    dm, drel = stat_errors(x, G, eps, n_terms)
    mc, rc, dmc, drc = (_per_channel(t, cpg) for t in (mean, rstd, dm, drel))
    sc = (rc * gamma).abs()
    terms = x.abs() * sc + mc.abs() * sc + beta.abs() + (res.abs() if res is not None else 0.0)
    dz = U32 * N_FWD * terms + sc * dmc + (x - mc).abs() * sc * drc
    z = (x - mc) * rc * gamma + beta + (res if res is not None else 0.0)
    y = act_f(z, act)
    inner = silu_error(z, dz) if act == "silu" else dz      # ReLU is 1-Lipschitz
    return half_ulp(y, dtype) + inner


def gn_backward_bound(x, dy, gamma, beta, G, eps, act, dres, dtype, n_terms, n_sum):
    """Tolerances of (dx [B, HW, Ctot], dgamma, dbeta [Ctot]) for act "none" / "silu"; ``n_sum`` = terms of an f32 partial sum of
    the backward's S1 / S2"""
    assert act in ("none", "silu")
    B, HW, Ctot = x.shape
    cpg = Ctot // G
    cnt = float(HW * cpg)
    mean, _v, rstd = real_stats(x, G, eps)
    dm, drel = stat_errors(x, G, eps, n_terms)
    mc, rc, dmc, drc = (_per_channel(t, cpg) for t in (mean, rstd, dm, drel))
    ref = gn_backward(x, dy, mean, rstd, gamma, beta, act)
    xh = ref.xh
    dxh = rc * dmc + xh.abs() * drc + 3 * U32 * (x.abs() * rc + (mc * rc).abs())
    if act == "silu":
        dzz = dxh * gamma.abs() + 2 * U32 * ((xh * gamma).abs() + beta.abs())
        # silu'' is bounded by 1/2; sigmoid and the polynomial around it: ~12 roundings of terms below 1.1, + |z| u from exp's argument
        ddz = dy.abs() * (0.5 * dzz + U32 * (12 + 2 * ref.z.abs()) * 1.1)
    else:
        ddz = torch.zeros_like(x)
    t2 = ref.dz * xh
    dS1 = ddz.sum(1) + n_sum * U32 * ref.dz.abs().sum(1)
    dS2 = (ddz * xh.abs() + ref.dz.abs() * dxh).sum(1) + (n_sum + 1) * U32 * t2.abs().sum(1)
    g1 = gamma.abs()
    dA = _per_channel((g1 * dS1).view(B, G, cpg).sum(2) / cnt, cpg) + U32 * ref.kA.abs()
    dB = _per_channel((g1 * dS2).view(B, G, cpg).sum(2) / cnt, cpg) + U32 * ref.kB.abs()
    terms = (gamma * ref.dz).abs() + ref.kA.abs() + (xh * ref.kB).abs()
    inner = g1 * ddz + dA + xh.abs() * dB + ref.kB.abs() * dxh + 4 * U32 * terms
    core = rc * (gamma * ref.dz - ref.kA - xh * ref.kB)
    ddx = rc * inner + core.abs() * (drc + U32) + (U32 * (core.abs() + dres.abs()) if dres is not None else 0.0)
    out = ref.dx + dres if dres is not None else ref.dx
    tol_dx = half_ulp(out, dtype) + ddx
    S1, S2 = ref.bsums[..., 0], ref.bsums[..., 1]
    tol_db = half_ulp(ref.dbeta, F32) + dS1.sum(0) + (B + 1) * U32 * S1.abs().sum(0)
    tol_dg = half_ulp(ref.dgamma, F32) + dS2.sum(0) + (B + 1) * U32 * S2.abs().sum(0)
    return SimpleNamespace(ref=ref, out=out, tol_dx=tol_dx, tol_dgamma=tol_dg, tol_dbeta=tol_db)


def ln_forward_bound(x, gamma, beta, eps, dtype):
    """two-pass LayerNorm in f32: the row sum and the sum of squared deviations of C terms each (any order)"""
    M, C = x.shape
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    dm = C * U32 * x.abs().mean(1, keepdim=True)
    dv = (C + 2) * U32 * var + 2 * d.abs().mean(1, keepdim=True) * dm + dm * dm
    drel = dv / (2 * (var + eps)) + 4 * U32
    y = d * rstd * gamma + beta
    terms = (x.abs() + mean.abs()) * rstd * gamma.abs() + beta.abs()
    return half_ulp(y, dtype) + U32 * 5 * terms + (rstd * gamma).abs() * dm + (d * rstd * gamma).abs() * drel


SOFTMAX_L = [4, 252, 256, 260, 4096]
SOFTMAX_ROWS = 5


def softmax_case(L_, scale):
    """f32 logits [5, L]: four random rows of spread 4 / scale, one row of equal logits"""
    g = torch.Generator().manual_seed(2000 + L_)
    s = (torch.randn((SOFTMAX_ROWS, L_), generator=g) * 4.0 / scale).float()
    s[3] = 1.375 / scale
    return s


def softmax_bound(s, scale, dtype):
    """(p, tolerance, relative f32 error) of softmax(scale s) over rows, float64.  p_i = 2^(s_i c - max c) / sum with
    c = scale log2 e rounded to f32: the exponent carries the rounding of c (twice: the constant and the product), of both
    products and of the difference; v_exp is 1 ulp; one wave sums a row: ceil(L / 64) terms per lane and a six-level butterfly;
    the reciprocal (1 ulp) and the final product."""
    sd = s.double()
    L_ = s.shape[1]
    p = torch.softmax(sd * scale, 1)
    c = scale * math.log2(math.e)
    mx = sd.max(1, keepdim=True).values
    e2 = U32 * (2 * (sd - mx).abs() * abs(c) + (sd * c).abs() + (mx * c).abs() + ((sd - mx) * c).abs())
    rel_e = math.log(2.0) * e2 + 2 * U32
    rel_sum = (p * rel_e).sum(1, keepdim=True) + (-(-L_ // 64) + 6) * U32
    rel = rel_e + rel_sum + 3 * U32
    return p, half_ulp(p, dtype) + p * rel, rel


# ---- layer 3 ----------------------------------------------------------------------------------------------------------------------
COND_MU = [0, 4, 16, 64]
COND_ROWS = [("hw600_c320", 1, 600, 320, 32), ("hw61_c64", 2, 61, 64, 32)]
COND_FACTOR = 4.0     # E_kernel <= 4 E_torch32: a margin over the reference's arithmetic (a model of this apply formula with
#                       accurate statistics and a 1-ulp rsq lands at 1.2 - 1.4 x F.group_norm in float32)


def cond_case(name, mu):
    _n, B, HW, C, G = next(r for r in COND_ROWS if r[0] == name)
    g = torch.Generator().manual_seed(3000 + int(mu))
    x = (torch.randn((B, HW, C), generator=g) + float(mu)).float()
    y64 = F.group_norm(x.double().permute(0, 2, 1), G, eps=1e-5).permute(0, 2, 1)
    y32 = F.group_norm(x.permute(0, 2, 1), G, eps=1e-5).permute(0, 2, 1)
    return SimpleNamespace(B=B, HW=HW, C=C, G=G, x=x, y64=y64, e_torch=float((y32.double() - y64).abs().max()))


def cond_ln_case(mu, M=64, C=320):
    g = torch.Generator().manual_seed(3100 + int(mu))
    x = (torch.randn((M, C), generator=g) + float(mu)).float()
    y64 = F.layer_norm(x.double(), (C,), eps=1e-5)
    y32 = F.layer_norm(x, (C,), eps=1e-5)
    return SimpleNamespace(M=M, C=C, x=x, y64=y64, e_torch=float((y32.double() - y64).abs().max()))


def assert_within(got, ref, tol, what):
    """|got - ref| <= tol for EVERY element; a failure names the worst one"""
    err = (got.detach().cpu().double() - ref).abs()
    over = err - tol
    if bool((over > 0).any()):
        i = int(over.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f"{what}: {int((over > 0).sum())} of {err.numel()} elements outside their bound; worst at {idx}: "
                             f"got {float(got.detach().cpu().double().flatten()[i])!r}, reference {float(ref.flatten()[i])!r}, "
                             f"error {float(err.flatten()[i]):.3e}, bound {float(tol.flatten()[i]):.3e}")
    return float((err / tol).max())
