"""Integer-lattice inputs and float64 references for the six entry points of libmadm_det.so (host-only torch code), shared
by tests/test_det_host.py (the exactness conditions, the negative controls) and tests/test_det_gpu.py (torch.equal).

Every reference is  out[col] = sum_r weight[r] * term[r][col]  over the rows r of a reduction, ``weight`` all ones for the
real thing: a reference with one row dropped, one row counted twice or one slice left out is the same statement with
another weight vector, which is how the host test builds its negative controls.  On the lattice every term is a small
integer and the sum of the terms' magnitudes stays below 2^24, so every f32 partial sum a kernel can form -- in any order --
is exact and the output has ONE correct bit pattern.

GroupNorm: the kernel uses whatever statistics it is handed; sum x = 0 and sum x^2 = count with eps = 0 make mean = 0 and
rstd = 1 (count * (1 / count) rounds to 1.0f whatever the f64 product's last bit), so xh = x and, with act = none, dz = dy.
LayerNorm: rows of +-1 in equal numbers have mean 0 and variance 1; C * fl(1 / C) must be exactly 1.0f for rstd to be
exactly 1 (``ln_width_is_exact``)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT3, ID3 = [F32, BF16, F16], ["f32", "bf16", "f16"]
DTYPE_CODE = {F32: 0, BF16: 1, F16: 2}
ACC_MAX = float(1 << 24)
MIN_SLICE_ROWS, MAX_SLICES, DW_MAX_SLICES = 16, 1024, 256


def epc(dtype):
    return 4 if dtype == F32 else 8


def slices_for(rows, cap):
    """The library's slice count, restated (test_det_host.py holds the two together)."""
    s = min(-(-rows // MIN_SLICE_ROWS), cap)
    per = -(-rows // s)
    return -(-rows // per), per


def image_slices(B, rows):
    return slices_for(rows, 1 if B >= MAX_SLICES else MAX_SLICES // B)


# name, B, rows per image, column chunks, slices the case is meant to have
ROW_CASES = [("one_slice_one_chunk", 1, 9, 1, 1),
             ("ragged3_b3", 3, 37, 5, 3),          # 13 + 13 + 11 rows; 51 row lanes of 5 chunks, one thread idle
             ("past_two_slices_two_column_trips", 1, 33, 257, 3),
             ("many_slices_b3", 3, 600, 3, 38)]    # the fold's eight-at-a-time loop and its tail
# name, B, H, W, dilation, column chunks, slices
DW_CASES = [("13x13_d1", 2, 13, 13, 1, 1, 22), ("13x13_d6", 1, 13, 13, 6, 5, 11), ("13x13_d18", 2, 13, 13, 18, 1, 22),
            ("20x20_d1", 1, 20, 20, 1, 5, 25), ("20x20_d6_two_column_trips", 1, 20, 20, 6, 257, 25),
            ("20x20_d18", 3, 20, 20, 18, 1, 75), ("20x20_d12", 2, 20, 20, 12, 5, 50)]
FAMILIES = ["colsum", "groupnorm_stats", "groupnorm_bwd_sums", "layernorm_bwd_params", "dwconv3x3_wgrad"]


def ints(shape, seed, amp):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).double()


def ln_width_is_exact(C):
    c = np.float32(C)
    return bool(np.float32(c * (np.float32(1) / c)) == np.float32(1))


def gn_layout(C, two_source):
    """(c_off, Ctot, C1, G) of a GroupNorm window of C channels: alone, or the second source behind C1 = 2 C channels"""
    if not two_source:
        return 0, C, C, (4 if C % 4 == 0 and C > 4 else 2)
    return 2 * C, 3 * C, 2 * C, 3


@functools.lru_cache(maxsize=None)
def row_case(family, name, C, two_source=False):
    """Inputs (float64, integer-valued) and terms of one ROW_CASES row at width C for one of the row-reduction families.
    ``terms``: [NACC][B][rows][C]; the output is their sum over rows (see ``reduce``)."""
    _n, B, R, _chunks, _s = next(c for c in ROW_CASES if c[0] == name)
    seed = 100 * FAMILIES.index(family) + [c[0] for c in ROW_CASES].index(name)
    ns = SimpleNamespace(family=family, B=B, R=R, C=C)
    if family == "colsum":
        ns.x = ints((B * R, C), seed, 3)
        ns.terms = ns.x.view(1, B, R, C)
    elif family == "groupnorm_stats":
        ns.x = ints((B * R, C), seed, 3)
        ns.terms = torch.stack([ns.x, ns.x * ns.x]).view(2, B, R, C)
    elif family == "groupnorm_bwd_sums":
        ns.c_off, ns.Ctot, ns.C1, ns.G = gn_layout(C, two_source)
        ns.x = ints((B * R, C), seed, 3)
        ns.dy = ints((B * R, ns.Ctot), seed + 50, 3)
        cpg = ns.Ctot // ns.G
        assert ns.Ctot % ns.G == 0
        unit = torch.tensor([0.0, float(R)], dtype=torch.float64)          # per channel: sum 0, sum of squares = pixels
        ns.sums1 = unit.repeat(B, ns.C1, 1)
        ns.sums2 = unit.repeat(B, ns.Ctot - ns.C1, 1) if ns.C1 < ns.Ctot else None
        ns.count = R * cpg
        ns.gamma = ints((ns.Ctot,), seed + 51, 2)
        ns.beta = ints((ns.Ctot,), seed + 52, 2)
        d = ns.dy[:, ns.c_off:ns.c_off + C]
        ns.terms = torch.stack([d, d * ns.x]).view(2, B, R, C)
    elif family == "layernorm_bwd_params":
        M = R                                                               # one "image" of R rows, whatever the case's B
        ns.B = 1
        g = torch.Generator().manual_seed(seed)
        half = torch.cat([torch.ones(C // 2), -torch.ones(C - C // 2)]).double()
        ns.x = torch.stack([half[torch.randperm(C, generator=g)] for _ in range(M)])
        ns.dy = ints((M, C), seed + 50, 3)
        ns.terms = torch.stack([ns.dy * ns.x, ns.dy]).view(2, 1, M, C)    # dgamma, dbeta
    else:
        raise KeyError(family)
    return ns


@functools.lru_cache(maxsize=None)
def dw_case(name, C):
    _n, B, H, W, dil, _chunks, _s = next(c for c in DW_CASES if c[0] == name)
    return dw_geometry_case(B, H, W, dil, C, 900 + [c[0] for c in DW_CASES].index(name))


@functools.lru_cache(maxsize=None)
def dw_geometry_case(B, H, W, dil, C, seed):
    """x, dy (integers of magnitude <= 2, tokens [B*H*W, C]) and the term tensor of the depthwise weight gradient at any geometry"""
    ns = SimpleNamespace(family="dwconv3x3_wgrad", B=1, R=B * H * W, C=C, images=B, H=H, W=W, dil=dil)
    x = ints((B, C, H, W), seed, 2)
    dy = ints((B, C, H, W), seed + 50, 2)
    ns.x = x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()
    ns.dy = dy.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()
    # terms[t][0][p][c] = dy[p][c] * x[p + offset_t][c], zero where the tap falls outside
    xp = F.pad(x, (dil, dil, dil, dil))
    terms = []
    for r in range(3):
        for s in range(3):
            sh = xp[:, :, r * dil:r * dil + H, s * dil:s * dil + W]
            terms.append((dy * sh).permute(0, 2, 3, 1).reshape(1, B * H * W, C))
    ns.terms = torch.stack(terms)
    # the same through autograd, as tests/test_train_gpu.py states the gradient
    wr = torch.zeros((C, 1, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wr, padding=dil, dilation=dil, groups=C).backward(dy)
    assert torch.equal(wr.grad.reshape(C, 9).t(), reduce(ns)[:, 0, :])
    return ns


def reduce(ns, weight=None):
    """[NACC][B][C] float64: the sum over rows of weight[r] * term, weight [B][rows] (None = ones)"""
    t = ns.terms
    if weight is not None:
        t = t * weight.view(1, ns.B, ns.R, 1)
    return t.sum(2)


def check_exact(ns):
    """Every term an integer, and the sum of magnitudes over a reduction below 2^24: any partial sum in any order is exact."""
    t = ns.terms
    assert t.dtype == torch.float64 and bool(torch.equal(t, t.round())) and bool(torch.isfinite(t).all())
    assert float(t.abs().sum(2).max()) < ACC_MAX / 4        # (room for the accumulate-into test's old values)
    for name in ("x", "dy"):
        v = getattr(ns, name, None)
        if v is not None:
            assert float(v.abs().max()) <= 256.0 and bool(torch.equal(v, v.round()))   # bf16 holds every integer up to 256
    return ns


def mutants(ns, slice_rows):
    """Weight vectors of the three negative controls: one row dropped, one row twice, the second slice left out."""
    one = torch.ones((ns.B, ns.R), dtype=torch.float64)
    r = ns.R // 2
    drop, twice, noslice = one.clone(), one.clone(), one.clone()
    drop[ns.B - 1, r] = 0.0
    twice[0, r] = 2.0
    lo = min(slice_rows, ns.R - 1)
    noslice[0, lo:min(lo + slice_rows, ns.R)] = 0.0
    return {"row dropped": drop, "row twice": twice, "slice left out": noslice}


def expected_f32(old_f32, sum_f64):
    """old + sum with one rounding, as the fold kernels update f32 outputs"""
    return (old_f32.double() + sum_f64).float()
