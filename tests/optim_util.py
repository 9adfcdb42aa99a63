"""Data, float64 references, per-element bounds, mutants and row tables for the flat optimizer, EMA, sum-of-squares and snapshot
kernels (madm_amd/csrc/optim.hip).  No GPU work here: test_optim_exact_host.py proves these utilities on the CPU
(every exact row really is exact in stepwise float32, every bound holds for a stepwise-float32 emulation, every mutant differs on
the rows it applies to); test_optim_exact_gpu.py holds the kernels to them.

One formula, three uses.  ``adamw_formula`` is the single-tensor step of torch.optim.AdamW written with operators only, so the
same text runs in float64 (the reference), in float32 tensors on the CPU (one IEEE rounding per operation, no contraction: the
emulation) and on the device in float64 (the 67 M-element row).  The kernel's scalar arguments enter as the float32 values the
launcher passes: lr, betas, eps, weight decay and the gradient scale as given, bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t)
computed in double and rounded once.

Assumptions, stated once: ``sqrtf`` and ``/`` of the device are correctly rounded (hipcc's default for HIP, no fast-math flag in
the Makefile), float32 subnormals are kept, and the compiler may contract a product and a sum into an FMA anywhere -- the exact
rows do not care (every intermediate is representable), the bounds count the uncontracted form (an FMA only removes a rounding)."""
import functools
import math

import numpy as np
import torch

U32 = 2.0 ** -24                # unit roundoff of float32
SUB = 2.0 ** -150               # half the spacing of float32 subnormals: the absolute error of an operation that underflows
SECOND = 1.0 + 2.0 ** -20       # second-order terms: (1 + u)^k - 1 - k u < 2^-20 k u for the k <= 70 counted anywhere below

# launch geometry the rows name (optim.hip: grid_for, sumsq_kernel, madm_adamw_step_table)
BLOCKS, THREADS, FLUSH = 2048, 256, 64
TRIP = BLOCKS * THREADS * 4     # 2^21 elements: one trip of the grid-stride loop of every flat kernel
TABLE_GRID, CHUNK = 65536, 1024
FLAT_SIZES = [1, 3, 4, 5, 1027, TRIP, TRIP + 3075, 3 * TRIP + 7]
HKEYS = ("lr", "wd", "b1", "b2", "eps", "bc1", "bc2s", "gs")


def f32(x):
    return float(np.float32(x))


def rnd32(t):
    return t.float().double()


def hyper(h, dtype, device="cpu"):
    """the scalars (or per-row columns) of ``h`` as tensors of ``dtype``: an operation between two of them stays in ``dtype``"""
    out = {k: torch.as_tensor(h[k], dtype=torch.float64).to(dtype=dtype, device=device) for k in HKEYS}
    out["one"] = torch.ones((), dtype=dtype, device=device)
    return out


def bias_corrections(b1, b2, step):
    """(bc1, bc2_sqrt) as madm_adamw_step and TableAdamW.step round them: double arithmetic on the float32 betas, one rounding"""
    return f32(1.0 - f32(b1) ** step), f32(math.sqrt(1.0 - f32(b2) ** step))


# ---- 1. AdamW: the formula, its mutants, its bound ---------------------------------------------------------------------------------
ADAMW_MUTANTS = ("eps_inside", "l2", "decay_after", "bc2_plain", "gscale_m_only", "gscale_once_in_v")


def adamw_formula(p, g, m, v, h, mutant=None, trace=None):
    """One AdamW step on tensors of the dtype of ``h`` (``hyper``): returns (p, m, v).  ``trace``: a dict that receives every
    intermediate.  The order of operations is adamw1's (optim.hip); torch.optim.AdamW's ``lerp`` and ``addcmul`` are the same
    real-number function, which test_optim_exact_host checks against torch itself in float64."""
    lr, wd, b1, b2, eps, bc1, bc2s, gs = (h[k] for k in HKEYS)
    one = h["one"]
    t = {}
    t["g1"] = g1 = g * gs                                   # the unscale and the clip coefficient
    if mutant == "l2":
        t["g1"] = g1 = g1 + wd * p
    t["lrwd"] = lrwd = lr * wd
    t["c"] = c = one - lrwd
    t["p1"] = p1 = p if mutant in ("l2", "decay_after") else p * c
    t["ob1"] = ob1 = one - b1
    t["ob2"] = ob2 = one - b2
    t["mA"] = mA = b1 * m
    t["mB"] = mB = ob1 * g1
    t["m1"] = m1 = mA + mB
    gv = g if mutant == "gscale_m_only" else g1
    t["vt"] = vt = ob2 * gv
    t["vB"] = vB = vt * (g if mutant in ("gscale_m_only", "gscale_once_in_v") else g1)
    t["vA"] = vA = b2 * v
    t["v1"] = v1 = vA + vB
    t["sq"] = sq = torch.sqrt(v1)
    if mutant == "eps_inside":
        t["den"] = den = (sq + eps) / bc2s
    else:
        t["r"] = r = sq / (bc2s * bc2s if mutant == "bc2_plain" else bc2s)
        t["den"] = den = r + eps
    t["a"] = a = lr / bc1
    t["q"] = q = m1 / den
    t["U"] = U = a * q
    t["p2"] = p2 = (p1 - U) * c if mutant == "decay_after" else p1 - U
    if trace is not None:
        trace.update(t)
    return p2, m1, v1


def adamw_ref(p, g, m, v, h, mutant=None, trace=None, device="cpu"):
    """float64 reference on float32 (or float64) inputs"""
    return adamw_formula(p.double(), g.double(), m.double(), v.double(), hyper(h, torch.float64, device), mutant, trace)


def adamw_emulate(p, g, m, v, h, trace=None):
    """stepwise float32 on the CPU: one rounding per operation, nothing contracted"""
    assert p.dtype == torch.float32 and not p.is_cuda
    return adamw_formula(p, g.float(), m.float(), v.float(), hyper(h, torch.float32), None, trace)


def adamw_emulate_fma(p, g, m, v, h):
    """the contraction hipcc emits for adamw1 (products feeding a sum fused: c, m, v and the final p), each FMA as a float64
    expression of float32 operands rounded once (the products are exact in float64; 53 >= 2 * 24 + 2 keeps the double rounding
    of the sum innocuous).  Used to show that the bounds cover the fused form too."""
    H = hyper(h, torch.float32)
    lr, wd, b1, b2, eps, bc1, bc2s, gs = (H[k].double() for k in HKEYS)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    g1 = rnd32(g * gs)
    c = rnd32(1.0 - lr * wd)
    ob1, ob2 = rnd32(1.0 - b1), rnd32(1.0 - b2)
    m1 = rnd32(b1 * m + rnd32(ob1 * g1))
    v1 = rnd32(b2 * v + rnd32(rnd32(ob2 * g1) * g1))
    den = rnd32(rnd32(torch.sqrt(v1).float().double() / bc2s) + eps)
    U = rnd32(rnd32(lr / bc1) * rnd32(m1 / den))
    return rnd32(c * p - U).float(), m1.float(), v1.float()


def adamw_bounds(p, g, m, v, h, device="cpu"):
    """(p, m, v) of the float64 reference and a tolerance per element for each, by a running first-order error analysis that
    counts every float32 rounding of adamw1 next to the operation it belongs to (u = 2^-24 of the operation's result, SUB where
    a product or a quotient may underflow), times SECOND:

        g1 = g gs                      1            m: b1 m (1), 1 - b1 (1), (1 - b1) g1 (1), g1 itself (1), the sum (1)  = 5
        v: b2 v (1), 1 - b2 (1), (1 - b2) g1 (1), (..) g1 (1), g1 twice (2), the sum (1)                                  = 7
        denom: v's error through the root (halved), the root (1), / bc2_sqrt (1), + eps (1)
        update: m's and denom's errors, the quotient (1), lr / bc1 (1), their product (1)
                -- without cancellation in m and with eps small, 5 + 7/2 + 3 + 3 = 14.5 roundings of |update|
        p: lr wd (1, of |p| lr wd), 1 - lr wd (1), p (1 - lr wd) (1), the difference (1, of |p'|): 4 roundings of |p|,
           plus the update's error.
    """
    tr = {}
    P, M, V = adamw_ref(p, g, m, v, h, trace=tr, device=device)
    H = hyper(h, torch.float64, device)
    a = lambda x: x.abs()                                                               # noqa: E731
    dg = U32 * a(tr["g1"]) + SUB
    dmB = 2 * U32 * a(tr["mB"]) + a(tr["ob1"]) * dg + SUB
    dm = U32 * a(tr["mA"]) + SUB + dmB + U32 * a(M)
    dvt = 2 * U32 * a(tr["vt"]) + a(tr["ob2"]) * dg + SUB
    dvB = a(tr["vt"]) * dg + a(tr["g1"]) * dvt + U32 * a(tr["vB"]) + SUB
    dv = U32 * a(tr["vA"]) + SUB + dvB + U32 * a(V)
    sq = tr["sq"]
    lo = torch.sqrt((V - SECOND * dv).clamp_min(0.0))
    dsq = torch.minimum(torch.sqrt(SECOND * dv), SECOND * dv / (sq + lo).clamp_min(1e-300)) + U32 * sq
    dr = dsq / H["bc2s"] + U32 * tr["r"] + SUB
    dden = dr + U32 * tr["den"]
    den_lo = tr["den"] - SECOND * dden
    assert bool((den_lo > 0).all())
    dq = (SECOND * dm + a(tr["q"]) * SECOND * dden) / den_lo + U32 * a(tr["q"]) + SUB
    dU = a(tr["a"]) * dq + 2 * U32 * a(tr["U"]) + SUB
    dp1 = U32 * a(p.double()) * (a(tr["c"]) + a(tr["lrwd"])) + U32 * a(tr["p1"]) + SUB
    dp = dp1 + dU + U32 * a(P)
    return (P, M, V), (SECOND * dp, SECOND * dm, SECOND * dv)


# ---- 2. exact AdamW data: index-based, so a row of any size is generated in pieces on any device -------------------------------------
EX = dict(b1=0.5, b2=0.75, lr=2.0 ** -6, wd=2.0 ** -3, eps=2.0 ** -4, gs=2.0 ** -7)
EX_LR = (2.0 ** -6, 2.0 ** -5, 2.0 ** -7)          # per-tensor values of the table rows
EX_WD = (2.0 ** -3, 0.0, 2.0 ** -2)
_MULT = (0.0, 1.0, 3.0, 7.0, 15.0, -1.0, -3.0, -7.0, -15.0)       # unscaled gradient / eps: 0 and +-(2^k - 1), k = 1..4


def exact_hyper(row, **over):
    """row 'a': step 1 from zero moments (bc1 = bc2_sqrt = 1/2 exactly); row 'b': both bias corrections exactly 1"""
    bc = 0.5 if row == "a" else 1.0
    return dict(EX, bc1=bc, bc2s=bc, **over)


def exact_elems(lo, hi, row, device="cpu"):
    """(p, g, m, v) float32 for element indices [lo, hi).  p: multiples of 2^-4, |p| <= 8.  g: the unscaled gradient
    {0, +-(2^k - 1) eps} times the loss scale 2^7.  Row 'a': zero moments.  Row 'b': m0 a multiple of 2^-4, |m0| <= 4, and
    v0 = (unscaled g)^2, so v stays g^2 and the root is exact."""
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    mult = torch.tensor(_MULT, dtype=torch.float64, device=device)[(i * 7 + 3) % 9]
    gu = mult * EX["eps"]
    g = gu / EX["gs"]
    p = (((i * 13 + 5) % 257) - 128).double() / 16.0
    if row == "a":
        m = torch.zeros_like(p)
        v = torch.zeros_like(p)
    else:
        m = (((i * 11 + 1) % 129) - 64).double() / 16.0
        v = gu * gu
    return p.float(), g.float(), m.float(), v.float()


class TableCase:
    """A flat table layout: ``chunks[t]`` chunks of 1024 for tensor t, ``numel[t]`` live elements (the rest of its last chunk is
    padding: p = g = m = v = 0), one hyper row {lr, wd, bc1, bc2_sqrt} per tensor, bc1 = 0 for a skipped tensor."""

    def __init__(self, chunks, numel, skipped, row):
        self.chunks, self.numel, self.skipped, self.row = list(chunks), list(numel), set(skipped), row
        self.T = len(self.chunks)
        self.start = np.concatenate([[0], np.cumsum(self.chunks)])[:-1].astype(np.int64)        # first chunk of each tensor
        self.nchunks = int(sum(self.chunks))
        self.n = self.nchunks * CHUNK
        bc = 0.5 if row == "a" else 1.0
        self.hyper = np.zeros((self.T, 4), dtype=np.float32)
        for t in range(self.T):
            self.hyper[t] = (EX_LR[t % 3], EX_WD[(t // 2) % 3], 0.0 if t in self.skipped else bc, bc)

    def chunk_tensor(self, lo=0, hi=None, device="cpu"):
        hi = self.nchunks if hi is None else hi
        bounds = torch.as_tensor(self.start[1:], device=device)
        return torch.bucketize(torch.arange(lo, hi, device=device), bounds, right=True).to(torch.int32)

    def live(self, lo, hi, device="cpu"):
        """mask over chunks [lo, hi) x 1024: False on the padding tail of a tensor"""
        ct = self.chunk_tensor(lo, hi, device).long()
        start = torch.as_tensor(self.start, device=device)[ct]
        numel = torch.as_tensor(self.numel, device=device)[ct]
        c = torch.arange(lo, hi, device=device)
        e = (c - start).view(-1, 1) * CHUNK + torch.arange(CHUNK, device=device).view(1, -1)
        return e < numel.view(-1, 1)

    def elems(self, lo, hi, device="cpu", nan_in_skipped=False):
        """(p, g, m, v) float32 [hi - lo, 1024] for chunks [lo, hi)"""
        p, g, m, v = (x.view(-1, CHUNK) for x in exact_elems(lo * CHUNK, hi * CHUNK, self.row, device))
        live = self.live(lo, hi, device)
        p, g, m, v = (torch.where(live, x, torch.zeros_like(x)) for x in (p, g, m, v))
        if nan_in_skipped:
            sk = torch.as_tensor(sorted(self.skipped), device=device)
            is_sk = (self.chunk_tensor(lo, hi, device).long().view(-1, 1) == sk.view(1, -1)).any(1)
            g = torch.where(is_sk.view(-1, 1) & live, torch.full_like(g, float("nan")), g)
        return p, g, m, v

    def hyper_rows(self, lo, hi, device="cpu", shift=0):
        """per-chunk hyper columns [hi - lo, 1] for the formula; ``shift``: the row of chunk c - shift (a mutant)"""
        ct = self.chunk_tensor(lo - shift, hi - shift, device).long()
        hy = torch.as_tensor(self.hyper, device=device).double()[ct]
        h = dict(EX, lr=hy[:, 0:1], wd=hy[:, 1:2], bc1=hy[:, 2:3], bc2s=hy[:, 3:4])
        return h, (hy[:, 2:3] == 0)

    def reference(self, lo, hi, device="cpu", mutant=None, nan_in_skipped=False, trace=None):
        """float64 (p, m, v) for chunks [lo, hi).  Mutants: an ADAMW_MUTANTS name, 'skipped_decayed', 'skipped_moments',
        'second_trip_untouched', 'second_trip_hyper' (chunks from TABLE_GRID on use the row of chunk c - TABLE_GRID)."""
        p, g, m, v = self.elems(lo, hi, device, nan_in_skipped)
        shift = TABLE_GRID if mutant == "second_trip_hyper" and lo >= TABLE_GRID else 0
        h, skip = self.hyper_rows(lo, hi, device, shift)
        hs = dict(h, bc1=torch.where(skip, torch.ones_like(h["bc1"]), h["bc1"]))          # (no division by 0 in the skipped rows)
        fm = mutant if mutant in ADAMW_MUTANTS else None
        gz = torch.where(skip, torch.zeros_like(g), g)                                    # a skipped tensor's gradient is not read
        P, M, V = adamw_formula(p.double(), gz.double(), m.double(), v.double(), hyper(hs, torch.float64, device), fm, trace)
        keepP, keepM = skip, skip
        if mutant == "skipped_decayed":
            P = torch.where(skip, p.double() * (1.0 - h["lr"] * h["wd"]), P)
            keepP = torch.zeros_like(skip)
        if mutant == "skipped_moments":
            keepM = torch.zeros_like(skip)
        P = torch.where(keepP, p.double(), P)
        M, V = torch.where(keepM, m.double(), M), torch.where(keepM, v.double(), V)
        if mutant == "second_trip_untouched" and hi > TABLE_GRID:
            late = (torch.arange(lo, hi, device=device) >= TABLE_GRID).view(-1, 1)
            P, M, V = torch.where(late, p.double(), P), torch.where(late, m.double(), M), torch.where(late, v.double(), V)
        return P, M, V


# tensors of 1, 2 and 5 chunks; a skipped tensor first, in the middle and last; live sizes that end 1, 3 and 1000 short of a
# chunk, on it, and one element into it
_SM_CHUNKS = (1, 2, 5, 1, 2, 5, 1, 2, 1)
_SM_NUMEL = (1023, 2048, 5 * 1024 - 3, 24, 1025, 4 * 1024 + 1, 1024, 2 * 1024 - 1000, 7)
TABLE_SMALL = {row: TableCase(_SM_CHUNKS, _SM_NUMEL, (0, 4, 8), row) for row in ("a", "b")}
# 65 536 + 3 chunks: chunks 65 536 .. 65 538 are the second trip of the chunk loop and are three tensors of their own, the middle
# one skipped; chunks 0 .. 2 (what c - 65 536 names) belong to tensor 0, whose hyper row differs from all three
TABLE_BIG = TableCase((30000, TABLE_GRID - 30000, 1, 1, 1), (30000 * 1024 - 5, (TABLE_GRID - 30000) * 1024, 1021, 1024, 3), (3,), "b")
TABLE_MUTANTS = ("skipped_decayed", "skipped_moments")
TABLE_BIG_MUTANTS = ("second_trip_untouched", "second_trip_hyper")


def untouched_from(out, orig, start):
    """coverage mutant: elements from ``start`` on keep their old value (``start`` = n // 4 * 4: the tail; TRIP: the second trip)"""
    o = out.clone()
    o[start:] = orig[start:].to(o.dtype)
    return o


# ---- 3. layer-2 AdamW data -----------------------------------------------------------------------------------------------------------
L2_STEPS = (1, 2, 10, 1000, 20000, 10 ** 6)
L2_CLIP = 0.37                                  # the clip coefficient min(1, clip / norm) of a step whose norm exceeds the limit
L2_LRWD = ((1e-3, 0.05), (1e-4, 0.01))          # what the suite constructs MadmTrainer with
# (n, step, loss scale, lr / wd pair)
L2_ROWS = [(1027, s, sc, k % 2) for k, (s, sc) in enumerate((s, sc) for s in L2_STEPS for sc in (65536.0, 128.0))] + \
          [(TRIP + 3075, 1, 65536.0, 0), (TRIP + 3075, 1000, 128.0, 1), (TRIP + 3075, 10 ** 6, 65536.0, 0)]


def l2_id(row):
    return f"n{row[0]}_t{row[1]}_s{int(row[2])}_lr{row[3]}"


def l2_hyper(step, scale, which):
    lr, wd = L2_LRWD[which]
    bc1, bc2s = bias_corrections(0.9, 0.999, step)
    return dict(lr=f32(lr), wd=f32(wd), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), bc1=bc1, bc2s=bc2s, gs=f32(L2_CLIP / scale))


@functools.lru_cache(maxsize=4)
def l2_case(row):
    """(p, g, m, v) float32 and the hyper dict.  Unscaled |g| log-uniform over 1e-24 .. 1e2 with one zero in 16, stored times the
    loss scale; m of the size of the clipped gradient with either sign, v of the size of its square (1e-48 .. 1e4: float32
    normals, subnormals and zeros); p ~ N(0, 0.1) with zeros."""
    n, step, scale, which = row
    gen = torch.Generator().manual_seed(1000 + n % 997 + step % 991 + int(scale))
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)                        # noqa: E731
    mag = 10.0 ** (-24.0 + 26.0 * r())
    sign = torch.where(r() < 0.5, -1.0, 1.0)
    gu = torch.where(r() < 1.0 / 16, torch.zeros_like(mag), mag * sign)
    g = (gu * scale).float()
    gc = gu * L2_CLIP
    m = (gc.abs() * (2.0 * r() - 1.0) + torch.where(r() < 0.25, 10.0 ** (-24.0 + 26.0 * r()), torch.zeros_like(mag))).float()
    v = (gc * gc * (0.5 + r()) + torch.where(r() < 0.25, (10.0 ** (-24.0 + 26.0 * r())) ** 2, torch.zeros_like(mag))).float()
    if step == 1:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    p = (0.1 * torch.randn(n, generator=gen, dtype=torch.float64) * (r() > 1.0 / 16)).float()
    return (p, g, m, v), l2_hyper(step, scale, which)


def worst_ratio(got, want, tol):
    """max |got - want| / tol over all elements (0 / 0 counts as 0); a non-finite value anywhere gives inf"""
    d = (got.double() - want).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    return float(torch.where(d == 0, torch.zeros_like(d), d / tol).max())


# ---- 4. EMA --------------------------------------------------------------------------------------------------------------------------
EMA_EXACT_ALPHAS = (0.0, 0.5, 0.75)
EMA_L2_ALPHAS = (0.5, 2.0 / 3.0, 0.99, 0.999)
EMA_MUTANTS = ("swapped", "zero_is_skip")


def ema_ref(e, q, alpha, mutant=None):
    """The function ema_kernel computes, in float64: a = alpha rounded to float32, b = 1 - a (exact in float32 for a >= 1/2 and
    for a = 0), e' = a e + b q.  a + b is exactly 1: a teacher equal to its student stays equal."""
    a = f32(alpha)
    b = 1.0 - a
    if mutant == "swapped":
        a, b = b, a
    if mutant == "zero_is_skip" and a == 0.0:
        return e.double()
    return a * e.double() + b * q.double()


def ema_bounds(e, q, alpha):
    """a e (1), 1 - a (1, counted though exact for the rows), b q (1), the sum (1)"""
    a = f32(alpha)
    want = ema_ref(e, q, alpha)
    tol = SECOND * U32 * (abs(a) * e.double().abs() + 2 * abs(1.0 - a) * q.double().abs() + want.abs()) + 2 * SUB
    return want, tol


def ema_emulate(e, q, alpha, fused=True):
    """float32 stepwise; ``fused``: fma(a, e, fl(b q)), the form the kernel spells out (one rounding of a e + fl(b q))"""
    a = torch.tensor(alpha, dtype=torch.float32)
    b = torch.ones((), dtype=torch.float32) - a
    bq = b * q
    if not fused:
        return a * e + bq
    return rnd32(a.double() * e.double() + bq.double()).float()


def ema_exact_data(n, seed=0):
    """dyadic teacher and student: multiples of 2^-6 with |x| <= 32, so a e + b q is exact for a in {0, 1/2, 3/4}"""
    i = torch.arange(n, dtype=torch.int64)
    e = (((i * 29 + 7 + seed) % 4097) - 2048).double() / 64.0
    q = (((i * 31 + 11 + seed) % 4093) - 2046).double() / 64.0
    return e.float(), q.float()


def ema_random_data(n, seed=0):
    gen = torch.Generator().manual_seed(77 + seed)
    e = torch.randn(n, generator=gen) * (10.0 ** (-6 + 8 * torch.rand(n, generator=gen)))
    q = torch.randn(n, generator=gen) * (10.0 ** (-6 + 8 * torch.rand(n, generator=gen)))
    return e, q


# ---- 5. sum of squares ---------------------------------------------------------------------------------------------------------------
def sumsq_int_data(n, seed=0):
    """integers |x| <= 2^7: a thread's float32 partial holds at most 256 squares <= 2^14 (below 2^24), the rest is float64:
    the integer sum in any order.  x[0] is odd and every other element even, so the sum is odd: beyond 2^24 a float32
    final sum cannot hold it."""
    i = torch.arange(n, dtype=torch.int64)
    x = 2 * ((((i * 37 + 5 + seed) % 129) - 64))
    x[0] = 127
    return x.float()


def sumsq_emulate(x, blocks=BLOCKS, threads=THREADS, flush=FLUSH, tail=True, final_f32=False):
    """sumsq_kernel on the host for a launch of ``blocks`` x ``threads`` (the grid is NOT capped here: pass the capped value):
    per float4 s = y y, then fma(x, x, s), fma(z, z, s), fma(w, w, s) as hipcc contracts it, acc += s in float32, handed to
    float64 every ``flush`` trips (None: never); the n % 4 tail in float64 by one thread.  Returns a python float."""
    x = x.float()
    n = x.numel()
    n4 = n // 4
    T = blocks * threads
    trips = (n4 + T - 1) // T
    q = torch.zeros(trips * T * 4, dtype=torch.float64)
    q[:n4 * 4] = x[:n4 * 4].double()
    q = q.view(trips, T, 4)
    acc = torch.zeros(T, dtype=torch.float64)
    dacc = torch.zeros(T, dtype=torch.float64)
    for k in range(trips):
        s = rnd32(q[k, :, 1] * q[k, :, 1])
        for j in (0, 2, 3):
            s = rnd32(s + q[k, :, j] * q[k, :, j])
        acc = rnd32(acc + s)
        if flush is not None and (k + 1) % flush == 0:
            dacc, acc = dacc + acc, torch.zeros_like(acc)
    total = float((dacc + acc).sum())
    if tail:
        total += float((x[n4 * 4:].double() ** 2).sum())
    return f32(total) if final_f32 else total


def sumsq_grid(n, blocks=BLOCKS, threads=THREADS):
    return max(1, min(blocks, (n // 4 + threads - 1) // threads))


def sumsq_bounds(x, flush=FLUSH):
    """A thread's partial is a sum of non-negative terms: 4 roundings inside a float4 (a product, three FMAs) and at most
    ``flush`` float32 additions, so (flush + 4) u relative, whatever the order; every square may underflow (SUB each); float64
    beyond (2^-53 per addition of a few thousand: nothing on this scale)."""
    want = float((x.double() ** 2).sum())
    return want, SECOND * (flush + 4) * U32 * want + x.numel() * SUB + 2.0 ** -40 * want


def flush_row_elems(lo, hi, device="cpu", blocks=BLOCKS, threads=THREADS, flush=FLUSH):
    """The flush row, elements [lo, hi) of n = (flush + 1) trip + 5, trip = blocks threads 4.  Below flush * trip every float4 is
    2^10 {1, 2, 3, 4} with signs: squares are multiples of 2^20, a thread's partial after ``flush`` trips is 30 flush 2^20
    (1920 * 2^20 > 2^30 at 64: exact in float32, spacing 128).  From flush * trip on every element is +-1: the float4's 4 is below
    half that spacing and is lost unless the partial went to float64 first.  This row names the kernel's present geometry."""
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    sign = (1 - 2 * ((i // 4 + i) % 2)).double()
    big = 1024.0 * (1 + i % 4).double() * sign
    return torch.where(i < flush * blocks * threads * 4, big, sign).float()


def flush_row_n(blocks=BLOCKS, threads=THREADS, flush=FLUSH):
    return (flush + 1) * blocks * threads * 4 + 5


def flush_row_sum(blocks=BLOCKS, threads=THREADS, flush=FLUSH):
    trip = blocks * threads * 4
    return flush * (trip // 4) * 30 * 2 ** 20 + trip + 5


def adversarial_sumsq(n, lanes=(0, 1, 255, 256, 2047 * 256 + 255), blocks=BLOCKS, threads=THREADS):
    """zeros, except that in the partials of the threads ``lanes`` the first float4 holds 4096 (square 2^24) and every later
    one four halves (sum 1: a tie at 2^24, rounded to even, that is lost each time)"""
    x = torch.zeros(n, dtype=torch.float32)
    T = blocks * threads
    for j in lanes:
        k = 0
        while (j + k * T) * 4 + 3 < n // 4 * 4:
            o = (j + k * T) * 4
            if k == 0:
                x[o] = 4096.0
            else:
                x[o:o + 4] = 0.5
            k += 1
    return x


# ---- 6. fingerprint ------------------------------------------------------------------------------------------------------------------
FP_MUTANTS = ("base_ignored", "off_by_one", "index_dropped")
_M64 = (1 << 64) - 1


def fingerprint_ref(values, index_base=0, mutant=None):
    """fp_mix of optim.hip summed modulo 2^64, restated.  Mutants: 'base_ignored', 'off_by_one' (index + 1), 'index_dropped' (the
    shift carried out in 32 bits: the index never reaches the hash) and 'index_low32' (the index cut to its low 32 bits before a
    64-bit shift) -- the last one is the same function wherever index_base + n <= 2^32, which the launcher enforces: it is kept
    to state that, not counted as a mutant."""
    w = np.ascontiguousarray(values.detach().cpu().numpy() if torch.is_tensor(values) else values, dtype=np.float32)
    w = w.reshape(-1).view(np.uint32).astype(np.uint64)
    idx = np.arange(w.size, dtype=np.uint64) + np.uint64(0 if mutant == "base_ignored" else index_base)
    if mutant == "off_by_one":
        idx = idx + np.uint64(1)
    if mutant == "index_low32":
        idx = idx & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        h = w if mutant == "index_dropped" else ((idx << np.uint64(32)) | w)
        h = h * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(32)
        h = h * np.uint64(0xD6E8FEB86659FD93)
        h ^= h >> np.uint64(32)
        return int(h.sum(dtype=np.uint64)) & _M64


def special_values(n, seed=0):
    """float32 bit patterns that a value-wise copy could damage: quiet and signalling NaNs with payloads, -0.0, subnormals, +-inf,
    among ordinary numbers"""
    gen = torch.Generator().manual_seed(5 + seed)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x7FC00001, 0x7F800001, -0x00400000 + 5, -2 ** 31, 1, 0x007FFFFF, -2 ** 31 + 1, 0x7F800000,
                            -0x00800000, 0x7FFFFFFF], dtype=torch.int64).to(torch.int32)
    k = min(n, special.numel())
    pos = torch.randperm(n, generator=gen)[:k]
    bits[pos] = special[:k]
    return bits.view(torch.float32)


# ---- 7. EmaPairs on production's layout -----------------------------------------------------------------------------------------------
# Sizes in the teacher's (registration) order: multiples of 1024, non-multiples, and 1021 .. 1023 mod 1024 (where the teacher's pad
# to 4 and the student's pad to 1024 coincide: 3, 2, 1 elements).  LATE: indices the student flat moves to its front, as
# MadmTrainer does with the tensors whose gradient finishes last.  OUTSIDE: the student of this pair is a tensor of its own.
PAIR_SIZES = (2048, 1021, 1022, 1023, 24, 2024, 24, 3000, 1024, 7, 4096, 1023 + 1024)
PAIR_LATE = (4, 9)
PAIR_OUTSIDE = 7


def expected_spans(sizes=PAIR_SIZES, late=PAIR_LATE, outside=PAIR_OUTSIDE):
    """The launches EmaPairs may make, counted from the layout alone: walking the pairs in the teacher's order, pair i + 1 joins
    pair i's span iff it follows it directly on BOTH sides with the same padding between them: both in the student flat's
    ordered part, neither late nor outside, and pad4(n_i) == pad1024(n_i)."""
    spans = 0
    prev_joinable = False
    for i, n in enumerate(sizes):
        here = i not in late and i != outside
        same_pad = i > 0 and (-sizes[i - 1]) % 4 == (-sizes[i - 1]) % 1024
        if not (here and prev_joinable and same_pad):
            spans += 1
        prev_joinable = here
    return spans


def build_pairs(device="cpu", sizes=PAIR_SIZES, late=PAIR_LATE, outside=PAIR_OUTSIDE):
    """(teacher FlatParams(align=4), TableAdamW over the students with the late ones first, EmaPairs, teachers, students)"""
    from madm_amd import optim
    gen = torch.Generator().manual_seed(4)
    mk = lambda n, s: torch.nn.Parameter((torch.randint(-64, 65, (n,), generator=gen).float() / 8 + s).to(device))    # noqa: E731
    teachers = [mk(n, 0.0) for n in sizes]
    students = [mk(n, 0.125) for n in sizes]
    order = [i for i in late] + [i for i in range(len(sizes)) if i not in late and i != outside]
    tflat = optim.FlatParams(teachers, with_grad=False, align=4)
    opt = optim.TableAdamW([(students[i], 1e-3, 0.0) for i in order])
    return tflat, opt, optim.EmaPairs(teachers, students), teachers, students


def covered(spans, side, flat, tensors):
    """elements of ``flat`` that the spans' ``side`` (0 teacher, 1 student) cover, as a bool mask, and whether every span that
    starts inside ``flat`` stays inside it"""
    base, n = flat.data_ptr(), flat.numel()
    mask = torch.zeros(n, dtype=torch.bool)
    for sp in spans:
        o = (sp[side] - base) // 4
        if 0 <= o < n:
            assert o + sp[2] // 4 <= n
            mask[o:o + sp[2] // 4] = True
    return mask


def owned(flat, tensors):
    mask = torch.zeros(flat.numel(), dtype=torch.bool)
    for t in tensors:
        o = (t.data_ptr() - flat.data_ptr()) // 4
        if 0 <= o < flat.numel():
            mask[o:o + t.numel()] = True
    return mask
