"""Selector inputs and exact references for the attention kernels (host-only torch code).

The inputs are built so that the true result of softmax(Q K^T) V and of its gradients is known without a tolerance:

* every element of q, k, v and dO is a number that bf16 and f16 represent exactly, and scale = 1;
* for each query i a chosen set S(i) of one key ("single" form) or of two keys in different KV tiles ("pair" form) has
  score exactly 0, and every other key scores at most -G with G >= 40 nats: P is 1 on one key or 1/2 and 1/2 on a pair,
  and everything else together carries less than 2^-40 of the weight;
* the rows of V are distinct vectors of nonzero even integers, so an output row names the batch, head and key(s) it came
  from, and the mean over a pair is an integer vector.

A key that a wrong tail mask admits is the zero row an out-of-bounds load returns: it scores 0 and ties with S(i), so the
whole output row is cut to 1/2 or 2/3 of its value instead of moving by 1e-3.

Construction (per batch b and head h; ``nb`` bias dims at the end of the head, ``Dc = D - nb`` code dims):
  k_j   = [code(j), 1 .. 1]            code(j)[m] = +-1 by bit ((m + shift(b, h)) mod nbits) of j
  q_i   = [c (code(a) + code(b)) / 2, beta .. beta],  beta = -(q_code . code(a)) / nb   (b = a in the single form)
so score(i, j) = -2 c (number of code dims of bits != t in which j differs from a), t the bit in which a and b differ.
c is 8, doubled until the gap G = 2 c floor(Dc / nbits) reaches 104 nats (code_scale: 16 or 32 at D = 40, 8 elsewhere), so that
every off-set probability is exactly 0 in f32 (2^-150 and below) and not only below 2^-40.  With c = 8 at D = 40 (G = 48 or 80)
the off-set probabilities are about 2^-69 .. 2^-115: f32 keeps them, and the 16-bit MFMA does not round to nearest when such a
term meets a partial sum in its accumulator -- the bf16 backward returned 1 ulp of f32 at the partial sum's magnitude where
the true gradient is 0 (measured: dq 4.8e-7, dk 6.1e-5, dv 6.0e-8; f16 flushes the terms and f32 uses the exact f32 MFMA).
That is the hardware's arithmetic, not a routing fault, so the inputs keep it out of the result instead of a tolerance.

The causal inputs (f32 only, D = 64) add a bait: for every query with a later key, key i + 1 or the first key of the next
16-key block scores exactly +40 -- if the causal mask leaks, that key takes the whole row.  The bait comes from 22
thermometer dims of K ([j >= 16 m], m = 1..7, and [j mod 16 >= n], n = 1..15) that a query weights so that every visible key
outside S(i) is only pushed further down; see build_causal.

Everything is cached, float64, on the CPU, and must be treated as read-only.
"""
import functools
from types import SimpleNamespace

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT3, ID3 = [F32, BF16, F16], ["f32", "bf16", "f16"]
C_CODE = 8.0
GAP_MIN = 40.0
GAP_ZERO = 104.0            # exp(-104) < 2^-150: below the smallest f32 denormal
W_MAX = 2.0 ** -40

# B, H, Lq, Lk, D -- the smallest shapes that reach each instantiation of attn_kernel (testing section)
FWD_CASES = [
    (2, 3, 70, 77, 40),      # 16-bit <2,3,4,4> (ones column), f32 <3,3,4,4>; two tiles, tail 13
    (2, 3, 70, 128, 40),     # full-tile branch only
    (2, 3, 70, 517, 40),     # 16-bit <2,3,4,8>: five 128-key tiles, tail 5
    (2, 3, 70, 512, 40),     # Lk dispatch edge, 128-key side
    (2, 3, 70, 511, 40),     # Lk dispatch edge, 64-key side
    (1, 2, 2065, 517, 40),   # <2,3,8,8,2>: last block has 17 rows; Q aliased on KV buffer 1
    (1, 1, 2047, 517, 40),   # other side of the Lq edge
    (2, 3, 70, 141, 64),     # <2,4,4,4> / <4,4,4,4>
    (2, 3, 70, 141, 80),     # <3,5,4,4> / <5,5,4,4>
    (2, 3, 70, 517, 80),     # <3,5,4,8>
    (2, 3, 33, 77, 160),     # <5,10,4,4> / <10,10,4,4>
    (2, 1, 37, 45, 512),     # <16,32,2,2> (unpipelined, 32-key tiles), <float,32,32,1,1>
    (2, 1, 21, 37, 512),
]
BWD_CASES = [(2, 3, 70, 77, 40), (2, 3, 70, 141, 64), (2, 3, 130, 141, 80), (2, 3, 33, 77, 160), (1, 2, 200, 517, 40)]
CAUSAL_L = [1, 2, 77, 128]
CAUSAL_B, CAUSAL_H, CAUSAL_D = 2, 12, 64
FORMS = ["single", "pair"]


def case_id(c):
    return f"B{c[0]}H{c[1]}q{c[2]}k{c[3]}d{c[4]}"


def key_tiles(Lk, D):
    """KV tile lengths of the kernels that serve (Lk, D): forward f32 / 16-bit, and the backward's 64."""
    if D == 512:
        return (16, 32)
    return (64, 128) if Lk >= 512 else (64,)


def n_bias(D):
    return 8 if D == 512 else 1


def _bits(L):
    return max(1, (L - 1).bit_length())


def code_scale(L, Dc):
    """c: 8, doubled (a power of two keeps c * Dc representable in bf16) until 2 c floor(Dc / nbits) >= GAP_ZERO."""
    c = C_CODE
    while 2 * c * (Dc // _bits(L)) < GAP_ZERO:
        c *= 2
    return c


def _code(B, H, L, Dc, nbits):
    """[B, H, L, Dc] of +-1: dim m of (b, h) carries bit (m + shift(b, h)) mod nbits of the key index."""
    j = torch.arange(L).view(1, 1, L, 1)
    m = torch.arange(Dc).view(1, 1, 1, Dc)
    shift = (3 * torch.arange(B).view(B, 1, 1, 1) + torch.arange(H).view(1, H, 1, 1)) % nbits
    return (((j >> ((m + shift) % nbits)) & 1) * 2 - 1).double()


def _values(shape, g):
    """Nonzero even integers in [-6, 6]."""
    vals = torch.tensor([-6.0, -4.0, -2.0, 2.0, 4.0, 6.0], dtype=torch.float64)
    return vals[torch.randint(0, 6, tuple(shape), generator=g)]


def _dout(B, L, H, D, g):
    """At most four entries of +-1 per (b, i, h) row."""
    pos = torch.rand((B, L, H, D), generator=g).argsort(-1)[..., :4]
    sign = (torch.randint(0, 2, (B, L, H, 4), generator=g) * 2 - 1).double()
    return torch.zeros((B, L, H, D), dtype=torch.float64).scatter_(-1, pos, sign)


def _gather_rows(x, idx):
    """x [B, H, L, C], idx [B, H, Lq] -> [B, H, Lq, C]."""
    return torch.gather(x, 2, idx.unsqueeze(-1).expand(-1, -1, -1, x.shape[-1]))


def forced_selections(Lq, Lk, D):
    """(query row, key) pairs every (b, h) carries: key 0, the first key of the last tile and the last key of the first
    tile for every tile length in use, and key Lk - 1 on the last query row (the last row of the last block)."""
    out = [(0, 0)]
    for tz in key_tiles(Lk, D):
        out.append((len(out), (Lk - 1) // tz * tz))
        out.append((len(out), min(tz, Lk) - 1))
    out.append((Lq - 1, Lk - 1))
    assert len(out) <= Lq
    return out


@functools.lru_cache(maxsize=None)
def build(B, H, Lq, Lk, D, form, seed=0):
    """Selector inputs of one case: q, k, v, dout as float64 [B, L, H, D]; a, b as int64 [B, H, Lq] (b == a: one key)."""
    assert form in FORMS
    g = torch.Generator().manual_seed(1000 * seed + 7 * Lq + 13 * Lk + D + (1 if form == "pair" else 0))
    nb, nbits = n_bias(D), _bits(Lk)
    Dc = D - nb
    kc = _code(B, H, Lk, Dc, nbits)
    # partner of key j: j with the highest bit flipped that keeps it inside Lk and moves it to another tile of every length
    tmin = max(key_tiles(Lk, D)).bit_length() - 1
    keys = torch.arange(Lk)
    partner = keys.clone()
    for t in range(tmin, nbits):      # ascending: the highest valid bit wins
        cand = keys ^ (1 << t)
        partner = torch.where(cand < Lk, cand, partner)
    a = torch.randint(0, Lk, (B, H, Lq), generator=g)
    if form == "pair":
        has = torch.nonzero(partner != keys).flatten()
        if has.numel():
            alt = has[torch.randint(0, has.numel(), (B, H, Lq), generator=g)]
            a = torch.where(torch.rand((B, H, Lq), generator=g) < 0.75, alt, a)
    for row, key in forced_selections(Lq, Lk, D):
        a[:, :, row] = key
    b = partner[a] if form == "pair" else a.clone()
    ka, kb = _gather_rows(kc, a), _gather_rows(kc, b)
    qc = code_scale(Lk, Dc) * (ka + kb) / 2
    beta = -(qc * ka).sum(-1, keepdim=True) / nb
    q = torch.cat([qc, beta.expand(-1, -1, -1, nb)], -1).transpose(1, 2).contiguous()
    k = torch.cat([kc, torch.ones((B, H, Lk, nb), dtype=torch.float64)], -1).transpose(1, 2).contiguous()
    v = _values((B, Lk, H, D), g)
    dout = _dout(B, Lq, H, D, g)
    return SimpleNamespace(B=B, H=H, Lq=Lq, Lk=Lk, D=D, form=form, q=q, k=k, v=v, dout=dout, a=a, b=b, causal=False)


def selection_matrix(d):
    """The exact P: [B, H, Lq, Lk], 1 on a single selected key, 1/2 and 1/2 on a pair."""
    P = torch.zeros((d.B, d.H, d.Lq, d.Lk), dtype=torch.float64)
    P.scatter_add_(3, d.a.unsqueeze(-1), torch.full(d.a.shape + (1,), 0.5, dtype=torch.float64))
    P.scatter_add_(3, d.b.unsqueeze(-1), torch.full(d.b.shape + (1,), 0.5, dtype=torch.float64))
    return P


def closed_form(d):
    """Exact O, dQ, dK, dV (float64 [B, L, H, D]) and dS, dP - D for the selection matrix: O = mean of V over S(i),
    dV = P^T dO, dS = P o (dP - rowsum(dO o O)), dQ = dS K, dK = dS^T Q (scale = 1)."""
    P = selection_matrix(d)
    qh, kh, vh, gh = (t.transpose(1, 2) for t in (d.q, d.k, d.v, d.dout))      # [B, H, L, D]
    O = P @ vh
    dP = gh @ vh.transpose(2, 3)
    Dsum = (gh * O).sum(-1, keepdim=True)
    dS = P * (dP - Dsum)
    out = SimpleNamespace(P=P, dS=dS, dPmD=(dP - Dsum))
    out.o = O.transpose(1, 2).contiguous()
    out.dq = (dS @ kh).transpose(1, 2).contiguous()
    out.dk = (dS.transpose(2, 3) @ qh).transpose(1, 2).contiguous()
    out.dv = (P.transpose(2, 3) @ gh).transpose(1, 2).contiguous()
    return out


@functools.lru_cache(maxsize=None)
def exact(B, H, Lq, Lk, D, form, seed=0):
    return closed_form(build(B, H, Lq, Lk, D, form, seed))


def scores(d):
    """float64 scores [B, H, Lq, Lk] (scale = 1), no mask."""
    return d.q.transpose(1, 2) @ d.k.transpose(1, 2).transpose(2, 3)


def softmax_reference(d, k=None, v=None, mask=None, grad=False):
    """float64 softmax(Q K^T [+ mask]) V as plain torch statements; with ``grad`` also dQ, dK, dV for d.dout by autograd."""
    q = d.q.clone().requires_grad_(grad)
    k = (d.k if k is None else k).clone().requires_grad_(grad)
    v = (d.v if v is None else v).clone().requires_grad_(grad)
    s = q.transpose(1, 2) @ k.transpose(1, 2).transpose(2, 3)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    o = (p @ v.transpose(1, 2)).transpose(1, 2)
    if not grad:
        return SimpleNamespace(o=o, p=p)
    o.backward(d.dout)
    return SimpleNamespace(o=o.detach(), p=p.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def off_set_weight(d, p):
    """W: the largest total weight a query gives to keys outside S(i), from the float64 softmax ``p``."""
    return float((p * (selection_matrix(d) == 0)).sum(-1).max())


def backward_floor(d, W):
    """Bound on what the keys outside S(i) add to a gradient element: W Lk max|dP - D| max(|q|, |k|)."""
    ex = closed_form(d)
    return W * d.Lk * float(ex.dPmD.abs().max()) * max(float(d.q.abs().max()), float(d.k.abs().max()))


def representable(t, dtype):
    return torch.equal(t.to(torch.float32).to(dtype).double(), t)


# ---- causal (madm_causal_attention_fwd: f32, D = 64, L <= 128, 16 query rows per workgroup) ----
CB = 16                     # thermometer block = the kernel's query chunk
N_TB, N_TO = 7, 15          # dims [j >= 16 m], m = 1..7 and [j mod 16 >= n], n = 1..15
BAIT = 40.0


@functools.lru_cache(maxsize=None)
def build_causal(L, form, seed=0):
    """Causal selector inputs: S(i) inside the visible keys 0..i, and for every query with a later key a bait key j* > i
    whose score is exactly +40.

    Head layout: 41 code dims | 7 block dims | 15 offset dims | 1 bias dim.  Two ways to place the bait:
      mode A (j* = i + 1 in the same 16-key block): weight y on the offset dim n = i mod 16 + 1 and the same weight on the
              block dim of i's own block, with S(i) chosen inside that block.  Visible keys: S(i) gets y from the block dim
              (cancelled by the bias); keys of earlier blocks get at most y - y = 0 on top of their code penalty; keys of the
              own block up to i get the same y as S(i).  Key i + 1 gets 2 y.
      mode B (j* = first key of the next block): weight y on that block's dim; no visible key has it set.
    y = 40 - (code score of j*), so that j* scores exactly +40.  The last block's queries use mode A, a query at the end of
    a block mode B, the others a seeded mix."""
    assert form in FORMS and 1 <= L <= 128
    B, H, D = CAUSAL_B, CAUSAL_H, CAUSAL_D
    g = torch.Generator().manual_seed(5000 + 1000 * seed + 2 * L + (1 if form == "pair" else 0))
    nbits = _bits(L)
    Dc = D - 1 - N_TB - N_TO
    kc = _code(B, H, L, Dc, nbits)
    cs = code_scale(L, Dc)
    j = torch.arange(L)
    tb = (j.view(L, 1) >= CB * torch.arange(1, N_TB + 1).view(1, N_TB)).double()
    to = ((j % CB).view(L, 1) >= torch.arange(1, N_TO + 1).view(1, N_TO)).double()
    k = torch.cat([kc, tb.expand(B, H, L, N_TB), to.expand(B, H, L, N_TO), torch.ones((B, H, L, 1), dtype=torch.float64)], -1)
    a = torch.zeros((B, H, L), dtype=torch.int64)
    b = torch.zeros((B, H, L), dtype=torch.int64)
    bait = torch.full((B, H, L), -1, dtype=torch.int64)
    q = torch.zeros((B, H, L, D), dtype=torch.float64)
    rnd = torch.rand((B, H, L, 3), generator=g)
    tperm = torch.rand((B, H, L, 7), generator=g).argsort(-1)
    for bi in range(B):
        for h in range(H):
            for i in range(L):
                blk, off = divmod(i, CB)
                nxt = CB * (blk + 1)
                if i + 1 >= L:
                    mode = None
                elif off == CB - 1:
                    mode = "B"
                else:
                    mode = "A" if (nxt >= L or rnd[bi, h, i, 0] < 0.5) else "B"
                lo = CB * blk if mode == "A" else 0
                r = float(rnd[bi, h, i, 1])
                ai = i if r < 0.25 else (lo if r < 0.35 else lo + int(float(rnd[bi, h, i, 2]) * (i - lo + 1)))
                ai = min(ai, i)
                bj = ai
                if form == "pair":
                    for t in tperm[bi, h, i].tolist():
                        cand = ai ^ (1 << t)
                        if t < nbits and lo <= cand <= i:
                            bj = cand
                            break
                qc = cs * (kc[bi, h, ai] + kc[bi, h, bj]) / 2
                base = float(qc @ kc[bi, h, ai])
                q[bi, h, i, :Dc] = qc
                boost_a = 0.0
                if mode is not None:
                    js = i + 1 if mode == "A" else nxt
                    y = BAIT - (float(qc @ kc[bi, h, js]) - base)
                    if mode == "A":
                        q[bi, h, i, Dc + N_TB + off] = y             # offset dim n = off + 1
                        if blk >= 1:
                            q[bi, h, i, Dc + blk - 1] = y            # block dim m = blk
                            boost_a = y
                    else:
                        q[bi, h, i, Dc + blk] = y                    # block dim m = blk + 1
                    bait[bi, h, i] = js
                q[bi, h, i, D - 1] = -(base + boost_a)
                a[bi, h, i], b[bi, h, i] = ai, bj
    g2 = torch.Generator().manual_seed(77 + L)
    v = _values((B, L, H, D), g2)
    return SimpleNamespace(B=B, H=H, Lq=L, Lk=L, D=D, form=form, q=q.transpose(1, 2).contiguous(),
                           k=k.transpose(1, 2).contiguous(), v=v, dout=torch.zeros((B, L, H, D), dtype=torch.float64),
                           a=a, b=b, bait=bait, causal=True)


def causal_mask(L):
    return torch.ones((L, L), dtype=torch.bool).tril()
