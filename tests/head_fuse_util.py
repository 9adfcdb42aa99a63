"""Shared by the tests of ``DAFormerHead(final_fuse_vae_decoder_feat=True)`` (host-only torch code):

* the fixture cases, their seeded inputs and how a gradient is sampled into a fixture (tests/golden/gen_golden_headfuse.py
  writes with these, the tests read with them);
* ``FlaggedOracleHead``: a restatement of daformer_head.py:677-749 with the flag, on ``oracle.madm_path.OracleHead`` and
  ``oracle.third_party.BottleneckBlock`` (run in float64 by the tests);
* the fused classifier (include/madm_headfuse.h): its float64 reference with named mutants, integer-lattice inputs that make
  the result exact in f32 / bf16 / f16, and the per-element bound for random inputs.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ["s0", "s3", "s4", "s5"]
CHANNELS = [128, 512, 512, 512]
K = 11
SEED = 7
# name -> (B, [(H, W) per key], train mode)
CASES = {
    "headfuse_eval": (1, [(64, 64), (8, 8), (4, 4), (2, 2)], False),
    "headfuse_eval_odd": (1, [(72, 40), (9, 5), (5, 3), (3, 2)], False),
    "headfuse_eval_odd_s0": (1, [(71, 39), (9, 5), (5, 3), (3, 2)], False),
    "headfuse_train": (2, [(64, 64), (8, 8), (4, 4), (2, 2)], True),
}
# 72 x 40 halves to 36 x 20: odd for the small scales' resizes (9 x 5 -> 36 x 20 is no power of two), but still an exact 2x
# for the classifier, so that case takes the fused kernel.  The route that is NOT a 2x needs an odd s0: 71 x 39 -> 35 x 19.


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def case_feats(name):
    B, sizes, _ = CASES[name]
    return {k: torch.randn((B, c, h, w), generator=_gen(100 + i)) for i, (k, c, (h, w)) in enumerate(zip(KEYS, CHANNELS, sizes))}


def case_dropout_scale(name):
    B = CASES[name][0]
    keep = torch.rand((B, 256), generator=_gen(200)) >= 0.1
    return keep.to(torch.float32) / 0.9


def case_dlogits(name):
    B, sizes, _ = CASES[name]
    H, W = sizes[0]
    return torch.randn((B, K, H, W), generator=_gen(300)) / (B * H * W)


SAMPLE = 2048


def sample(t):
    """what a fixture keeps of a gradient: (at most SAMPLE evenly spaced elements of the flattened tensor, its L2 norm)"""
    f = t.detach().reshape(-1).double()
    step = max(1, -(-f.numel() // SAMPLE))
    return f[::step].float().numpy(), np.float64(f.norm().item())


def head_cfg():
    return dict(out_features=list(KEYS), head_in_channels=list(CHANNELS), num_classes=K)


class FlaggedOracleHead(nn.Module):
    """The flagged head on the oracle's modules.  ``dropout``: oracle.train_path.FixedDropout2d (a FIFO of scales)."""

    def __init__(self, cfg=None):
        super().__init__()
        from oracle import madm_path, third_party as tp, train_path
        cfg = head_cfg() if cfg is None else cfg
        base = madm_path.OracleHead(cfg)
        self.in_keys = base.in_keys
        self.embed_layers, self.fuse_layer = base.embed_layers, base.fuse_layer
        self.vae_decoder_feat_proj = nn.Sequential(tp.BottleneckBlock(128, 64, bottleneck_channels=32, norm="GN"))
        self.conv_seg = nn.Conv2d(256 + 64, cfg["num_classes"], 1)
        self.dropout = train_path.FixedDropout2d()

    def forward(self, input_dict):
        x = [input_dict['output_features'][k] for k in self.in_keys]
        s0 = x[0]
        x[0] = F.interpolate(s0, size=(s0.shape[2] // 2, s0.shape[3] // 2), mode='bilinear', align_corners=False)
        n = x[-1].shape[0]
        os_size = x[0].shape[2:]
        cs = []
        for i, f in enumerate(x):
            c = self.embed_layers[str(i)](f).permute(0, 2, 1).contiguous().reshape(n, -1, f.shape[2], f.shape[3])
            if c.shape[2:] != os_size:
                c = F.interpolate(c, size=os_size, mode='bilinear', align_corners=False)
            cs.append(c)
        feat = self.dropout(self.fuse_layer(torch.cat(cs, dim=1)))
        feat = F.interpolate(feat, size=s0.shape[2:], mode='bilinear', align_corners=False)
        return self.conv_seg(torch.cat((feat, self.vae_decoder_feat_proj(s0)), dim=1))


def init_head_(head):
    from madm_amd import weights
    weights.synth_init_(head, SEED, "head.")
    weights.synth_buffers_(head, SEED, "head.")
    return head


def run_case(head, name):
    """Runs a head with the oracle's interface (the reference's class or FlaggedOracleHead, already initialised) on a fixture
    case.  Returns {array name: numpy array} as the fixture stores it."""
    B, sizes, train = CASES[name]
    feats = case_feats(name)
    dt = next(head.parameters()).dtype
    feats = {k: v.to(dt) for k, v in feats.items()}
    out = {}
    if not train:
        head.eval()
        with torch.no_grad():
            out["logits"] = head({'output_features': dict(feats)}).float().numpy()
        return out
    head.train()
    head.dropout.scales = [case_dropout_scale(name).to(dt)]
    for v in feats.values():
        v.requires_grad_(True)
    logits = head({'output_features': dict(feats)})
    logits.backward(case_dlogits(name).to(dt))
    out["logits"] = logits.detach().float().numpy()
    for n_, p in head.named_parameters():
        out["grad:" + n_], out["gnorm:" + n_] = sample(p.grad)
    for k, v in feats.items():
        out["dfeat:" + k], out["dfnorm:" + k] = sample(v.grad)
    for n_, b in head.named_buffers():
        if n_.endswith(("running_mean", "running_var")):
            out["bn:" + n_] = b.detach().float().numpy().copy()
    return out


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the fused classifier ------------------------------------------------------------------------------------------------
def _axis(n_out, n_in, mutant):
    """PyTorch's align_corners=False source rows and weight of the second one at scale 1/2, per output index (float64)."""
    o = torch.arange(n_out, dtype=torch.float64)
    src = (o + 0.5) * 0.5 - 0.5
    if mutant != "no_clamp":
        src = src.clamp(min=0)
    i0 = torch.floor(src).long()
    lam = src - i0
    if mutant == "no_clamp":          # the border reads the far side of the map instead of its own edge
        i0, i1 = i0 % n_in, (i0 + 1) % n_in
    else:
        i0 = i0.clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
    if mutant == "swap_weights":
        lam = 1.0 - lam
    return i0, i1, lam


def _swapped(ly, lx):
    H, W = ly.numel(), lx.numel()
    py, px = torch.arange(H) % 2, torch.arange(W) % 2         # interior lambdas by parity: even 0.75, odd 0.25
    lam = lambda par: torch.where(par == 0, 0.75, 0.25).double()      # noqa: E731
    return lam(px)[None, :].expand(H, W), lam(py)[:, None].expand(H, W)


def up2x(x, mutant=None):
    """x [B, h, w, C] float64 -> [B, 2h, 2w, C]: the exact bilinear 2x (dyadic weights: no rounding in float64 on lattice data)"""
    B, h, w, C = x.shape
    y0, y1, ly = _axis(2 * h, h, mutant)
    x0, x1, lx = _axis(2 * w, w, mutant)
    LY, LX = ly[:, None].expand(2 * h, 2 * w), lx[None, :].expand(2 * h, 2 * w)
    if mutant == "swap_xy":           # the row weight taken from the column's parity and the other way round
        LY, LX = _swapped(ly, lx)
    LY, LX = LY[None, :, :, None], LX[None, :, :, None]
    g = lambda yy, xx: x[:, yy][:, :, xx]      # noqa: E731
    return (1 - LY) * (1 - LX) * g(y0, x0) + (1 - LY) * LX * g(y0, x1) + LY * (1 - LX) * g(y1, x0) + LY * LX * g(y1, x1)


MUTANTS = ["no_clamp", "swap_weights", "swap_xy", "swap_halves", "shift_class", "no_bias"]
SPATIAL_MUTANTS = {"no_clamp": (2, 2), "swap_weights": (2, 2), "swap_xy": (2, 2)}   # smallest (h, w) on which they are visible


def classify_ref(hd, proj, w, bias, dtype, mutant=None):
    """float64 result of mhf_upsample_cat_classify: hd [B, h, w, C1], proj [B, 2h, 2w, C2], w [Kp, C1 + C2], bias [Kp] (values
    already representable in ``dtype``) -> [B, 2h, 2w, Kp].  The upsampled value is rounded once to ``dtype``."""
    hd, proj, w, bias = hd.double(), proj.double(), w.double(), bias.double()
    C1 = hd.shape[-1]
    up = up2x(hd, mutant)
    if dtype != torch.float32:
        up = up.to(dtype).double()
    if mutant == "swap_halves":
        w = torch.cat((w[:, -C1:], w[:, :-C1]), dim=1)
    if mutant == "shift_class":
        w = torch.cat((w[:1], torch.roll(w[1:2], 1, dims=1), w[2:]), dim=0)
    out = up @ w[:, :C1].t() + proj @ w[:, C1:].t()
    return out if mutant == "no_bias" else out + bias


KERNEL_SIZES = [(1, 1), (3, 5), (17, 9), (40, 24)]     # h x w: every clamp, ragged 4 x 8 tiles, several workgroups per axis
KERNEL_KS = [9, 11, 19]
KERNEL_B, C1, C2 = 2, 256, 64
ACC_MAX = float(1 << 24)


def kp_of(k):
    return (k + 3) // 4 * 4


def lattice_case(h, w, k, seed=0):
    """Integer data on which every value the kernel forms is exact: hd in multiples of 16 (|hd| <= 48: the weights are
    k / 16, so every upsampled value is an integer of magnitude <= 48, which bf16 and f16 hold), integer classifier weights
    |w| <= 2, integer proj |p| <= 4 and bias.  Rows k .. Kp - 1 of w and bias are zero as the packed operand has them."""
    g = _gen(1000 + 131 * h + 17 * w + k + seed)
    B, kp = KERNEL_B, kp_of(k)
    hd = 16.0 * torch.randint(-3, 4, (B, h, w, C1), generator=g).double()
    proj = torch.randint(-4, 5, (B, 2 * h, 2 * w, C2), generator=g).double()
    wt = torch.randint(-2, 3, (kp, C1 + C2), generator=g).double()
    bias = torch.randint(-9, 10, (kp,), generator=g).double()
    wt[k:] = 0
    bias[k:] = 0
    return hd, proj, wt, bias


def random_case(h, w, k, dtype, seed=0):
    g = _gen(5000 + 131 * h + 17 * w + k + seed)
    B, kp = KERNEL_B, kp_of(k)
    q = lambda t: t.to(dtype).double()      # noqa: E731
    hd = q(torch.randn((B, h, w, C1), generator=g))
    proj = q(torch.randn((B, 2 * h, 2 * w, C2), generator=g))
    wt = q(torch.randn((kp, C1 + C2), generator=g) / 16)
    bias = torch.randn((kp,), generator=g).float().double()
    wt[k:] = 0
    bias[k:] = 0
    return hd, proj, wt, bias


def check_exact(hd, proj, wt, bias):
    """the exactness conditions of a lattice case; returns the float64 result"""
    up = up2x(hd)
    assert bool(torch.equal(up, up.round())) and float(up.abs().max()) <= 48
    for dt in (torch.bfloat16, torch.float16):
        for t in (hd, proj, wt, up):
            assert bool(torch.equal(t.to(dt).double(), t)), "a lattice value is not representable"
    # the four products of the blend are integers as well: 16 m * k / 16
    assert bool(torch.equal(hd / 16, (hd / 16).round()))
    mag = up.abs() @ wt[:, :C1].abs().t() + proj.abs() @ wt[:, C1:].abs().t() + bias.abs()
    assert float(mag.max()) < ACC_MAX          # the sum of magnitudes bounds every partial sum in every order
    out = classify_ref(hd, proj, wt, bias, torch.float32)
    assert bool(torch.equal(out, out.round()))
    return out


EPS = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}


def classify_bound(hd, proj, wt, bias, dtype):
    """Per-element bound on |kernel - float64| for inputs already rounded to ``dtype`` (DESIGN section 26's rule: one operand
    rounding plus the f32 accumulation term):

    * the blend runs in f32 with exact (dyadic) weights: four products and three sums, at most 7 roundings of 2^-24 relative to
      A = sum_i w_i |v_i| (the same blend of the magnitudes, >= |u|);
    * ONE rounding of the blended value to the compute dtype: half an ulp, eps = 2^-9 (bf16) / 2^-11 (f16) / 0 (f32) relative
      to at most A (1 + 7 * 2^-24);
    * K = C1 + C2 products (exact in the MFMA: 16-bit x 16-bit, or f32 fma) accumulated in f32 plus the bias: K + 1 additions.
      The 16-bit MFMA's inner adder is not documented to round to nearest, so each addition is granted a whole ulp, 2^-23, of the
      sum of the magnitudes S = sum_k |w_k| A_k + |bias|.  Split-K partial sums of the composed path stay inside this count.
    """
    eps = EPS[dtype]
    u24 = 2.0 ** -24
    A = up2x(hd.double().abs())
    du = A * (7 * u24 + eps * (1 + 7 * u24))
    w1, w2 = wt[:, :C1].double().abs(), wt[:, C1:].double().abs()
    S = A @ w1.t() + proj.double().abs() @ w2.t() + bias.double().abs()
    return du @ w1.t() + (C1 + C2 + 1) * 2.0 ** -23 * (S + du @ w1.t())
