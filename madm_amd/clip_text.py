"""CLIP text encoder (HF ``CLIPTextModel``, the ViT-L/14 text tower of SD-v1-4) on the HIP path.

The reference loads it from the snapshot's ``text_encoder/`` and runs it in fp32 on the empty prompt once at construction
(modeling/meta_arch/ldm_diffusers.py:57-58,76,219-243,268-280): ``last_hidden_state`` after ``final_layer_norm``, all 77
rows, is ``uncond_inputs``.  Here every layer is a libmadm_hip launch in f32 whatever the UNet's compute dtype:

    token + position embedding                      madm_token_embedding
    per layer (pre-LayerNorm):
      LayerNorm1 folded into the fused QKV linear   madm_conv2d_fwd (N = 3 C, ln_colsum)
      causal attention over the QKV column windows  madm_causal_attention_fwd
      out_proj + residual                           madm_conv2d_fwd
      LayerNorm2 folded into fc1                    madm_conv2d_fwd (ln_colsum)
      quick_gelu                                    madm_quick_gelu
      fc2 + residual                                madm_conv2d_fwd
    final LayerNorm                                 madm_layernorm_fwd

Parameter names are those of the SD-v1-4 ``text_encoder`` files (``text_model.embeddings.token_embedding.weight``, ...).

``python -m madm_amd.clip_text <snapshot> [--out PATH]`` writes ``uncond_inputs.pt`` (f32 [1, 77, 768]) for the snapshot.
"""
import json
import os

import torch
import torch.nn as nn

from . import ops
from .nn import Linear, LayerNorm, _Packed

IGNORED_KEYS = ("text_model.embeddings.position_ids",)   # a buffer older checkpoints carry; not a parameter
HEAD_DIM = 64                                            # the head dim madm_causal_attention_fwd serves
MAX_POSITIONS = 128                                      # its longest sequence

# SD-v1-4 text_encoder/config.json
SD14_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                   num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)


class Embedding(nn.Module):
    def __init__(self, num, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num, dim))


class CLIPEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])


class CLIPAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C = cfg["hidden_size"]
        self.heads = cfg["num_attention_heads"]
        self.head_dim = C // self.heads
        self.scale = self.head_dim ** -0.5
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (Linear(C, C) for _ in range(4))


class CLIPMLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.fc1 = Linear(cfg["hidden_size"], cfg["intermediate_size"])
        self.fc2 = Linear(cfg["intermediate_size"], cfg["hidden_size"])


class CLIPEncoderLayer(_Packed):
    def __init__(self, cfg):
        super().__init__()
        C, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.self_attn = CLIPAttention(cfg)
        self.layer_norm1 = LayerNorm(C, eps)
        self.mlp = CLIPMLP(cfg)
        self.layer_norm2 = LayerNorm(C, eps)

    def operands(self):
        """(fused QKV with LayerNorm1 folded, fc1 with LayerNorm2 folded): (W' f32 [N, C], bias', colsum) each; derived
        once and re-derived when a parameter changes."""
        a, m = self.self_attn, self.mlp
        n1, n2 = self.layer_norm1, self.layer_norm2

        def build():
            W = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0)
            b = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0)
            qkv = ops.fold_layernorm_pack(W, b, n1.weight, n1.bias, torch.float32)
            fc1 = ops.fold_layernorm_pack(m.fc1.weight, m.fc1.bias, n2.weight, n2.bias, torch.float32)
            return qkv, fc1

        ver = tuple((p._version, p.data_ptr()) for p in (a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias,
                                                         a.v_proj.weight, a.v_proj.bias, n1.weight, n1.bias, m.fc1.weight,
                                                         m.fc1.bias, n2.weight, n2.bias))
        return self._cache_get("ln_folded", build, ver=ver)

    def forward(self, h, B, L):
        """h: f32 [B*L, C] residual stream -> the layer's output (same shape)."""
        a, m = self.self_attn, self.mlp
        (wq, bq, cq), (w1, b1, c1) = self.operands()
        C = h.shape[1]
        qkv = ops.linear(h, wq, bias=bq, ln=(cq, self.layer_norm1.eps))
        o = ops.causal_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, a.heads, L, a.head_dim, a.scale)
        h = a.out_proj(o, residual=h)
        t = ops.quick_gelu(ops.linear(h, w1, bias=b1, ln=(c1, self.layer_norm2.eps)))
        return m.fc2(t, residual=h)


class CLIPEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList(CLIPEncoderLayer(cfg) for _ in range(cfg["num_hidden_layers"]))


class CLIPTextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = CLIPEmbeddings(cfg)
        self.encoder = CLIPEncoder(cfg)
        self.final_layer_norm = LayerNorm(cfg["hidden_size"], cfg["layer_norm_eps"])


def check_config(cfg):
    """The subset of CLIPTextConfig this encoder implements; anything else is refused."""
    cfg = dict(SD14_CONFIG, **{k: v for k, v in cfg.items() if k in SD14_CONFIG})
    if cfg["hidden_act"] != "quick_gelu":
        raise NotImplementedError(f"CLIP text encoder: hidden_act {cfg['hidden_act']!r} (only 'quick_gelu' is built)")
    C, H = cfg["hidden_size"], cfg["num_attention_heads"]
    if C % H or C // H != HEAD_DIM:
        raise NotImplementedError(f"CLIP text encoder: width {C} / {H} heads: head dim {C / H:g} "
                                  f"(the causal attention kernel serves {HEAD_DIM})")
    kt = ops.k_tile(torch.float32)
    if C % kt or cfg["intermediate_size"] % kt:
        raise NotImplementedError(f"CLIP text encoder: width {C} / MLP {cfg['intermediate_size']} not multiples of {kt}")
    if cfg["max_position_embeddings"] > MAX_POSITIONS:
        raise NotImplementedError(f"CLIP text encoder: {cfg['max_position_embeddings']} positions (at most {MAX_POSITIONS})")
    return cfg


class CLIPTextModel(nn.Module):
    """``CLIPTextModel(cfg)``; ``forward(ids [N, L] int64) -> [N, L, C] f32`` (``last_hidden_state``)."""

    def __init__(self, cfg=None):
        super().__init__()
        self.config = check_config(cfg or {})
        self.text_model = CLIPTextTransformer(self.config)

    @torch.no_grad()
    def forward(self, ids):
        tm = self.text_model
        tok = tm.embeddings.token_embedding.weight
        pos = tm.embeddings.position_embedding.weight
        ids_host = torch.as_tensor(ids, dtype=torch.int64).cpu()   # checked on the host, before upload
        if ids_host.dim() != 2:
            raise ValueError(f"CLIPTextModel: ids must be [N, L], got {tuple(ids_host.shape)}")
        N, L = ids_host.shape
        if L > pos.shape[0]:
            raise ValueError(f"CLIPTextModel: {L} tokens but only {pos.shape[0]} positions")
        V = tok.shape[0]
        bad = (ids_host < 0) | (ids_host >= V)
        if bool(bad.any()):
            raise ValueError(f"CLIPTextModel: token ids outside the vocabulary [0, {V}): {ids_host[bad][:8].tolist()}")
        if not tok.is_cuda:
            raise RuntimeError("CLIPTextModel runs on the HIP path only: move it to a CUDA (ROCm) device first")
        h = ops.token_embedding(ids_host.contiguous().to(tok.device), tok.detach(), pos.detach())
        for layer in tm.encoder.layers:
            h = layer(h, N, L)
        h = tm.final_layer_norm(h)
        return h.view(N, L, -1)


def read_config(snapshot):
    with open(os.path.join(snapshot, "text_encoder", "config.json")) as f:
        return json.load(f)


def load_text_encoder_dir(module, snapshot):
    """Loads ``<snapshot>/text_encoder/model.safetensors`` (falling back to ``pytorch_model.bin``) into ``module`` as
    strictly as weights.load_diffusers_dir: a missing or unexpected key raises; ``text_model.embeddings.position_ids``
    (a buffer older checkpoints carry) is ignored."""
    d = os.path.join(snapshot, "text_encoder")
    st = os.path.join(d, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    else:
        sd = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu")
    sd = {k: v.float() for k, v in sd.items() if k not in IGNORED_KEYS}
    missing, unexpected = module.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError(f"text_encoder: missing {missing[:5]}..., unexpected {unexpected[:5]}...")
    return module


def has_text_encoder(snapshot):
    return bool(snapshot) and os.path.isdir(os.path.join(snapshot, "text_encoder")) and \
        os.path.isdir(os.path.join(snapshot, "tokenizer"))


class TextEncoder:
    """Tokenizer + encoder of a snapshot: ``TextEncoder(snapshot, device)(texts) -> [N, max_length, C] f32``."""

    def __init__(self, snapshot, device):
        from .clip_tokenizer import CLIPTokenizer
        for sub in ("text_encoder", "tokenizer"):
            if not os.path.isdir(os.path.join(snapshot, sub)):
                raise FileNotFoundError(f"{snapshot!r} has no {sub}/ directory: the CLIP text encoder needs the "
                                        "snapshot's text_encoder/ and tokenizer/")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the CLIP text encoder runs on the HIP path only (device {device}); it has no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.tokenizer = CLIPTokenizer.from_dir(os.path.join(snapshot, "tokenizer"))
        model = CLIPTextModel(read_config(snapshot))
        load_text_encoder_dir(model, snapshot)
        self.model = model.to(device)

    def __call__(self, texts):
        return self.model(torch.tensor(self.tokenizer(list(texts)), dtype=torch.int64))


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Write <snapshot>/uncond_inputs.pt: the CLIP text embedding of '' "
                                             "(f32 [1, 77, 768]) computed by the HIP text encoder")
    ap.add_argument("snapshot", help="diffusers snapshot directory with text_encoder/ and tokenizer/")
    ap.add_argument("--out", default=None, help="output path (default: <snapshot>/uncond_inputs.pt)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    emb = TextEncoder(os.path.expanduser(args.snapshot), args.device)([""]).cpu().contiguous()
    out = args.out or os.path.join(os.path.expanduser(args.snapshot), "uncond_inputs.pt")
    torch.save(emb, out)
    print(f"wrote {out}: {tuple(emb.shape)} {emb.dtype}")


if __name__ == "__main__":
    main()
