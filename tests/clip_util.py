"""Shared by the CLIP tests: a synthetic CLIP tokenizer directory (vocab.json / merges.txt / special-token files in the
layout of the SD-v1-4 snapshot's tokenizer/, special tokens last) and a torch-CPU fp32 restatement of HF CLIPTextModel's
``last_hidden_state``."""
import collections
import json
import os

import torch
import torch.nn.functional as F

from madm_amd.clip_tokenizer import bytes_to_unicode, normalize, split_words

CORPUS = ["a photo of a cat sitting on the mat", "the quick brown fox jumps over the lazy dog 1234567890",
          "don't stop, it's 3:45pm!! we'll see... they're here, I'm sure you've heard", "cafe café résumé naïve façade",
          "a street scene at night, foggy and dark; cars, people and buildings"]


def _symbols(word, b2u):
    s = "".join(b2u[b] for b in word.encode("utf-8"))
    return tuple(s[:-1]) + (s[-1] + "</w>",)


def write_tokenizer(d, corpus=CORPUS, n_merges=300, vocab_size=None):
    """Byte-level base symbols (with and without ``</w>``), ``n_merges`` merges learned from ``corpus``, optional filler
    entries up to ``vocab_size``, then ``<|startoftext|>`` / ``<|endoftext|>`` as the last two ids.  Returns the vocab."""
    b2u = bytes_to_unicode()
    base = list(b2u.values())
    vocab = base + [c + "</w>" for c in base]
    words = collections.Counter(_symbols(w, b2u) for t in corpus for w in split_words(normalize(t)))
    merges = []
    for _ in range(n_merges):
        pairs = collections.Counter()
        for w, c in words.items():
            for p in zip(w[:-1], w[1:]):
                pairs[p] += c
        if not pairs:
            break
        best = max(pairs, key=lambda p: (pairs[p], p))
        merges.append(best)
        vocab.append(best[0] + best[1])
        merged = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i < len(w) - 1 and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1])
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            merged[tuple(out)] += c
        words = merged
    if vocab_size is not None:
        vocab += [f"filler{i}</w>" for i in range(vocab_size - 2 - len(vocab))]
    vocab += ["<|startoftext|>", "<|endoftext|>"]
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump({t: i for i, t in enumerate(vocab)}, f, ensure_ascii=False)
    with open(os.path.join(d, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    with open(os.path.join(d, "special_tokens_map.json"), "w") as f:
        json.dump({"bos_token": {"content": "<|startoftext|>"}, "eos_token": {"content": "<|endoftext|>"},
                   "pad_token": "<|endoftext|>", "unk_token": {"content": "<|endoftext|>"}}, f)
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump({"model_max_length": 77, "tokenizer_class": "CLIPTokenizer", "do_lower_case": True}, f)
    return vocab


def restate_clip(sd, cfg, ids):
    """HF CLIPTextModel's last_hidden_state (after final_layer_norm) in torch-CPU fp32 from a state dict with the
    checkpoint names."""
    sd = {k: v.detach().cpu().float() for k, v in sd.items()}
    C, H, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    D = C // H
    N, L = ids.shape
    ln = lambda x, p: F.layer_norm(x, (C,), sd[p + ".weight"], sd[p + ".bias"], eps)  # noqa: E731
    lin = lambda x, p: F.linear(x, sd[p + ".weight"], sd[p + ".bias"])             # noqa: E731
    x = sd["text_model.embeddings.token_embedding.weight"][ids] + sd["text_model.embeddings.position_embedding.weight"][:L]
    mask = torch.full((L, L), float("-inf")).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        h = ln(x, p + "layer_norm1")
        q, k, v = (lin(h, p + f"self_attn.{n}_proj").view(N, L, H, D).transpose(1, 2) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5 + mask, dim=-1) @ v
        x = x + lin(a.transpose(1, 2).reshape(N, L, C), p + "self_attn.out_proj")
        h = lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), p + "mlp.fc2")
    return ln(x, "text_model.final_layer_norm")
