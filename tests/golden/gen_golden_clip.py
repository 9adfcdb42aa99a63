"""Generates tests/golden/clip_text_tiny.npz: the fp32 ``last_hidden_state`` (after ``final_layer_norm``) of
``transformers.CLIPTextModel`` -- the class the reference loads from the snapshot's text_encoder/
(modeling/meta_arch/ldm_diffusers.py:57-58,76,219-243) -- at a small config, for three rows of token ids.  Needs
``transformers`` (the GPU test that reads the fixture does not).

The weights are NOT stored (2 MB of random f32 would not compress): they are ``weights.synth_init_`` draws keyed by the
checkpoint names (``text_model.<...>``), so tests/test_clip_gpu.py redraws the same values on the HIP module tree.

    python tests/golden/gen_golden_clip.py       # writes tests/golden/clip_text_tiny.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from madm_amd import weights  # noqa: E402

SEED = 7
# 2 layers, width 128, 2 heads of 64, MLP 512, 1 000 tokens with BOS / EOS the last two ids, 77 positions
TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
BOS, EOS = 998, 999


def id_rows():
    g = torch.Generator().manual_seed(11)
    empty = [BOS] + [EOS] * 76                                                # tokenizer('') padded with EOS
    full = [BOS] + torch.randint(0, BOS, (75,), generator=g).tolist() + [EOS]  # a prompt that fills all 77 positions
    rand = torch.randint(0, TINY["vocab_size"], (77,), generator=g).tolist()  # any id anywhere
    return torch.tensor([empty, full, rand], dtype=torch.int64)


def synth_hf(model, seed):
    """synth_init_ under the checkpoint names whatever transformers' own prefix (4.x keeps ``text_model.``, 5.x drops it)."""
    first = next(iter(model.state_dict()))
    return weights.synth_init_(model, seed, prefix="" if first.startswith("text_model.") else "text_model.")


def main():
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = CLIPTextConfig(**TINY, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=EOS, attn_implementation="eager")
    model = synth_hf(CLIPTextModel(cfg).eval(), SEED)
    ids = id_rows()
    with torch.no_grad():
        out = model(input_ids=ids).last_hidden_state.float()
    path = os.path.join(HERE, "clip_text_tiny.npz")
    np.savez_compressed(path, ids=ids.numpy(), last_hidden_state=out.numpy(), seed=np.int64(SEED),
                        config=np.array(repr(sorted(TINY.items()))))
    print(f"wrote {path}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}")


if __name__ == "__main__":
    main()
