"""CLIP tokenizer / text encoder surface (madm_amd/clip_tokenizer.py, madm_amd/clip_text.py): CPU-only, no kernel launches.
The transformers comparisons skip where transformers is not installed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from clip_util import restate_clip, write_tokenizer
from madm_amd import clip_text, weights
from madm_amd.clip_tokenizer import CLIPTokenizer

HERE = os.path.dirname(os.path.abspath(__file__))

PROMPTS = ["", "a photo of a cat", "A Photo   OF a\tcat\n", "the quick brown fox jumps over the lazy dog",
           "1234567890 3.14 2024-06-01 42nd", "hello, world!!! (really?) #tag @user ...",
           "don't stop: it's here, we'll see; they're gone, I'm sure you've heard he'd go",
           "'sun 'llama 'DON'T", "café résumé naïve façade Ærøskøbing Zürich", "ÀÉÎÕÜ àéîõü ñ ç",
           " ".join(["street"] * 90), "x" * 300]


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("clip_tok")
    write_tokenizer(str(d))
    return str(d)


def test_empty_prompt_is_bos_then_eos_padding(tmp_path):
    write_tokenizer(str(tmp_path), vocab_size=49408)
    tok = CLIPTokenizer.from_dir(str(tmp_path))
    assert (tok.bos_id, tok.eos_id, tok.pad_id, tok.max_length) == (49406, 49407, 49407, 77)
    assert tok([""]) == [[49406] + [49407] * 76]


def test_truncation_keeps_eos(tok_dir):
    tok = CLIPTokenizer.from_dir(tok_dir)
    ids = tok(" ".join(["cat"] * 200))[0]
    assert len(ids) == 77 and ids[0] == tok.bos_id and ids[-1] == tok.eos_id and tok.eos_id not in ids[1:-1]
    short = tok("a cat")[0]
    assert short[-1] == tok.pad_id and len(short) == 77


@pytest.mark.parametrize("text", PROMPTS)
def test_bpe_matches_transformers(tok_dir, text):
    transformers = pytest.importorskip("transformers")
    ref = transformers.CLIPTokenizer.from_pretrained(tok_dir)
    want = ref(text, padding="max_length", truncation=True, max_length=77).input_ids
    got = CLIPTokenizer.from_dir(tok_dir)(text)[0]
    assert got == want


def _ours_names(cfg):
    with torch.device("meta"):
        m = clip_text.CLIPTextModel(cfg)
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_parameter_names_match_transformers_sd14():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPTextConfig(**clip_text.SD14_CONFIG)
    with torch.device("meta"):
        hf = transformers.CLIPTextModel(cfg)
    want = {}
    for k, v in hf.state_dict().items():
        k = k if k.startswith("text_model.") else "text_model." + k     # transformers 5.x drops the prefix; the files keep it
        if k not in clip_text.IGNORED_KEYS:
            want[k] = tuple(v.shape)
    assert _ours_names(clip_text.SD14_CONFIG) == want
    assert len(want) == 2 + 12 * 16 + 2


def test_config_refusals():
    clip_text.check_config(clip_text.SD14_CONFIG)
    with pytest.raises(NotImplementedError, match="quick_gelu"):
        clip_text.check_config(dict(clip_text.SD14_CONFIG, hidden_act="gelu"))
    with pytest.raises(NotImplementedError, match="head dim"):
        clip_text.check_config(dict(clip_text.SD14_CONFIG, hidden_size=1024, num_attention_heads=8, intermediate_size=4096))
    with pytest.raises(NotImplementedError, match="positions"):
        clip_text.check_config(dict(clip_text.SD14_CONFIG, max_position_embeddings=256))


TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def _tiny_sd():
    m = weights.synth_init_(clip_text.CLIPTextModel(TINY), 3)
    return m, {k: v.clone() for k, v in m.state_dict().items()}


def _save(snapshot, sd, bin_=False):
    d = os.path.join(snapshot, "text_encoder")
    os.makedirs(d, exist_ok=True)
    for n in ("model.safetensors", "pytorch_model.bin"):
        if os.path.exists(os.path.join(d, n)):
            os.remove(os.path.join(d, n))
    if bin_:
        torch.save(sd, os.path.join(d, "pytorch_model.bin"))
    else:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(d, "model.safetensors"))


def test_loader_is_strict(tmp_path):
    src, sd = _tiny_sd()
    sd_pos = dict(sd, **{"text_model.embeddings.position_ids": torch.arange(77)[None]})   # older checkpoints carry it
    for bin_ in (False, True):
        _save(str(tmp_path), sd_pos, bin_)
        m = clip_text.load_text_encoder_dir(clip_text.CLIPTextModel(TINY), str(tmp_path))
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k
    missing = dict(sd)
    missing.pop("text_model.encoder.layers.1.mlp.fc2.bias")
    _save(str(tmp_path), missing)
    with pytest.raises(RuntimeError, match="missing"):
        clip_text.load_text_encoder_dir(clip_text.CLIPTextModel(TINY), str(tmp_path))
    extra = dict(sd, **{"text_model.encoder.layers.2.mlp.fc2.bias": torch.zeros(128)})
    _save(str(tmp_path), extra)
    with pytest.raises(RuntimeError, match="unexpected"):
        clip_text.load_text_encoder_dir(clip_text.CLIPTextModel(TINY), str(tmp_path))


def test_ids_outside_vocab_are_rejected_on_the_host():
    m, _ = _tiny_sd()
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m(torch.tensor([[0, 1000]]))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m(torch.tensor([[-1, 5]]))
    with pytest.raises(RuntimeError, match="HIP path only"):   # valid ids on a CPU module: no CPU fallback
        m(torch.tensor([[0, 999]]))


def test_restatement_matches_transformers_fixture():
    """The torch restatement the GPU tests compare against reproduces transformers' output stored in the fixture."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from gen_golden_clip import SEED, TINY as GEN_TINY
    z = np.load(os.path.join(HERE, "golden", "clip_text_tiny.npz"))
    m = weights.synth_init_(clip_text.CLIPTextModel(GEN_TINY), SEED)
    ids = torch.from_numpy(z["ids"])
    got = restate_clip(m.state_dict(), m.config, ids)
    want = torch.from_numpy(z["last_hidden_state"])
    assert ((got - want).norm() / want.norm()).item() < 1e-5


def test_snapshot_with_text_encoder_on_cpu_raises(tmp_path):
    from madm_amd.ldm_rocm import LdmRocm
    _, sd = _tiny_sd()
    _save(str(tmp_path), sd)
    with open(os.path.join(tmp_path, "text_encoder", "config.json"), "w") as f:
        import json
        json.dump(TINY, f)
    write_tokenizer(str(tmp_path / "tokenizer"), vocab_size=1000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LdmRocm(str(tmp_path), [], [5, 8, 11], (), weights='synthetic', device='cpu')
    with pytest.raises(FileNotFoundError, match="tokenizer"):
        clip_text.TextEncoder(str(tmp_path / "nowhere"), "cuda")


def test_new_symbols_are_exported_and_refuse_bad_args():
    from madm_amd import _lib, ops
    names = {n for n, _, _ in _lib.SYMBOLS}
    assert {"madm_token_embedding", "madm_causal_attention_fwd", "madm_quick_gelu"} <= names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("madm_token_embedding", "madm_causal_attention_fwd", "madm_quick_gelu"):
        assert hasattr(lib, n)
    for f in ("causal_attention", "token_embedding", "quick_gelu"):
        assert callable(getattr(ops, f))
    # every refusal happens on the host before any launch: fake (never dereferenced) pointers are enough
    fake = 0x1000

    def args(**kw):
        a = _lib.AttentionArgs()
        a.dtype, a.q, a.k, a.v, a.o = _lib.MADM_F32, fake, fake, fake, fake
        a.ldq = a.ldk = a.ldv = 3 * 768
        a.ldo = 768
        a.B, a.H, a.Lq, a.Lk, a.D, a.scale = 1, 12, 77, 77, 64, 0.125
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, msg in ((dict(dtype=_lib.MADM_F16), "f32 only"), (dict(dtype=_lib.MADM_BF16), "f32 only"),
                    (dict(D=40, ldo=480), "head dim"), (dict(Lk=76), "self-attention only"),
                    (dict(Lq=129, Lk=129), "sequence length"), (dict(Lq=0, Lk=0), "sequence length"),
                    (dict(ldq=700), "row strides")):
        rc = _lib.lib.madm_causal_attention_fwd(ctypes.byref(args(**kw)), None)
        assert rc == -1, kw
        assert msg in _lib.lib.madm_last_error().decode(), (kw, _lib.lib.madm_last_error())
    rc = _lib.lib.madm_token_embedding(fake, 1, 78, fake, 10, fake, 77, 64, fake, None)
    assert rc == -1 and b"positions" in _lib.lib.madm_last_error()
