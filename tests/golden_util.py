"""Shared by the CPU and GPU parity tests: seeded inputs of the golden cases and fixture loading."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHT_SEED = 0
CH_STRIDE_FULL = 16

CASES = {
    "small_t0": dict(B=2, H=64, W=64, t=0, cond_scale=0.0, lora=False),
    "small_t60": dict(B=2, H=64, W=64, t=60, cond_scale=0.02, lora=False),
    "small_lora": dict(B=2, H=64, W=64, t=60, cond_scale=0.02, lora=True),
    "rect_t0": dict(B=1, H=64, W=128, t=0, cond_scale=0.02, lora=False),
    "full_t0": dict(B=1, H=512, W=512, t=0, cond_scale=0.0, lora=False),
}


def make_inputs(B, H, W, t, cond_scale, **_):
    images = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(1234))
    cond = 0.02 * torch.randn((1, 77, 768), generator=torch.Generator().manual_seed(1235))
    cond_inputs = cond.repeat_interleave(B, dim=0)
    cond_emb = cond_scale * torch.randn((B, 1, 1280), generator=torch.Generator().manual_seed(1236))
    timesteps = torch.full((B,), t, dtype=torch.int64)
    shared_noise = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(42))
    return images, cond_inputs, cond_emb, timesteps, shared_noise


def load_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in 'fiub'}


def add_lora(unet, LoraConfig, seed=WEIGHT_SEED):
    """Same adapters / values as tests/golden/gen_golden.py::add_lora, for any module tree with the
    peft-shaped names (oracle or madm_amd)."""
    unet.add_adapter(LoraConfig(r=8, lora_alpha=8), "default")
    unet.add_adapter(LoraConfig(r=8, lora_alpha=16), "Depth")
    unet.set_adapter(["default", "Depth"])
    seed_lora_(unet, seed)
    for m in unet.modules():
        if hasattr(m, "_active_adapter"):
            m._active_adapter = ["Depth"]


def seed_lora_(unet, seed=WEIGHT_SEED):
    """Name-keyed seeded values for every LoRA tensor already present in ``unet`` (peft's own init has B = 0: the
    adapters would be no-ops and their A gradients zero)."""
    from madm_amd import weights
    with torch.no_grad():
        for name, p in unet.named_parameters():
            if ".lora_" in name:
                # A ~ N(0, 1/K) keeps x A^T O(1); B ~ 0.1 N(0, 1/r): a ~10-20 % perturbation of the base
                # layer (B = 0, peft's init, would make the adapter a no-op)
                g = weights._gen(seed, "unet." + name)
                gain = 0.1 if ".lora_B." in name else 1.0
                p.copy_((gain * torch.randn(p.shape, generator=g) / (p.shape[1] ** 0.5)).to(p.device))


def tap_subset(name, t):
    return t[:, ::CH_STRIDE_FULL] if name.startswith("full") else t


LORA_CONFIGS = ['default_r8_a8', 'Depth_r8_a16']


# ---- full inference forward (config 3): backbone + head + eval post-processing ---------------------------------
EVAL_CASES = {
    # non-512 input: /255, pad to 512x640, T.Resize to 512x512, head at 64x64, bilinear up + crop
    "eval_s345": dict(cfg="S345", H=480, W=640),
    # the shipped RGB->Depth configuration: VAE decoder -> s0 projection -> head at 512x512
    "eval_depth": dict(cfg="DEPTH", H=512, W=512),
    # the shipped RGB->Infrared configuration (K = 9, FMB test images are resized to 512 x 512 by the mapper,
    # config_files/common/data/cityscapes_rgb_to_fmb_9_infrared_semseg.py:43); RGB->Event is the Depth graph (K = 11)
    "eval_infrared": dict(cfg="INFRARED", H=512, W=512),
    # the Depth configuration with ``--lora_configs default_r8_a8 Depth_r8_a16`` (main.py:613-616,794) through the
    # meta-architecture's eval branch: 'name_rN_aM' parsing, set_multi_lora, set_lora_adapter(target) (mtmadise.py:48-54,
    # 115-147,672); LoRA values seeded by ``seed_lora_``
    "eval_depth_lora": dict(cfg="DEPTH", H=512, W=512, lora_configs=LORA_CONFIGS),
}


def eval_image(H, W):
    return 255.0 * torch.rand((3, H, W), generator=torch.Generator().manual_seed(777))


def init_eval_params(backbone, head, seed=WEIGHT_SEED):
    """Seeded parameters / BatchNorm statistics of everything outside unet/vae (name-keyed: identical values for the
    reference classes, the oracle restatement and the madm_amd modules)."""
    from madm_amd import weights
    for prefix, mod in (("backbone.feature_projections.", backbone.feature_projections),
                        ("backbone.clip_project_rgb.", backbone.feature_extractor.clip_project_rgb),
                        ("head.", head)):
        weights.synth_init_(mod, seed, prefix)
        weights.synth_buffers_(mod, seed, prefix)


# ---- label / pseudo-label pipeline (tests/golden/labels.npz) ----
LABEL_CASE = dict(B=2, K=19, H=48, W=80, thr=0.5, mix_seed=11)


def label_inputs(B, K, H, W, **_):
    """Seeded inputs of the label-pipeline tests: labels with ~8 % ignore pixels, a random K-colour palette, teacher
    logits at quarter resolution, two image / label pairs for ClassMix."""
    g = torch.Generator().manual_seed(4321)
    lab = torch.randint(0, K, (B, 1, H, W), generator=g)
    lab[torch.rand(lab.shape, generator=g) < 0.08] = 255
    palette = [int(v) for v in torch.randint(0, 256, (K * 3,), generator=g)]
    logits = 3.0 * torch.randn((B, K, H // 4, W // 4), generator=g)
    imgs = torch.randn((B, 3, H, W), generator=g)
    return {"label": lab, "palette": palette, "logits": logits, "imgs": imgs}


# ---- one training step of the shipped RGB->Depth configuration at 64 x 64 (tests/golden/train_depth.npz) --------------
TRAIN_CASE = dict(B=2, size=64, K=11, py_seed=20240, np_seed=20241, full_grad_max_numel=70000,
                  pseudo_threshold=0.25,     # low threshold: random-weight teachers are never 96.8 % confident
                  # the input seed is chosen so that NO teacher decision of any variant sits within fp32 noise of its
                  # discontinuity (tools/exp/scan_train_fixture_seed.py): smallest top-2 probability gap / distance
                  # of a max-probability to the threshold over the 8 192 pixels: depth 1.8e-5 / 2.1e-5, event 7.4e-5 / 6.0e-5,
                  # lora 9.5e-6 / 1.05e-5 (the round-2..4 seed 8899: 3.3e-6 / 3.9e-6, 1.5e-5 / 1.9e-6, 8.8e-7 / 1.06e-6)
                  input_seed=8908)
# model arguments of the shipped task configs (config_files/SemSeg/MTMADISE/*.py) that differ between the fixtures
TRAIN_VARIANTS = {
    "train_depth": dict(vae_decoder_loss='st', vae_decoder_loss_weight=[1.0, 1.0], denoise_timestep_range=[60, 61],
                        rev_noise_end_iter=5000),
    # mtmadise_cityscapes_rgb_to_event_11.py:43-58: source-only decoder loss with weight 20, teacher noise step 50
    "train_event": dict(vae_decoder_loss='s', vae_decoder_loss_weight=[20.0], denoise_timestep_range=[50, 51],
                        rev_noise_end_iter=8000),
    # --lora_configs default_r8_a8 Depth_r8_a16 --add_zero_grad on the Depth config (finetune_unet='all', the model
    # config's value, mtmadise_multi_lora.py:34): base weights AND both adapters train; 'default' gets its gradient from the
    # source pass, 'Depth' from the mixed-image pass (mtmadise.py:240,286)
    "train_depth_lora": dict(vae_decoder_loss='st', vae_decoder_loss_weight=[1.0, 1.0], denoise_timestep_range=[60, 61],
                             rev_noise_end_iter=5000, lora_configs=LORA_CONFIGS, add_zero_grad=True, finetune_unet='all'),
    # adapters only: finetune_unet='no' (main.py:558-559) freezes the UNet INCLUDING the adapters (ldm_diffusers.py:101-104
    # runs after peft marked them trainable, mtmadise.py:127), so the harness re-enables requires_grad on the LoRA tensors
    # (``lora_trainable``: peft's mark_only_lora_as_trainable convention, the north_star's LoRA mode -- NOT a reference
    # flag); a third adapter that no pass uses receives the zero gradient of add_zero_gead_on_unused_lora
    "train_depth_lora_only": dict(vae_decoder_loss='st', vae_decoder_loss_weight=[1.0, 1.0], denoise_timestep_range=[60, 61],
                                  rev_noise_end_iter=5000, lora_configs=LORA_CONFIGS + ['Event_r4_a4'], add_zero_grad=True,
                                  finetune_unet='no', lora_trainable=True),
}
HARNESS_KEYS = ("finetune_unet", "lora_trainable")     # not MTMADISE arguments


def model_args(variant):
    return {k: v for k, v in TRAIN_VARIANTS[variant].items() if k not in HARNESS_KEYS}


def prepare_lora_(unet, variant):
    """After construction of the meta-architecture: seeded LoRA values; ``lora_trainable`` variants mark the adapters
    trainable again."""
    v = TRAIN_VARIANTS[variant]
    if not v.get("lora_configs"):
        return
    seed_lora_(unet)
    if v.get("lora_trainable"):
        for n, p in unet.named_parameters():
            if ".lora_" in n:
                p.requires_grad = True


def train_inputs(B, size, K, input_seed, **_):
    """list[dict] as the dataset mapper hands it over (data/dataset/cross_modality_dataset.py:423-521): 0..255 images,
    int64 labels with ~6 % ignore pixels."""
    g = torch.Generator().manual_seed(input_seed)
    out = []
    for _i in range(B):
        lab = torch.randint(0, K, (1, size // 8, size // 8), generator=g)
        lab = lab.repeat_interleave(8, 1).repeat_interleave(8, 2)             # blocky regions, like real label maps
        noise = torch.rand((1, size, size), generator=g)
        lab[noise < 0.06] = 255
        out.append({"source_rgb": 255.0 * torch.rand((3, size, size), generator=g), "source_label": lab.long(),
                    "target_second_modality": 255.0 * torch.rand((3, size, size), generator=g),
                    "width": size, "height": size})
    return out


TIE_BAND = 1.5e-6      # what fp32 summation order can move a teacher probability by (f32 forward parity: 2 .. 6e-6 of the
# logits' magnitude, tests/test_parity_gpu.py)


def fixture_decision_margins(gold, size, pseudo_threshold):
    """From the fixture's own teacher logits: per pixel, the gap between the two largest class probabilities (an argmax tie
    flips the pseudo label) and the distance of the largest one to the confidence threshold (a crossing moves pseudo_weight
    by 1 / pixels) -- mtmadise.py:339-349.  A build may legitimately differ from the fixture only at pixels whose margin is
    inside TIE_BAND; with no such pixel the labels must be exact and the losses meet the tight gate."""
    x = torch.nn.functional.interpolate(gold["ema_logits"], size=(size, size), mode="bilinear", align_corners=False)
    top = torch.softmax(x.double(), dim=1).topk(2, dim=1).values
    return top[:, 0] - top[:, 1], (top[:, 0] - pseudo_threshold).abs()


def criterion_inputs():
    """Seeded logits / labels / weights / latents of the criterion pin (tests/golden/reference_pins.npz criterion_*):
    (source logits, target logits, decoder prediction) as fresh leaf tensors, and the targets dict."""
    B, K, h, H = 2, 11, 16, 64
    sp = torch.randn((B, K, h, h), generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    tp_ = torch.randn((B, K, h, h), generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    pred = torch.randn((B, 4, 8, 8), generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    gt = torch.randint(0, K, (B, 1, H, H), generator=torch.Generator().manual_seed(4))
    gt[torch.rand((B, 1, H, H), generator=torch.Generator().manual_seed(5)) < 0.1] = 255
    tgt = {'source_gt': gt, 'target_pl': gt.flip(0), 'target_pw': torch.rand((B, H, H), generator=torch.Generator().manual_seed(6)),
           'vae_decoder_loss': {'source': {'pred': pred, 'gt': torch.randn((B, 4, 8, 8), generator=torch.Generator().manual_seed(7)),
                                           'mask': torch.rand((B, 1, H, H), generator=torch.Generator().manual_seed(8)),
                                           'loss_weight': 20.0, 'loss_type': 'L1'},
                                'target': {'pred': pred * 0.5, 'gt': torch.randn((B, 4, 8, 8), generator=torch.Generator().manual_seed(9)),
                                           'mask': torch.rand((B, 1, H, H), generator=torch.Generator().manual_seed(10)),
                                           'loss_weight': 1.0, 'loss_type': 'L2'}}}
    return sp, tp_, pred, tgt


# tap sets of the unused-parameter pin (tests/golden/reference_names.json unused_params, keyed "kind:taps")
UNUSED_PARAM_CASES = [([5, 8, 11], "after"), ([5, 8], "after"), ([2, 7], "after"), ([5, 8, 11], "in"), ([3, 9], "in")]


def unused_param_inputs():
    """An 8 x 8 latent and a context for the dummy backward of ldm_diffusers.py:123-141 (the set of parameters without
    gradient does not depend on the size)."""
    g = torch.Generator().manual_seed(1)
    return torch.rand((1, 4, 8, 8), generator=g), torch.rand((1, 77, 768), generator=g)


def train_palette(K):
    return [int(v) for v in torch.randint(0, 256, (K * 3,), generator=torch.Generator().manual_seed(99))]


def train_dropout_scales(B, C=256, p=0.1, n=3):
    """Injected Dropout2d keep-scales of the head calls in call order: source, target (student head), teacher."""
    g = torch.Generator().manual_seed(515)
    return [(torch.rand((B, C), generator=g) >= p).float() / (1.0 - p) for _ in range(n)]


def grad_probe(name, shape, seed=7):
    """Seeded unit-variance probe vector of a gradient tensor (its dot product is a checksum of the whole tensor)."""
    from madm_amd import weights
    return torch.randn(shape, generator=weights._gen(seed, "probe." + name))


def grad_summary(named_grads, full_max):
    """{name: grad} -> (names, [n, 2] f64 array of (l2 norm, probe dot), {name: full tensor for small ones})."""
    names, rows, full = [], [], {}
    for n, g in named_grads:
        g = g.detach().double().cpu()
        names.append(n)
        rows.append([g.norm().item(), (g * grad_probe(n, g.shape).double()).sum().item()])
        if g.numel() <= full_max and (".unet." not in n or (".lora_" in n and (".down_blocks.0.attentions.0." in n
                                                                              or ".mid_block." in n))):
            full[n] = g.float()
    return names, np.array(rows, dtype=np.float64), full
