"""Generates the masked-image-consistency fixtures (mic / mic_reg, /root/reference/modeling/meta_arch/mtmadise.py:404-420,
:471-488).  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): one training step of the shipped Depth flags at
64 x 64 through ``OracleMicMTMADISE`` -- oracle/train_path.OracleMTMADISE plus a restatement of the MIC branch -- with the
REFERENCE's DAFormerHead, its CmdiseCriterion (which holds both MIC terms) and, at B = 1, its own
``BlockMaskGenerator.mask_image`` (utils/dacs_transforms.py:136-166, loaded by path under an inert kornia stub).  The
reference raises for B > 1 (mask_image indexes the batch with a [B*B, C, H, W] mask; the masked CE hands a batch of one
label to a B-image prediction), so train_depth_mic_b2.npz is built with the restated mask and criterion terms (one mask
per image, per-image pseudo labels): the port's deliberate extension.

    python tests/golden/gen_golden_mic.py        # writes tests/golden/train_depth_mic*.npz and mic_pins.npz
"""
import importlib.util
import os
import random
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import train_path, labels as OL, ldm_path, augment as OA  # noqa: E402
from golden_util import TRAIN_CASE  # noqa: E402

REF_DACS = "/root/reference/utils/dacs_transforms.py"

# TRAIN_CASE geometry.  The teacher's BatchNorm statistics (and so its decisions) depend on the batch, so the margins of the
# B = 1 batch were checked again (main() prints them): smallest top-2 probability gap / distance to the threshold 1.5e-5 /
# 3.8e-5 at B = 1 (input seed 8908, the first image of TRAIN_CASE's batch), 1.8e-5 / 2.1e-5 at B = 2 -- 10 x TIE_BAND
MIC_CASES = {
    "train_depth_mic": dict(B=1, mic=True, mic_reg=False),
    "train_depth_mic_reg": dict(B=1, mic=False, mic_reg=1.0),
    "train_depth_mic_b2": dict(B=2, mic=True, mic_reg=False),
}
MIC_SEEDS = dict(torch_seed=20242, input_seed_b1=8908, mask_ratio=0.7, full_grad_max_numel=4096)


def reference_block_mask_generator():
    """The REFERENCE's own BlockMaskGenerator (this container only): dacs_transforms.py imports kornia at module level,
    which is not installed and not used by the mask; an inert module stands in for it while the file loads."""
    saved = sys.modules.get("kornia")
    sys.modules["kornia"] = types.ModuleType("kornia")
    try:
        spec = importlib.util.spec_from_file_location("_madm_ref_dacs", REF_DACS)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            sys.modules.pop("kornia", None)
        else:
            sys.modules["kornia"] = saved
    return mod.BlockMaskGenerator


def restated_mask_image(imgs, mask_ratio, mask_block_size=32, u=None):
    """mask_image with one mask per image, broadcast over channels (what the reference means; equal to it at B = 1)."""
    B, _, H, W = imgs.shape
    if u is None:
        u = torch.rand((B, 1, round(H / mask_block_size), round(W / mask_block_size)))
    keep = F.interpolate((u > mask_ratio).float(), size=(H, W), mode='nearest').expand_as(imgs)
    lo, hi = torch.min(imgs), torch.max(imgs)
    out = imgs.clone()
    if 0 <= lo <= hi <= 1:
        out[keep == 0] = 0.5
    elif -1 <= lo <= hi <= 1:
        out = out * keep
    else:
        assert 0 <= lo <= hi <= 255
        out[keep == 0] = 127.5
    return out


def restated_mic_losses(targets, loss_weight=1.0):
    """CmdiseCriterion's two MIC terms (criterion.py:211-218, 247-253) with per-image labels ``label`` [B, 1, H, W]."""
    losses = {}
    if 'masked_prompt_consistency' in targets:
        e = targets['masked_prompt_consistency']
        pred = F.interpolate(e['pred'], size=e['label'].shape[-2:], mode='bilinear', align_corners=False)
        losses['masked_prompt_consistency_loss'] = loss_weight * train_path.CmdiseCriterionRestated.cross_entropy(
            pred, e['label'][:, 0], pixel_weight=e['pixel_weight'])
    if 'mic_decoder_loss' in targets:
        e = targets['mic_decoder_loss']
        f = F.l1_loss if e['loss_type'] == 'L1' else F.mse_loss
        losses['mic_vae_decoder_loss'] = f(e['pred'], e['gt']) * e['pixel_weight'] * e['loss_weight']
    return losses


class MicCriterionRestated(train_path.CmdiseCriterionRestated):
    def forward(self, outputs, targets, **kwargs):
        losses = super().forward(outputs, targets)
        losses.update(restated_mic_losses(targets, self.loss_weight))
        return losses


def oracle_strong_color(param, data):
    """strong_transform(param, data) with mix None and colour augmentation on (dacs_transforms.py:11-25): torch draws the
    jitter factors, numpy the blur sigma -- the order of the product (madm_amd.augment.strong_color)."""
    from madm_amd import augment
    if param['color_jitter'] > param['color_jitter_p']:
        data = torch.stack([OA.color_jitter_image(data[i], *augment.jitter_params(param['color_jitter_s']))
                            for i in range(data.shape[0])])
    if param['blur'] > 0.5:
        sigma = np.random.uniform(0.15, 1.15)
        H, W = data.shape[-2:]
        data = OA.gaussian_blur(data, augment.blur_kernel_size(H), augment.blur_kernel_size(W), sigma)
    return data


class _Capture(torch.nn.Module):
    """Stands in for the criterion inside OracleMTMADISE.forward_train: records its arguments, returns no loss."""

    def forward(self, loss_input, loss_target):
        self.args = (loss_input, loss_target)
        return {}


class OracleMicMTMADISE(train_path.OracleMTMADISE):
    """OracleMTMADISE + the MIC branch (mtmadise.py:404-420, 343-348, 471-488).  The parent's step runs first with its
    criterion call captured; the masked pass follows -- after the teacher, as in the reference, so the random draws keep
    their order (torch jitter factors, numpy blur sigma, torch mask grid) -- and the criterion then sees every target at
    once.  ``mask_fn(imgs)``: the reference's mask_image (B = 1) or restated_mask_image; ``per_image_label``: the masked CE
    gets pseudo_label[:, None] (B > 1) instead of the reference's pseudo_label[None]."""

    def __init__(self, *a, mic=False, mic_reg=False, mask_ratio=0.7, MIC_reg_wo_pl_val=False, mask_fn=None,
                 per_image_label=False, **kw):
        super().__init__(*a, **kw)
        assert not (mic and mic_reg)
        self.mic, self.mic_reg, self.MIC_reg_wo_pl_val = mic, mic_reg, MIC_reg_wo_pl_val
        self.mask_ratio = mask_ratio
        self.mask_fn = mask_fn or (lambda imgs: restated_mask_image(imgs, self.mask_ratio))
        self.per_image_label = per_image_label

    def forward_train(self, batched_inputs):
        st = random.getstate()                     # the parent's two uniforms (mtmadise.py:217-225), read ahead
        cj = random.uniform(0, 1)
        bl = random.uniform(0, 1) if self.blur else 0
        random.setstate(st)
        crit, cap = self.criterion, _Capture()
        self.criterion = cap
        # the reference draws the UNet timesteps with torch.randint(..., device=...) from the DEVICE's generator; on the CPU
        # that draw would advance the CPU generator that the masked image's jitter factors and mask grid come from, so the
        # oracle hands the parent step the CPU generator's state and restores it afterwards
        rng = torch.random.get_rng_state()
        try:
            losses = super().forward_train(batched_inputs)
        finally:
            self.criterion = crit
            torch.random.set_rng_state(rng)
        loss_input, loss_target = cap.args
        ls = self.last_step
        pseudo_label, pseudo_weight = ls['pseudo_label'], ls['pseudo_weight']
        target = train_path.tp.ImageList.from_tensors([(x['target_second_modality'] - 0.0) / 255.0 for x in batched_inputs],
                                                      64).tensor
        strong_parameters = {'mix': None, 'color_jitter': cj, 'color_jitter_s': self.color_jitter_strength,
                             'color_jitter_p': self.color_jitter_probability, 'blur': bl, 'mean': None, 'std': None}
        with torch.no_grad():
            if self.mic_reg:                                                  # :343-345 (teacher block)
                pl_color, _ = OL.convert_label_to_rgb(pseudo_label[:, None], self.reg_target_palette)
                pl_color_latent = ldm_path.vae_encoder(self.backbone.feature_extractor.ldm_extractor.vae, pl_color, [])[0]
            pseudo_val = float(pseudo_weight.flatten()[0])                    # :346-348 (sum(...).item() / size)
            masked_img = oracle_strong_color(strong_parameters, target.clone())      # :405-406
            masked_img = self.mask_fn(masked_img)                                    # :408
        self.set_lora_adapter(state=self.target_modality)                    # :409
        if self.mic:
            masked_pred = self.sem_seg_head_sec_modal(self.backbone(masked_img, input_modal='others'))
            loss_target['masked_prompt_consistency'] = {                      # :471-476
                'pred': masked_pred, 'label': pseudo_label[:, None] if self.per_image_label else pseudo_label[None],
                'pixel_weight': pseudo_weight}
        else:
            _, masked_out = self.backbone(masked_img, return_unet_final_output=True, input_modal='others')
            loss_target['mic_decoder_loss'] = {                               # :477-488
                'pred': masked_out['before_vae.decoder'], 'gt': pl_color_latent,
                'pixel_weight': 1.0 if self.MIC_reg_wo_pl_val else pseudo_val, 'loss_weight': self.mic_reg,
                'loss_type': self.vae_decoder_loss_type}
        out = self.criterion(loss_input, loss_target)
        out.update(losses)                                                    # (zero_grad, when on)
        ls['masked_img'] = masked_img
        if self.mic:
            ls['masked_logits'] = masked_pred
        return out


def build(case, reference=True):
    """The MIC oracle of ``case`` on the build_train_oracle recipe (tests/golden/gen_golden.py); ``reference``: the
    reference's DAFormerHead, CmdiseCriterion and (B = 1) BlockMaskGenerator, else the restatements."""
    spec = importlib.util.spec_from_file_location("_gen_golden", os.path.join(HERE, "gen_golden.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    from golden_util import train_dropout_scales
    c = MIC_CASES[case]
    base = gg.build_train_oracle(reference=reference, variant="train_depth")
    ref = reference and c["B"] == 1
    if ref:
        gen = reference_block_mask_generator()(MIC_SEEDS["mask_ratio"], 32)
        mask_fn = gen.mask_image
    else:
        mask_fn = None
    crit = base.criterion if ref else MicCriterionRestated(loss_weight=1.0)
    base.__class__ = OracleMicMTMADISE
    base.criterion = crit
    base.mic, base.mic_reg, base.MIC_reg_wo_pl_val = c["mic"], c["mic_reg"], False
    base.mask_ratio = MIC_SEEDS["mask_ratio"]
    base.mask_fn = mask_fn or (lambda imgs: restated_mask_image(imgs, base.mask_ratio))
    base.per_image_label = c["B"] > 1
    sc = train_dropout_scales(c["B"], n=4)       # source, target, teacher, masked
    base.sem_seg_head.dropout.scales = [sc[0], sc[1], sc[3]]
    base.ema_sem_seg_head.dropout.scales = [sc[2]]
    return base


def mic_inputs(B):
    from golden_util import train_inputs
    case = dict(TRAIN_CASE, B=B)
    if B == 1:
        case["input_seed"] = MIC_SEEDS["input_seed_b1"]
    return train_inputs(**case)


def seed_step():
    random.seed(TRAIN_CASE["py_seed"])
    np.random.seed(TRAIN_CASE["np_seed"])
    torch.manual_seed(MIC_SEEDS["torch_seed"])


def run_step(model, B):
    from golden_util import grad_summary
    seed_step()
    losses = model.forward_train(mic_inputs(B))
    sum(losses.values()).backward()
    named = [(n, p.grad) for n, p in model.named_parameters() if p.requires_grad and p.grad is not None]
    names, rows, full = grad_summary(named, MIC_SEEDS["full_grad_max_numel"])
    out = {"loss_" + k: np.array(v.item(), dtype=np.float64) for k, v in losses.items()}
    out["grad_names"] = np.array("\n".join(names))
    out["grad_rows"] = rows
    for n, g in full.items():
        out["grad:" + n] = g.numpy()
    ls = model.last_step
    out["mixed_lbl"] = ls["mixed_lbl"].to(torch.uint8).numpy()
    out["pseudo_label"] = ls["pseudo_label"].to(torch.uint8).numpy()
    out["pseudo_weight0"] = np.array(ls["pseudo_weight"].flatten()[0].item())
    out["mixed_seg_weight"] = ls["mixed_seg_weight"].numpy()
    out["ema_logits"] = ls["ema_logits"].detach().numpy()
    out["masked_img"] = ls["masked_img"].detach().numpy()
    return out


def main():
    torch.set_num_threads(os.cpu_count())
    from golden_util import TIE_BAND, fixture_decision_margins
    for case, c in MIC_CASES.items():
        if sys.argv[1:] and case not in sys.argv[1:]:
            continue
        t0 = time.time()
        out = run_step(build(case, reference=True), c["B"])
        gap, thr = fixture_decision_margins({"ema_logits": torch.from_numpy(out["ema_logits"])}, TRAIN_CASE["size"],
                                            TRAIN_CASE["pseudo_threshold"])
        np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
        print(f"{case}: {time.time() - t0:.1f}s", {k: float(v) for k, v in out.items() if k.startswith("loss_")},
              len(out["grad_rows"]), f"gradient tensors; margins {gap.min().item():.2e} / {thr.min().item():.2e} "
              f"(band {TIE_BAND:g})")
    if not sys.argv[1:] or "pins" in sys.argv[1:]:
        main_pins()


def pin_inputs():
    """Seeded batches of the mask / criterion pins: one per range branch of mask_image, B = 1."""
    g = torch.Generator().manual_seed(77)
    imgs = {"unit": torch.rand((1, 3, 80, 112), generator=g), "signed": 2 * torch.rand((1, 3, 64, 64), generator=g) - 1,
            "byte": 255 * torch.rand((1, 3, 96, 48), generator=g)}
    K = 11
    pred = torch.randn((1, K, 16, 16), generator=g)
    label = torch.randint(0, K, (1, 64, 64), generator=g)
    label[torch.rand((1, 64, 64), generator=g) < 0.05] = 255
    weight = torch.full((1, 64, 64), 0.37)
    dec_pred, dec_gt = torch.randn((1, 4, 8, 8), generator=g), torch.randn((1, 4, 8, 8), generator=g)
    return imgs, pred, label, weight, dec_pred, dec_gt


def main_pins():
    """The reference's mask_image on the three range branches (the grid drawn from torch's seeded default generator) and
    its CmdiseCriterion's two MIC terms on seeded predictions -> mic_pins.npz."""
    BMG = reference_block_mask_generator()
    imgs, pred, label, weight, dec_pred, dec_gt = pin_inputs()
    out = {}
    for k, x in imgs.items():
        torch.manual_seed(5)
        out["mask_" + k] = BMG(0.7, 32).mask_image(x.clone()).numpy()
    crit = train_path.reference_criterion()(loss_weight=1.0)
    sp = torch.zeros((1, K_PIN, 16, 16))
    base_t = {'source_gt': torch.zeros((1, 1, 64, 64), dtype=torch.long), 'target_pl': torch.zeros((1, 1, 64, 64), dtype=torch.long),
              'target_pw': torch.ones((1, 64, 64))}
    for lt in ("L1", "L2"):
        t = dict(base_t, masked_prompt_consistency={'pred': pred, 'label': label[None], 'pixel_weight': weight},
                 mic_decoder_loss={'pred': dec_pred, 'gt': dec_gt, 'pixel_weight': 0.37, 'loss_weight': 2.0, 'loss_type': lt})
        losses = crit({'source_rgb_pred': sp, 'target_sec_modal_pred': sp}, t)
        out["masked_ce"] = np.array(losses['masked_prompt_consistency_loss'].item())
        out["mic_dec_" + lt] = np.array(losses['mic_vae_decoder_loss'].item())
    np.savez_compressed(os.path.join(HERE, "mic_pins.npz"), **out)
    print("mic_pins.npz", {k: getattr(v, "shape", v) for k, v in out.items()})


K_PIN = 11

if __name__ == "__main__":
    main()
