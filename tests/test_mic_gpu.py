"""Masked image consistency (mic / mic_reg) on the device: the block-mask kernel bit for bit against the CPU restatement,
one full MIC training step against the fixtures of tests/golden/gen_golden_mic.py (the reference's head, criterion and
BlockMaskGenerator at B = 1), the trainer's gradient sink over three passes, the teacher side stream, and MIC off."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from golden_util import TRAIN_CASE, TIE_BAND, fixture_decision_margins, train_dropout_scales, grad_probe, load_golden
from util import rel_err
from test_train_gpu import build_product_train

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
    spec = importlib.util.spec_from_file_location("_gen_golden_mic", os.path.join(HERE, "golden", "gen_golden_mic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _batch(kind, B, H, W, g):
    x = torch.rand((B, 3, H, W), generator=g)
    return {"unit": x, "signed": 2 * x - 1, "byte": 255 * x, "out": 300 * x - 10}[kind]


@pytest.mark.parametrize("H,W", [(512, 512), (64, 64), (80, 112), (80, 50)])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_block_mask_kernel_is_bit_exact(cuda, B, H, W):
    from madm_amd import augment
    gm = _gen()
    g = torch.Generator().manual_seed(1000 * B + H + W)
    for kind in ("unit", "signed", "byte"):
        x = _batch(kind, B, H, W, g)
        u = torch.rand((B, 1) + augment.mask_grid_shape(H, W), generator=g)
        got, ud, flag = augment.block_mask(x.cuda(), 0.7, keep_u=u)
        want = gm.restated_mask_image(x, 0.7, u=u)
        assert torch.equal(got.cpu(), want), (kind, int((got.cpu() != want).sum()))
        assert int(flag.item()) == 0 and torch.equal(ud.cpu(), u)
        augment.check_mask_flag(flag)
    # the grid drawn from torch's default CPU generator, as the reference draws it
    x = _batch("unit", B, H, W, g)
    torch.manual_seed(3)
    got, ud, _ = augment.block_mask(x.cuda(), 0.7)
    torch.manual_seed(3)
    u = torch.rand(ud.shape)
    assert torch.equal(ud.cpu(), u) and torch.equal(got.cpu(), gm.restated_mask_image(x, 0.7, u=u))
    # outside [0, 255] and NaN: the reference asserts -> the flag is set, the host check raises, nothing faults
    nan = x.clone()
    nan[B - 1, 2, H - 1, W - 1] = float("nan")
    for bad in (_batch("out", B, H, W, g), nan):
        _, _, flag = augment.block_mask(bad.cuda(), 0.7)
        assert int(flag.item()) == 1
        with pytest.raises(AssertionError, match="outside"):
            augment.check_mask_flag(flag)
    torch.cuda.synchronize()


def build_mic(dtype, case, **kw):
    gm = _gen()
    c = gm.MIC_CASES[case]
    model = build_product_train(dtype, "train_depth", mic=c["mic"], mic_reg=c["mic_reg"], **kw)
    sc = train_dropout_scales(c["B"], n=4)           # source, target, teacher, masked
    model.sem_seg_head.dropout_scale_override = [sc[0], sc[1], sc[3]]
    model.ema_sem_seg_head.dropout_scale_override = [sc[2]]
    return model, gm


@pytest.mark.parametrize("case,dtype", [("train_depth_mic", torch.float32), ("train_depth_mic", torch.bfloat16),
                                        ("train_depth_mic", torch.float16), ("train_depth_mic_reg", torch.float32),
                                        ("train_depth_mic_b2", torch.float32)],
                         ids=["mic-f32", "mic-bf16", "mic-f16", "mic_reg-f32", "mic_b2-f32"])
def test_mic_train_step_matches_fixture(cuda, case, dtype):
    gold = load_golden(case)
    model, gm = build_mic(dtype, case)
    B = gm.MIC_CASES[case]["B"]
    gm.seed_step()
    losses = model(gm.mic_inputs(B))
    mic_key = "masked_prompt_consistency_loss" if gm.MIC_CASES[case]["mic"] else "mic_vae_decoder_loss"
    assert set(losses) == {"source_loss", "target_loss", "vae_decoder_source_loss", "vae_decoder_target_loss", mic_key}
    gscale = 1.0 if dtype == torch.float32 else 4096.0
    (sum(losses.values()) * gscale).backward()
    torch.cuda.synchronize()
    for p in model.parameters():
        if p.grad is not None:
            p.grad.div_(gscale)
    f32 = dtype == torch.float32
    gap, thr = fixture_decision_margins(gold, TRAIN_CASE["size"], TRAIN_CASE["pseudo_threshold"])
    assert float(gap.min()) > TIE_BAND and float(thr.min()) > TIE_BAND      # no teacher decision inside fp32 noise
    ltol = 1e-4 if f32 else (1e-2 if dtype == torch.float16 else 5e-2)
    rep = []
    for k, v in losses.items():
        ref = gold["loss_" + k].item()
        rep.append(f"{k} {v.item():.6f} / {ref:.6f}")
        assert abs(v.item() - ref) <= ltol * max(abs(ref), 1e-3), rep[-1]
    print(dtype, "; ".join(rep))
    ls = model.last_step
    assert set(ls) == {"mixed_img", "mixed_lbl", "mixed_seg_weight", "pseudo_label", "pseudo_weight", "ema_logits",
                       "source_logits", "target_logits", "masked_img", "mask_grid"} | \
        ({"masked_logits"} if gm.MIC_CASES[case]["mic"] else set())
    # masked image: the fill of the masked blocks bit for bit; the kept pixels carry the colour jitter, whose device kernels
    # match the kornia restatement to 2e-5 (tests/test_train_gpu.py::test_color_augmentation_kernels)
    got, want = ls["masked_img"].cpu(), gold["masked_img"]
    H = got.shape[-1]
    keep = torch.nn.functional.interpolate((ls["mask_grid"].cpu() > 0.7).float(), size=(H, H), mode="nearest").bool()
    keep = keep.expand_as(got)
    assert torch.equal(got[~keep], want[~keep]) and bool((got[~keep] == 0.5).all())
    assert float((got[keep] - want[keep]).abs().max()) < 2e-5
    if f32:
        assert torch.equal(ls["pseudo_label"].cpu().to(torch.uint8), gold["pseudo_label"])
        assert torch.equal(ls["mixed_lbl"].cpu().to(torch.uint8), gold["mixed_lbl"])
        assert abs(ls["pseudo_weight"].flatten()[0].item() - gold["pseudo_weight0"].item()) < 1e-6
    else:
        assert (ls["pseudo_label"].cpu().to(torch.uint8) == gold["pseudo_label"]).float().mean() > 0.9
    # every trainable tensor: |g| and the seeded probe checksum, with the gates of test_train_step_matches_fixture
    z = np.load(os.path.join(HERE, "golden", case + ".npz"))
    names, rows = str(z["grad_names"]).split("\n"), z["grad_rows"]
    params = dict(model.named_parameters())
    assert not [n for n in names if n not in params or params[n].grad is None]
    assert not [n for n, p in params.items() if p.requires_grad and p.grad is not None and n not in set(names)]
    ntol, ptol, mtol = {torch.float32: (2e-3, 8e-3, 1e-3), torch.float16: (4e-2, 3e-1, 6e-2),
                        torch.bfloat16: (8e-2, 1.2, 1.6e-1)}[dtype]
    typical = float(np.median(rows[:, 0][rows[:, 0] > 0]))
    errs = []
    for n, (norm, dot) in zip(names, rows):
        gd = params[n].grad.detach().double().cpu()
        gn = gd.norm().item()
        if norm < 1e-5 * typical:        # mathematically zero (q / k of the one-token mid-block attention at this size)
            assert gn < 1e-4 * typical, (n, gn, norm)
            continue
        errs.append((abs(gn - norm) / norm, abs((gd * grad_probe(n, gd.shape).double()).sum().item() - dot) / norm, n))
    med_p = sorted(e[1] for e in errs)[len(errs) // 2]
    worst = max(errs, key=lambda e: e[1])
    print(dtype, f"{len(errs)} gradient tensors: worst probe error {worst[1]:.2e} ({worst[2]}), median {med_p:.2e}")
    bad = [e for e in errs if e[0] > ntol or e[1] > ptol]
    assert not bad, sorted(bad, key=lambda e: -e[1])[:8]
    assert med_p < mtol, (med_p, mtol)
    for k in z.files:
        if k.startswith("grad:") and float(np.linalg.norm(z[k])) >= 1e-5 * typical:
            e = rel_err(params[k[5:]].grad.cpu(), torch.from_numpy(z[k]))[0]
            assert e < (1e-2 if f32 else (5e-1 if dtype == torch.float16 else 1.0)), (k, e)


def _trainer_step(model, gm, B, **kw):
    from madm_amd.train import MadmTrainer
    trainer = MadmTrainer(model, lr=0.0, weight_decay=0.0, grad_clip=None, amp=False, **kw)
    gm.seed_step()
    losses, _, stepped = trainer.run_step(gm.mic_inputs(B))
    torch.cuda.synchronize()
    assert stepped
    return trainer, losses


@pytest.mark.parametrize("case", ["train_depth_mic", "train_depth_mic_reg"])
def test_trainer_grad_sink_over_three_passes_matches_autograd(cuda, case):
    """MadmTrainer's flat gradient buffer (the sink: earlier passes accumulate, the last one finishes a span, what only the
    earlier passes touched is finished after the walk) against the plain autograd path of the same step."""
    model, gm = build_mic(torch.float32, case)
    B = gm.MIC_CASES[case]["B"]
    gm.seed_step()
    losses = model(gm.mic_inputs(B))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    plain = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    model.train_iter_index = 0
    sc = train_dropout_scales(B, n=4)
    model.sem_seg_head.dropout_scale_override = [sc[0], sc[1], sc[3]]
    model.ema_sem_seg_head.dropout_scale_override = [sc[2]]
    trainer, tl = _trainer_step(model, gm, B)
    for k, v in losses.items():
        assert abs(tl[k] - v.item()) <= 1e-6 * abs(v.item()), k
    seen = 0
    top = max(float(a.abs().max()) for a in plain.values())      # (a floor for the mathematically zero gradients)
    for n, p in model.named_parameters():
        if n not in plain:
            continue
        seen += 1
        a, b = plain[n], p.grad
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 1e-5 * scale + 1e-7 * top, (n, float((a - b).abs().max()), scale)
    assert seen == len(plain) > 700


def test_mic_teacher_side_stream_is_bit_identical(cuda):
    """MADM_TEACHER_OVERLAP=1: the masked pass runs before the main stream waits for the teacher; with lr = 0 the second
    step's losses and masked image are bit-identical to the step run in line."""
    out = {}
    for overlap in (False, True):
        model, gm = build_mic(torch.float32, "train_depth_mic_b2")
        model.overlap_teacher = overlap
        sc = train_dropout_scales(2, n=4)
        model.sem_seg_head.dropout_scale_override = [sc[0], sc[1], sc[3]] * 2
        model.ema_sem_seg_head.dropout_scale_override = [sc[2]] * 2
        from madm_amd.train import MadmTrainer
        trainer = MadmTrainer(model, lr=0.0, weight_decay=0.0, grad_clip=None, amp=False)
        rec = []
        for _ in range(2):         # the first step at a geometry runs in line either way
            gm.seed_step()
            losses, _, _ = trainer.run_step(gm.mic_inputs(2))
            rec.append((losses, model.last_step["masked_img"].clone(), model.last_step["pseudo_label"].clone()))
        torch.cuda.synchronize()
        assert (model._teacher_stream is not None) == overlap
        out[overlap] = rec
        del model, trainer
    for (la, ma, pa), (lb, mb, pb) in zip(out[False], out[True]):
        assert la == lb and torch.equal(ma, mb) and torch.equal(pa, pb)


def test_mic_off_changes_nothing(cuda):
    """MIC off (every shipped configuration): the same loss names and last_step keys as before, no third pass."""
    model = build_product_train(torch.float32, "train_depth")
    sc = train_dropout_scales(TRAIN_CASE["B"])
    model.sem_seg_head.dropout_scale_override = [sc[0], sc[1]]
    model.ema_sem_seg_head.dropout_scale_override = [sc[2]]
    from golden_util import train_inputs
    random.seed(TRAIN_CASE["py_seed"])
    np.random.seed(TRAIN_CASE["np_seed"])
    losses = model(train_inputs(**TRAIN_CASE))
    assert set(losses) == {"source_loss", "target_loss", "vae_decoder_source_loss", "vae_decoder_target_loss"}
    assert set(model.last_step) == {"mixed_img", "mixed_lbl", "mixed_seg_weight", "pseudo_label", "pseudo_weight",
                                    "ema_logits", "source_logits", "target_logits"}
    assert not model.mic and not model.mic_reg
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    gold = load_golden("train_depth")
    for k, v in losses.items():
        assert abs(v.item() - gold["loss_" + k].item()) <= 1e-4 * abs(gold["loss_" + k].item()), k
