"""Masked image consistency (mic / mic_reg) on the host: the restated mask and MIC loss terms of
tests/golden/gen_golden_mic.py against the reference values recorded in tests/golden/mic_pins.npz, the all-oracle MIC
training step against the three MIC fixtures, and the option contract of MTMADISE."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen():
    spec = importlib.util.spec_from_file_location("_gen_golden_mic", os.path.join(HERE, "golden", "gen_golden_mic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restated_mask_and_mic_terms_reproduce_the_reference():
    gm = _gen()
    z = np.load(os.path.join(HERE, "golden", "mic_pins.npz"))
    imgs, pred, label, weight, dec_pred, dec_gt = gm.pin_inputs()
    for k, x in imgs.items():                 # one batch per range branch: 0.5 fill, x * 0, 127.5 fill
        torch.manual_seed(5)
        got = gm.restated_mask_image(x.clone(), 0.7, 32)
        assert np.array_equal(got.numpy(), z["mask_" + k]), k
    for lt in ("L1", "L2"):
        t = {'masked_prompt_consistency': {'pred': pred, 'label': label[:, None], 'pixel_weight': weight},
             'mic_decoder_loss': {'pred': dec_pred, 'gt': dec_gt, 'pixel_weight': 0.37, 'loss_weight': 2.0, 'loss_type': lt}}
        losses = gm.restated_mic_losses(t)
        assert abs(losses['masked_prompt_consistency_loss'].item() - float(z["masked_ce"])) <= 1e-6 * float(z["masked_ce"])
        assert abs(losses['mic_vae_decoder_loss'].item() - float(z["mic_dec_" + lt])) <= 1e-6 * float(z["mic_dec_" + lt])


@pytest.mark.parametrize("case", ["train_depth_mic", "train_depth_mic_reg", "train_depth_mic_b2"])
def test_mic_oracle_step_reproduces_the_fixture(case):
    """The all-oracle build (OracleHead, restated criterion and mask) reproduces the fixture that the reference's head,
    criterion and (B = 1) BlockMaskGenerator produced: losses, labels, the masked image and every gradient checksum."""
    gm = _gen()
    out = gm.run_step(gm.build(case, reference=False), gm.MIC_CASES[case]["B"])
    z = np.load(os.path.join(HERE, "golden", case + ".npz"))
    names = {k for k in z.files if k.startswith("loss_")}
    assert names == {k for k in out if k.startswith("loss_")}
    assert ("loss_masked_prompt_consistency_loss" in names) == gm.MIC_CASES[case]["mic"]
    assert ("loss_mic_vae_decoder_loss" in names) == bool(gm.MIC_CASES[case]["mic_reg"])
    for k in names:
        assert abs(float(out[k]) - float(z[k])) <= 1e-6 * max(1.0, abs(float(z[k]))), k
    assert np.array_equal(out["pseudo_label"], z["pseudo_label"]) and np.array_equal(out["mixed_lbl"], z["mixed_lbl"])
    assert np.array_equal(out["masked_img"], z["masked_img"])
    want = dict(zip(str(z["grad_names"]).split("\n"), z["grad_rows"]))
    got = dict(zip(str(out["grad_names"]).split("\n"), out["grad_rows"]))
    assert set(want) == set(got)
    nz = z["grad_rows"][:, 0]
    tiny = 1e-5 * float(np.median(nz[nz > 0]))
    # mathematically zero gradients (q / k of the mid block's one-token self-attention at 64 x 64) are summation noise of
    # ~1e-8 in both builds: bounded absolutely, everything else relatively
    zero = {n for n in want if want[n][0] < tiny}
    assert all(got[n][0] < tiny for n in zero) and len(zero) < 8, zero
    worst = max(np.max(np.abs(got[n] - want[n])) / want[n][0] for n in want if n not in zero)
    assert worst < 1e-4, worst


def _model(**kw):
    from madm_amd.mtmadise import MTMADISE
    from madm_amd.criterion import CmdiseCriterion
    bb = torch.nn.Module()        # construction reads the modules the EMA teacher copies
    bb.feature_projections = torch.nn.Linear(2, 2)
    fe = bb.feature_extractor = torch.nn.Module()
    fe.clip_project_others = torch.nn.Linear(2, 2)
    fe.ldm_extractor = torch.nn.Module()
    return MTMADISE(bb, torch.nn.Linear(2, 2), CmdiseCriterion(num_classes=11), target_modality="Depth",
                    train_palette=[0, 0, 0], **kw)


def test_mtmadise_accepts_the_mic_options():
    m = _model(mic=True)
    assert m.mic and not m.mic_reg and m.mask_ratio == 0.7 and m.mask_block_size == 32
    m = _model(mic=True, mask_ratio=0.5)
    assert m.mask_ratio == 0.5
    m = _model(mic_reg=1.0, MIC_reg_wo_pl_val=True)
    assert m.mic_reg == 1.0 and not m.mic and m.MIC_reg_wo_pl_val
    m = _model()
    assert not m.mic and not m.mic_reg
    with pytest.raises(AssertionError):
        _model(mic=True, mic_reg=1.0)
    with pytest.raises(NotImplementedError):
        _model(mic=True, mask_diff=True)
    with pytest.raises(NotImplementedError):
        _model(mic=True, sem_seg_head_sec_modal=True)


def test_mask_grid_shape_uses_bankers_rounding():
    from madm_amd import augment
    assert augment.mask_grid_shape(512, 512) == (16, 16)
    assert augment.mask_grid_shape(80, 112) == (2, 4)          # round(2.5) == 2, round(3.5) == 4
    assert augment.mask_grid_shape(64, 96) == (2, 3)
