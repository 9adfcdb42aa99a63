"""The evaluator's exports on the GPU: the pack kernel (csrc/eval_export.hip) byte for byte against the numpy restatement
of its layout and against files PIL wrote from the reference's statements (tests/golden/eval_export_pil.npz),
``DSECSemSegEvaluator`` under several streams with a small ring, the sheet mode against ``vis.compose``, and
``inference_on_dataset`` end to end on the DEPTH eval model."""
import os
import threading

import numpy as np
import pytest
import torch

from eval_export_util import DELIVER_PALETTE, DIRS, fixture, pack_ref, planes_ref, read_png

pytestmark = pytest.mark.gpu

K19 = 19
PALETTE19 = np.random.default_rng(19).integers(0, 256, 3 * K19).tolist()


def _pack_case(H, W, seed, u8):
    rng = np.random.default_rng(seed)
    image = (rng.random((3, H, W)) * 255.0).astype(np.float32)
    probes = (0.4, 254.999, 255.0, 0.0, 0.999, 1.0)
    flat = image.reshape(-1)
    flat[:min(len(probes), flat.size)] = probes[:flat.size]          # truncation, not rounding (d2_evaluator.py:170)
    if u8:
        image = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    pred = rng.integers(0, K19, (H, W)).astype(np.int64)
    pred.reshape(-1)[-1] = K19 - 1
    gt = rng.integers(0, K19, (H, W)).astype(np.int64)
    gt[: max(1, H // 8)] = 255                                          # ignored rows
    gt[H // 2, W // 3:] = 255
    return image, pred, gt


def _run_pack(image, pred, gt, palette, num_classes, offset=0):
    from madm_amd import ops, labels
    H, W = pred.shape
    n = ops.eval_export_pack_bytes(H, W)
    big = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda")    # an unwritten byte shows, and so does one too many
    out = big[offset:offset + n]
    assert out.data_ptr() % 4 == offset % 4
    pal = labels._device_palette(list(palette), out.device)
    ops.eval_export_pack(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(image).cuda(), pal,
                         num_classes, 255, out=out)
    got = big.cpu().numpy()
    assert (got[:offset] == 0xAA).all() and (got[offset + n:] == 0xAA).all(), "bytes outside the buffer were written"
    return got[offset:offset + n]


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (64, 3), (97, 131), (33, 256), (512, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_kernel_is_byte_exact(cuda, shape):
    H, W = shape
    for u8 in (False, True):
        image, pred, gt = _pack_case(H, W, 100 * H + W, u8)
        want = pack_ref(image, pred, gt, PALETTE19, K19, 255)
        got = _run_pack(image, pred, gt, PALETTE19, K19)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"u8={u8}: {bad.size} bytes differ, first at {bad[:4]} (got {got[bad[:4]]}, want {want[bad[:4]]})"
        # the 16-bit samples are big-endian: the high byte (0) first, the class id second
        row0 = got[H * (1 + 3 * W):][:1 + 2 * W]
        assert row0[0] == 0 and (row0[1::2] == 0).all() and np.array_equal(row0[2::2], pred[0].astype(np.uint8))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_pack_kernel_at_an_unaligned_offset(cuda, offset):
    image, pred, gt = _pack_case(97, 131, 7, False)
    want = pack_ref(image, pred, gt, PALETTE19, K19, 255)
    assert np.array_equal(_run_pack(image, pred, gt, PALETTE19, K19, offset=offset), want)
    image, pred, gt = _pack_case(1, 1, 8, True)                         # 15 bytes: shorter than the aligned part may be
    assert np.array_equal(_run_pack(image, pred, gt, PALETTE19, K19, offset=offset), pack_ref(image, pred, gt, PALETTE19, K19, 255))


def test_pack_kernel_reproduces_the_pil_fixture(cuda):
    from madm_amd import eval_export
    fx = fixture()
    pred = fx["pred_in"]
    H, W = pred.shape
    got = _run_pack(fx["image_in"], pred, fx["gt_in"], fx["palette"].tolist(), int(fx["num_classes"]), offset=1)
    for d, (off, n), (_d, depth, colour, bpp) in zip(DIRS, eval_export.plane_slices(H, W), eval_export.PLANES):
        rows = got[off:off + n].reshape(H, 1 + bpp * W)
        assert not rows[:, 0].any() and (depth, colour) == tuple(fx[d + "_ihdr"].tolist()), d
        body = np.ascontiguousarray(rows[:, 1:])
        a = body.view(">u2").astype(np.uint16).reshape(H, W) if depth == 16 else body.reshape(H, W, 3)
        assert np.array_equal(a, fx[d]), d


def _evaluator(out, **kw):
    from madm_amd.evaluation import DSECSemSegEvaluator
    args = dict(dataset_name="DS", stuff_classes=[f"c{i}" for i in range(11)], palette=DELIVER_PALETTE, ignore_label=255,
                output_dir=None if out is None else str(out), save_predictions_json=False)
    args.update(kw)
    return DSECSemSegEvaluator(**args)


def _synthetic(n=5):
    """n (data, outputs) pairs of two sizes with synthetic logits, as test_device_evaluator_is_bit_exact draws them."""
    g = torch.Generator().manual_seed(55)
    out = []
    for i in range(n):
        H, W = (97, 131) if i % 2 == 0 else (64, 48)
        logits = torch.randn((1, 11, H, W), generator=g)
        logits[0, 2, 5, 5] = logits[0, 9, 5, 5] = 50.0                  # tie -> first maximal class
        gt = torch.randint(0, 11, (1, H, W), generator=g)
        gt[0, :7] = 255
        image = 255.0 * torch.rand((3, H, W), generator=g)
        if i % 2:
            image = image.to(torch.uint8)
        out.append((dict(target_second_modality=image.cuda() if i % 3 else image, target_label=gt), logits))
    return out


def test_evaluator_exports_every_image_under_streams(cuda, tmp_path, monkeypatch):
    from madm_amd.evaluation import SemSegEvaluator
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    cases = _synthetic()
    ev = _evaluator(tmp_path, save_eval_results_step=1, eval_only=True, export_workers=2, export_depth=2)
    plain = SemSegEvaluator(11, ignore_label=255)
    ev.reset()
    streams = [torch.cuda.Stream() for _ in range(4)]
    dev_logits = [l.cuda() for _d, l in cases]
    torch.cuda.synchronize()
    for i, (data, _l) in enumerate(cases):
        with torch.cuda.stream(streams[i % 4]):
            ev.process([data], [{"sem_seg": dev_logits[i]}])
    res = ev.evaluate()                                                   # waits for the files
    st = ev.exporter.stats
    assert st["images"] == 5 and st["files"] == 20 and st["encode_ms"] > 0 and st["stalls"] >= 0
    for i, (data, logits) in enumerate(cases):
        plain.process([data], [{"sem_seg": dev_logits[i]}])
        pred = logits[0].argmax(dim=0).numpy()
        want = planes_ref(data["target_second_modality"].cpu().numpy(), pred, data["target_label"][0].numpy(),
                          DELIVER_PALETTE, 11, 255)
        for d, a in zip(DIRS, want):
            got, _ihdr = read_png(tmp_path / d / f"{i:06d}_rank0.png")
            assert got.shape == a.shape and np.array_equal(got, a), (i, d)
    for d in DIRS:
        assert sorted(os.listdir(tmp_path / d)) == [f"{i:06d}_rank0.png" for i in range(5)]
    assert np.array_equal(ev.confusion(), plain.confusion())
    assert res["default"]["sem_seg_default"]["DS/mIoU"] == plain.evaluate()["sem_seg"]["mIoU"]
    assert os.path.exists(tmp_path / "sem_seg_default_evaluation.pth")
    ev.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("madm-eval-export")]


def test_sheet_mode_equals_vis_compose(cuda, tmp_path, monkeypatch):
    from madm_amd import vis
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    cases = _synthetic()
    cases[2][0]["pred_save_name"] = "named.png"
    ev = _evaluator(tmp_path, save_eval_results_step=2, export_workers=2, export_depth=2)
    ev.reset()
    for data, logits in cases:
        ev.process([data], [{"sem_seg": logits.cuda()}])
    ev.evaluate()
    pngs = sorted(n for n in os.listdir(tmp_path) if n.endswith(".png"))
    assert pngs == ["000000_rank0.png", "000004_rank0.png", "named.png"]
    for i, name in ((0, pngs[0]), (2, "named.png"), (4, pngs[1])):
        data, logits = cases[i]
        H, W = logits.shape[-2:]
        pred = logits[0].argmax(dim=0)
        gt = data["target_label"][0].clone()
        gt[gt == 255] = 11
        tiles = [dict(data_type="image", info="image", data=data["target_second_modality"].cuda()[None].float(),
                      denorm=(1.0 / 255.0, 0.0)),
                 dict(data_type="label", info="pred", data=pred[None].cuda()),
                 dict(data_type="label", info="gt", data=gt[None].cuda())]
        want = vis.compose(tiles, cols_max=3, palette=DELIVER_PALETTE).cpu().numpy()
        got, ihdr = read_png(tmp_path / name)
        assert ihdr == (8, 2) and got.shape == (H, 3 * W, 3) and np.array_equal(got, want), name
        assert not got[:7, 2 * W:].any()                                  # the ignored rows of the gt tile are black
    ev.close()


def _build_depth_model():
    """tests/test_eval_gpu.py::_build_product("DEPTH", f16), by the same recipe."""
    from golden_util import init_eval_params
    from madm_amd.ldm_rocm import LdmRocm
    from madm_amd.backbone import BasePromptTimeGenerator, AttentionFeatureExtractorBackbone
    from madm_amd.head import DAFormerHead
    from madm_amd.meta_arch import MadmInference
    from oracle import madm_path
    cfg = madm_path.cfg_by_name("DEPTH")
    ldm = LdmRocm("", encoder_block_indices=[], unet_block_indices=[5, 8, 11], decoder_block_indices=(),
                  input_range='-1+1', unet_block_indices_type='after', finetune_unet='no', compute_dtype=torch.float16,
                  weights='synthetic', seed=0, vae_decoder_loss=cfg["vae_decoder_loss"])
    gen = BasePromptTimeGenerator(learnable_cond_prompt=True, learnable_cond_time=True, clip_state='no', num_timesteps=1,
                                  clip_model_name="ViT-L-14-336", ldm_extractor=ldm, same_cond_params=True)
    backbone = AttentionFeatureExtractorBackbone(
        attention_features_res=None, feature_dims=list(cfg["feature_dims"]), projection_dim=list(cfg["projection_dim"]),
        attention_features_location=None, feature_extractor=gen, num_res_blocks=1, out_features=list(cfg["out_features"]))
    n = len(cfg["out_features"])
    head = DAFormerHead(in_channels=list(cfg["head_in_channels"]), in_keys=list(cfg["out_features"]), in_index=list(range(n)),
                        channels=256, dropout_ratio=0.1, num_classes=cfg["num_classes"], norm_cfg=dict(type='BN'),
                        align_corners=False, decoder_params=madm_path.head_decoder_params())
    init_eval_params(backbone, head)
    return MadmInference(backbone.cuda(), head.cuda(), target_modality="Depth").eval()


def test_inference_on_dataset_exports_end_to_end(cuda, tmp_path, monkeypatch):
    from madm_amd import ops
    from madm_amd.evaluation import inference_on_dataset
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    model = _build_depth_model()
    g = torch.Generator().manual_seed(77)
    loader = []
    for i in range(5):
        H, W = (512, 512) if i != 2 else (448, 512)
        img = 255.0 * torch.rand((3, H, W), generator=g)
        if i % 2:
            img = img.to(torch.uint8)
        loader.append([{"target_second_modality": img.cuda() if i % 3 else img,
                        "target_label": torch.randint(0, 11, (1, H, W), generator=g)}])
    ev = _evaluator(tmp_path / "on", save_eval_results_step=1, eval_only=True)
    res = inference_on_dataset(model, loader, ev)
    off = _evaluator(None)
    res_off = inference_on_dataset(model, loader, off)
    assert off.exporter is None and np.array_equal(ev.confusion(), off.confusion())
    on_m, off_m = res["default"]["sem_seg_default"], res_off["default"]["sem_seg_default"]
    assert list(on_m) == list(off_m) and "DS/mIoU" in on_m
    assert all(on_m[k] == off_m[k] or (np.isnan(on_m[k]) and np.isnan(off_m[k])) for k in on_m)
    for i, inputs in enumerate(loader):
        with ops.tuning_profile("throughput", pin=True):     # the rows the runner's graphs were captured under
            sem = model(inputs)[0]["sem_seg"]
        want = sem[0].argmax(dim=0).cpu().numpy()
        got, ihdr = read_png(tmp_path / "on" / "pred" / f"{i:06d}_rank0.png")
        assert ihdr == (16, 0) and got.shape == want.shape and np.array_equal(got, want), i
        img = read_png(tmp_path / "on" / "image" / f"{i:06d}_rank0.png")[0]
        assert np.array_equal(img, planes_ref(inputs[0]["target_second_modality"].cpu().numpy(), want, want, DELIVER_PALETTE,
                                              11, 255)[0]), i
    for d in DIRS:
        assert sorted(os.listdir(tmp_path / "on" / d)) == [f"{i:06d}_rank0.png" for i in range(5)]
    ev.close()
    # the deferred range assert still fires, and nothing of the exporter outlives the call
    bad = [{"target_second_modality": loader[0][0]["target_second_modality"] * 1.01 + 1.0,
            "target_label": loader[0][0]["target_label"]}]
    ev = _evaluator(tmp_path / "bad", save_eval_results_step=1, eval_only=True)
    with pytest.raises(AssertionError, match="input range check"):
        inference_on_dataset(model, [loader[0], bad, loader[3], loader[4]], ev)
    assert ev.exporter is None
    assert not [t for t in threading.enumerate() if t.name.startswith("madm-eval-export")]
    left = [os.path.join(r, n) for r, _d, names in os.walk(tmp_path / "bad") for n in names if n.endswith(".tmp")]
    assert not left, left
