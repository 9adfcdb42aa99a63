"""GPU tests of the periodic training picture: ``madm_vis_compose`` (csrc/vis.hip) against a numpy / torch-CPU restatement
written here -- every tile kind bit-exact, the in-kernel bilinear resize of low-resolution logits, the sheet composition --
and the dump of ``MTMADISE`` end to end (file == device canvas == recomposition from ``last_step``), its asynchronous safety
and that switching it off changes nothing."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import TRAIN_CASE, train_inputs
from test_vis_host import decode_png

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------- the restatement (include/madm_hip.h)
def _to_byte(v01):
    """(int)floorf(fmaf(255, v, 0.5f)) for f32 v in [0, 1]: the product is exact in f64 and so is the sum wherever it can
    reach the next integer, so one rounding to f32 -- the fma's."""
    return np.floor((255.0 * v01.astype(np.float64) + 0.5).astype(np.float32)).astype(np.uint8)


def _clip01(v):
    v = np.where(np.isnan(v), np.float32(0), v).astype(np.float32)
    return np.minimum(np.maximum(v, np.float32(0)), np.float32(1))


def ref_image(x, scale=0.5, shift=0.5):
    """f32 [B, 3, H, W] -> u8 [B, H, W, 3]"""
    x = x.numpy().astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * np.float32(scale) + np.float32(shift)          # two f32 roundings
    return _to_byte(_clip01(v)).transpose(0, 2, 3, 1)


def ref_label(lab, palette):
    pal = np.asarray(list(palette) + [0] * (768 - len(palette)), dtype=np.uint8).reshape(256, 3)
    return pal[(lab.numpy() & 255)]


def ref_logits(x, palette):
    return ref_label(torch.argmax(x, dim=1), palette)           # the first maximal class


def ref_heat(x):
    v = _clip01(x.numpy().astype(np.float32))
    t = (np.float32(255) * v).astype(np.int32)
    u = t.astype(np.float32) / np.float32(255)
    u4 = np.float32(4) * u
    ch = [_to_byte(_clip01(np.float32(1.5) - np.abs(u4 - np.float32(k)))) for k in (3, 2, 1)]
    return np.stack(ch, axis=-1)


REF = {"image": lambda t, pal: ref_image(t["data"], *t.get("denorm", (0.5, 0.5))), "label": lambda t, pal: ref_label(t["data"], pal),
       "logits": lambda t, pal: ref_logits(t["data"], pal), "heatmap": lambda t, pal: ref_heat(t["data"])}


def ref_sheet(tiles, cols_max, palette, H, W):
    """The whole sheet from per-tile pictures u8 [B, H, W, 3]: background 255 (cmdise.py:250,261)."""
    from madm_amd import vis
    B = tiles[0]["data"].shape[0]
    rows, cols, cells = vis.layout(len(tiles), B, cols_max)
    sheet = np.full((rows * H, cols * W, 3), 255, dtype=np.uint8)
    for i, t in enumerate(tiles):
        pic = REF[t["data_type"]](t, palette)
        for j in range(B):
            r, c = cells[i][j]
            sheet[r * H:(r + 1) * H, c * W:(c + 1) * W] = pic[j]
    return sheet


def on_device(tiles):
    return [dict(t, data=t["data"].cuda()) for t in tiles]


def make_tiles(B, H, W, K, seed):
    g = torch.Generator().manual_seed(seed)
    img = 1.6 * torch.randn((B, 3, H, W), generator=g)          # well outside [-1, 1] after the denorm
    img[0, 1, 3, 5] = float("nan")
    img[-1, 2, H - 1, W - 1] = float("inf")
    img[-1, 0, 0, 0] = float("-inf")
    img01 = torch.rand((B, 3, H, W), generator=g) * 1.4 - 0.2
    lab = torch.randint(0, K, (B, H, W), generator=g)
    lab[torch.rand((B, H, W), generator=g) < 0.1] = 255
    lab[0, 0, 1] = 256 + 3                                        # wraps like astype(uint8)
    logits = torch.randn((B, K, H, W), generator=g)
    logits[:, 2, ::3, ::5] = logits[:, 6, ::3, ::5] = 9.0         # exact ties: the first maximal class wins
    heat = torch.rand((B, H, W), generator=g) * 1.5 - 0.25
    heat[0, 2, 2] = float("nan")
    heat[0, 2, 3], heat[0, 2, 4] = 1.0, 0.0
    return [dict(data_type="image", info="img", data=img), dict(data_type="label", info="lab", data=lab),
            dict(data_type="logits", info="logits", data=logits), dict(data_type="heatmap", info="heat", data=heat),
            dict(data_type="image", info="img01", data=img01, denorm=(1.0, 0.0)),
            dict(data_type="label", info="lab4", data=lab[:, None].clone()),
            dict(data_type="heatmap", info="heat_grid", data=(torch.arange(B * H * W).reshape(B, H, W) % 256).float() / 255.0)]


def palette_for(K, seed=99):
    return [int(v) for v in torch.randint(1, 256, (K * 3,), generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize("H,W,K", [(64, 64, 11), (48, 50, 9)], ids=["64x64-K11", "48x50-K9"])
def test_every_tile_kind_is_bit_exact(cuda, H, W, K):
    """One tile per sheet (n = 1: a B x 1 sheet).  48 x 50: the row pitch 150 is no multiple of 4 and W no multiple of the 4
    pixels a thread writes."""
    from madm_amd import vis
    pal = palette_for(K)
    tiles = make_tiles(2, H, W, K, seed=H * W + K)
    for t, td in zip(tiles, on_device(tiles)):
        got = vis.compose([td], 5, pal).cpu().numpy()
        assert got.shape == (2 * H, W, 3) and got.dtype == np.uint8
        want = ref_sheet([t], 5, pal, H, W)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (t["info"], len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
    # the scalar properties the recipe promises
    img = ref_image(tiles[0]["data"])
    assert img[0, 3, 5, 1] == 0 and img[-1, H - 1, W - 1, 2] == 255 and img[-1, 0, 0, 0] == 0      # NaN, +inf, -inf
    assert (ref_label(tiles[1]["data"], pal)[tiles[1]["data"].numpy() == 255] == 0).all()                   # 255: black
    heat = ref_heat(tiles[3]["data"])
    assert tuple(heat[0, 2, 2]) == (0, 0, 128) and tuple(heat[0, 2, 3]) == (128, 0, 0)


def test_shapes_that_do_not_fit_are_refused(cuda):
    from madm_amd import vis
    from madm_amd._lib import MadmHipError
    pal = palette_for(4)
    img = torch.zeros((1, 3, 16, 16), device="cuda")
    with pytest.raises(MadmHipError, match="only logits"):
        vis.compose([dict(data_type="image", info="a", data=img),
                     dict(data_type="label", info="b", data=torch.zeros((1, 8, 8), dtype=torch.int64, device="cuda"))], 5, pal)
    with pytest.raises(ValueError, match="tiles"):
        vis.compose([dict(data_type="image", info="a", data=img)] * 17, 5, pal)
    with pytest.raises(ValueError):
        vis.compose([dict(data_type="attention_maps", info="a", data=img)], 5, pal)


def test_low_resolution_logits_on_the_integer_lattice(cuda):
    """Integer logits in [-8, 8] at 16 x 16 -> 64 x 64: every bilinear weight is a multiple of 1/8, every product and sum a
    multiple of 1/64 below 2^4 -- exact in f32 whatever the order, so F.interpolate on the CPU is THE answer, the ~1 % exactly
    tied pixels included (the first maximal class)."""
    from madm_amd import vis
    B, K, h, H = 2, 11, 16, 64
    pal = palette_for(K)
    g = torch.Generator().manual_seed(4242)
    x = torch.randint(-8, 9, (B, K, h, h), generator=g).float()
    up = F.interpolate(x, size=(H, H), mode="bilinear", align_corners=False)
    top2 = up.topk(2, dim=1).values
    ties = float((top2[:, 0] == top2[:, 1]).float().mean())
    print(f"lattice: {100 * ties:.2f} % exactly tied pixels")
    assert ties > 0.002
    anchor = dict(data_type="label", info="anchor", data=torch.zeros((B, H, H), dtype=torch.int64, device="cuda"))
    got = vis.compose([anchor, dict(data_type="logits", info="x", data=x.cuda())], 5, pal).cpu().numpy()
    want = ref_label(up.argmax(dim=1), pal)
    for j in range(B):
        assert np.array_equal(got[j * H:(j + 1) * H, H:], want[j])


def test_low_resolution_logits_float_case(cuda):
    """Seeded randn at (24, 20) -> (48, 50).  Reference: F.interpolate in f64 on the CPU.  The class must agree wherever the
    f64 top-2 margin is at least 1e-4 (f32 evaluation order moves a value by ~1e-7 of its magnitude: three decades below);
    pixels under that margin may be at most 0.1 % of all."""
    from madm_amd import vis
    B, K, h, w, H, W = 2, 9, 24, 20, 48, 50
    pal = palette_for(K)
    x = torch.randn((B, K, h, w), generator=torch.Generator().manual_seed(777))
    up = F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=False)
    top2 = up.topk(2, dim=1).values
    close = ((top2[:, 0] - top2[:, 1]) < 1e-4).numpy()
    share = close.mean()
    print(f"float case: {100 * share:.4f} % of the pixels have an f64 top-2 margin below 1e-4")
    assert share <= 1e-3
    anchor = dict(data_type="heatmap", info="anchor", data=torch.zeros((B, H, W), device="cuda"))
    got = vis.compose([anchor, dict(data_type="logits", info="x", data=x.cuda())], 5, pal).cpu().numpy()
    want = ref_label(up.argmax(dim=1), pal)
    for j in range(B):
        diff = (got[j * H:(j + 1) * H, W:] != want[j]).any(axis=-1)
        assert not (diff & ~close[j]).any(), int((diff & ~close[j]).sum())


def test_composition_of_a_ragged_sheet(cuda):
    """n = 7 at cols_max 5, B = 2: a 4 x 5 sheet whose second row of every image has three blank cells.  The canvas is handed in
    pre-filled with 0x5A: every byte must be written -- the blanks 255 -- and every tile lands in its rectangle only."""
    from madm_amd import vis
    B, H, W, K = 2, 48, 50, 9
    pal = palette_for(K)
    tiles = make_tiles(B, H, W, K, seed=5)
    g = torch.Generator().manual_seed(6)
    tiles[2] = dict(data_type="logits", info="low", data=torch.randint(-8, 9, (B, K, 12, 25), generator=g).float())
    assert len(tiles) == 7
    canvas = torch.full((4 * H, 5 * W, 3), 0x5A, dtype=torch.uint8, device="cuda")
    out = vis.compose(on_device(tiles), 5, pal, out=canvas)
    assert out.data_ptr() == canvas.data_ptr()
    got = out.cpu().numpy()
    ref_tiles = list(tiles)
    up = F.interpolate(tiles[2]["data"], size=(H, W), mode="bilinear", align_corners=False)   # exact: weights k/4 and k/8... / 2^n
    ref_tiles[2] = dict(tiles[2], data=up)
    want = ref_sheet(ref_tiles, 5, pal, H, W)
    for r in (1, 3):
        assert (got[r * H:(r + 1) * H, 2 * W:] == 255).all(), "blank cells are white"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4])
    # the same tiles on a narrower sheet (cols_max 3: rows of 3, 3, 1)
    got3 = vis.compose(on_device(tiles), 3, pal).cpu().numpy()
    assert got3.shape == (B * 3 * H, 3 * W, 3) and np.array_equal(got3, ref_sheet(ref_tiles, 3, pal, H, W))


def test_submit_is_safe_against_later_writes(cuda, tmp_path):
    """``submit`` returns with the sheet composed in stream order: overwriting every source in place right after it, on the
    same stream, must not reach the file."""
    from madm_amd import vis
    B, H, W, K = 2, 64, 64, 11
    pal = palette_for(K)
    tiles = make_tiles(B, H, W, K, seed=8)
    dev = on_device(tiles)
    want = ref_sheet(tiles, 5, pal, H, W)
    w = vis.VisWriter(tmp_path, async_write=True)
    canvas = w.submit(250, dev, cols_max=5, palette=pal)
    for t in dev:
        t["data"].zero_()
    w.wait()
    assert np.array_equal(decode_png(open(w.path(250), "rb").read()), want)
    assert np.array_equal(canvas.cpu().numpy(), want)
    side = json.load(open(w.path(250, "json")))
    assert [t["info"] for t in side["tiles"]] == [t["info"] for t in tiles] and side["tile_size"] == [H, W]
    # the canvas is kept and reused; in line the same code runs
    w2 = vis.VisWriter(tmp_path / "inline", async_write=False)
    dev = on_device(tiles)
    c1 = w2.submit(1, dev, cols_max=5, palette=pal)
    assert os.path.exists(w2.path(1)) and w2._thread is None
    c2 = w2.submit(2, dev, cols_max=5, palette=pal)
    assert c1.data_ptr() == c2.data_ptr()
    assert open(w2.path(1), "rb").read() == open(w2.path(2), "rb").read() == open(w.path(250), "rb").read()


# ---------------------------------------------------------------------------------- MTMADISE
def _seed():
    random.seed(TRAIN_CASE["py_seed"])
    np.random.seed(TRAIN_CASE["np_seed"])
    torch.manual_seed(31)


def _rect(sheet, meta, info, j):
    t = next(t for t in meta["tiles"] if t["info"].startswith(info))
    x, y, w, h = t["rects"][j]
    return sheet[y:y + h, x:x + w]


def test_dump_end_to_end(cuda, tmp_path):
    """The small train model, f32, vis_period = 2, the writer on its thread, two steps: exactly one picture and one sidecar; the file is the device canvas
    ``last_vis`` keeps; the tiles that show what the step trained on are a recomposition from ``last_step``."""
    from madm_amd import vis
    from test_train_gpu import build_product_train
    model = build_product_train(torch.float32, vis_period=2, output_dir=str(tmp_path), vis_async=True)
    assert model.vis_writer is not None and model.last_vis is None
    _seed()
    data = train_inputs(**TRAIN_CASE)
    for _ in range(2):
        losses = model(data)
    assert all(torch.isfinite(v) for v in losses.values())
    model.vis_writer.wait()
    d = tmp_path / "vis_results"
    assert sorted(p.name for p in d.iterdir()) == ["000002_rank0.json", "000002_rank0.png"]
    lv, ls = model.last_vis, model.last_step
    assert lv["iteration"] == 2 and lv["path"] == str(d / "000002_rank0.png")
    sheet = decode_png(open(lv["path"], "rb").read())
    assert np.array_equal(sheet, lv["canvas"].cpu().numpy())
    side = json.load(open(d / "000002_rank0.json"))
    infos = [t["info"] for t in side["tiles"]]
    # mtmadise.py:559-601 + the picture-only pass (:603-621): 'st' decoder losses, reg_uncertain, rev_noise_sup before its end
    assert len(infos) == 15 and infos[:4] == ["source_rgb", "source_pred", "source_label", "target_sec_modal"], infos
    t_ = int(infos[4][len("target_sec_modal_pl_"):-len("_t")])            # the teacher's timestep of THIS step (:556-557)
    assert infos[4] == f"target_sec_modal_pl_{t_}_t" and t_ in (int(60 * (1 - 1 / 5000)), int(61 * (1 - 1 / 5000)))
    assert infos[5:12] == ["mixup_modal", "mixup_pred", "mixup_label", "source_vae_decoder_out", "target_vae_decoder_out",
                           "pl_reg", "pl_prob_reg"] and infos[13:] == ["no_noise_t_reg", "no_noise_t_pred"], infos
    # the share of confident pixels in the title is formatted on the writer thread from a device scalar
    assert infos[12] == "pl_prob_{:.3f}".format(float(ls["pseudo_weight"].reshape(-1)[-1])) and lv["infos"][12] == "pl_prob_{:.3f}"
    assert [t["kind"] for t in side["tiles"]] == ["image", "logits", "label", "image", "label", "image", "logits", "label",
                                                  "image", "image", "logits", "heatmap", "heatmap", "image", "logits"]
    B, S = TRAIN_CASE["B"], TRAIN_CASE["size"]
    assert side["tile_size"] == [S, S] and (side["rows"], side["cols"]) == (B * 3, 5) and sheet.shape == (B * 3 * S, 5 * S, 3)
    pal = model.train_palette
    for info, tile in (("mixup_label", dict(data_type="label", data=ls["mixed_lbl"])),
                       ("mixup_modal", dict(data_type="image", data=ls["mixed_img"])),
                       ("target_sec_modal_pl", dict(data_type="label", data=ls["pseudo_label"]))):
        again = vis.compose([dict(tile, info=info)], 5, pal, denorm=model.vis_denorm).cpu().numpy()
        for j in range(B):
            assert np.array_equal(_rect(sheet, side, info, j), again[j * S:(j + 1) * S]), (info, j)
    # ... and against the restatement, from host copies
    assert np.array_equal(_rect(sheet, side, "mixup_label", 1), ref_label(ls["mixed_lbl"][:, 0].cpu(), pal)[1])
    assert np.array_equal(_rect(sheet, side, "mixup_modal", 0), ref_image(ls["mixed_img"].cpu())[0])
    assert (sheet[:, :, :] != 255).any() and (_rect(sheet, side, "no_noise_t_pred", 0) != 255).any()


def test_off_changes_nothing(cuda, tmp_path):
    """vis_period=None and a vis_period beyond the run: losses, what the step hands on and every generator state are
    bit-identical to a model built without the arguments (f32, two optimizer-free steps with lr = 0)."""
    from madm_amd.train import MadmTrainer
    from madm_amd import ldm_rocm
    from test_train_gpu import build_product_train
    keys = ("ema_logits", "pseudo_label", "pseudo_weight", "mixed_lbl", "mixed_img")
    runs = []
    for kw in (dict(), dict(vis_period=None, output_dir=str(tmp_path)), dict(vis_period=1000, output_dir=str(tmp_path))):
        model = build_product_train(torch.float32, **kw)
        trainer = MadmTrainer(model, lr=0.0, weight_decay=0.0, grad_clip=None, amp=False)
        _seed()
        torch.cuda.manual_seed(32)
        ldm_rocm._const_cache.clear()
        ldm_rocm._noise_cache.clear()
        rec = []
        for i in range(2):
            data = train_inputs(**dict(TRAIN_CASE, input_seed=TRAIN_CASE["input_seed"] + i))
            losses, _norm, _stepped = trainer.run_step(data)
            rec.append((dict(losses), {k: model.last_step[k].detach().clone() for k in keys}))
        torch.cuda.synchronize()
        gens = (random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
                torch.get_rng_state().numpy().tobytes(), torch.cuda.get_rng_state().cpu().numpy().tobytes())
        runs.append((rec, gens))
        assert model.last_vis is None
        assert (model.vis_writer is None) == (not kw.get("vis_period"))
        if model.vis_writer is not None:
            assert model.vis_writer.canvas is None and model.vis_writer._thread is None
        del model, trainer
        torch.cuda.empty_cache()
    assert not (tmp_path / "vis_results").exists()
    (base, base_gens) = runs[0]
    for rec, gens in runs[1:]:
        assert gens == base_gens
        for (la, ta), (lb, tb) in zip(base, rec):
            assert la == lb, (la, lb)
            for k in keys:
                assert torch.equal(ta[k], tb[k]), k
