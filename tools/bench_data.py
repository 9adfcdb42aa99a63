#!/usr/bin/env python3
"""What the device-side dataset pipeline (madm_amd/data.py) delivers, on synthetic PNG files of the shipped sizes written
with the project's own encoder (vis.encode_png / eval_export.encode_png_rows):

  Cityscapes source   2048 x 1024 RGB + gray label -> resize 1024 x 512 -> crop 512 x 512
  DELIVER target      1024 x 1024 RGB 'depth' + RGBA label -> train: resize 712 x 712, crop 512 x 512; test: resize 512 x 512

Reported, one JSON line:
  train_samples_per_s   the train loader alone (one sample = source image + source label + target image)
  test_images_per_s     the test loader alone (image + label)
  eval                  ``inference_on_dataset`` on the DEPTH eval model fed by the test loader, and the same call fed by the same
                        samples as pre-built device tensors, same process, interleaved; ``ratio`` = loader-fed / pre-built (best
                        steady rates).  Nothing is gated.

    python tools/bench_data.py [--files 16] [--images 64] [--workers 4] [--json profiles/data_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SKIP = 8


def _photo(rng, h, w):
    """Photo-like rather than white noise (inflate's cost depends on it): a smooth field + a little noise, uint8 [h, w, 3]."""
    low = torch.from_numpy(rng.rand(1, 3, h // 32, w // 32).astype(np.float32)) * 255.0
    img = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0]
    img = (img + 4.0 * torch.from_numpy(rng.randn(3, h, w).astype(np.float32))).clamp_(0.0, 255.0)
    return img.permute(1, 2, 0).to(torch.uint8).contiguous().numpy()


def _classes(rng, h, w, n, block=32):
    return rng.randint(0, n, size=(h // block, w // block)).astype(np.uint8).repeat(block, 0).repeat(block, 1)


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def _rows(a):
    """uint8 [H, W] or [H, W, C] -> PNG scanlines with filter byte 0."""
    h = a.shape[0]
    raw = np.zeros((h, 1 + a[0].size), dtype=np.uint8)
    raw[:, 1:] = a.reshape(h, -1)
    return raw


def write_tree(root, files, images):
    from madm_amd.eval_export import encode_png_rows
    from madm_amd.vis import encode_png
    rng = np.random.RandomState(4242)
    src, tgt = os.path.join(root, "cityscapes"), os.path.join(root, "deliver") + os.sep
    js = {"source_data": {"RGB": [], "label": []}, "target_data": {"second_modality": [], "label": []}}
    for i in range(files):
        rgb, lab = f"leftImg8bit/train/c/{i}.png", f"gtFine/train/c/{i}_labelIds.png"
        _write(os.path.join(src, rgb), encode_png(_photo(rng, 1024, 2048)))
        _write(os.path.join(src, lab), encode_png_rows(_rows(_classes(rng, 1024, 2048, 34)), 2048, 1024, 8, 0))
        js["source_data"]["RGB"].append(rgb)
        js["source_data"]["label"].append(lab)
        d, l = f"depth/cloud/test/MAP/{i}_depth_front.png", f"semantic/cloud/test/MAP/{i}_semantic_front.png"
        _write(os.path.join(tgt, d), encode_png(_photo(rng, 1024, 1024)))
        cls = _classes(rng, 1024, 1024, 12)
        cls[cls == 0] = 255
        rgba = np.stack([cls, cls, cls, np.full_like(cls, 255)], axis=2)
        _write(os.path.join(tgt, l), encode_png_rows(_rows(rgba), 1024, 1024, 8, 6))
        js["target_data"]["second_modality"].append(d)
        js["target_data"]["label"].append(l)
    # the evaluation set: ``images`` entries over the same files
    js["target_data"]["second_modality"] = [js["target_data"]["second_modality"][i % files] for i in range(images)]
    js["target_data"]["label"] = [js["target_data"]["label"][i % files] for i in range(images)]
    json_path = os.path.join(root, "Cityscapes_RGB_to_DELIVER_Depth.json")
    with open(json_path, "w") as f:
        json.dump(js, f)
    return json_path, src, tgt


class TimedLoader:
    def __init__(self, items):
        self.items, self.t = items, []

    def __iter__(self):
        self.t = []
        for it in self.items:
            self.t.append(time.perf_counter())
            yield it


def loader_rate(it, n, warm):
    for _ in range(warm):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        batch = next(it)
    del batch
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def eval_run(model, items):
    from madm_amd.evaluation import SemSegEvaluator, inference_on_dataset
    ev = SemSegEvaluator(11, ignore_label=255)
    loader = TimedLoader(items)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = inference_on_dataset(model, loader, ev)
    t1 = time.perf_counter()
    n = len(loader.t)
    return dict(whole_images_per_s=round(n / (t1 - t0), 2), steady_images_per_s=round((n - SKIP) / (t1 - loader.t[SKIP]), 2),
                mIoU=float(res["sem_seg"]["mIoU"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=16, help="distinct files written per kind")
    ap.add_argument("--images", type=int, default=64, help="length of the evaluation set (entries repeat the files)")
    ap.add_argument("--train-batches", type=int, default=24)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--no-eval", action="store_true", help="the loaders' own rates only (no model)")
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()
    assert args.images > SKIP + 8
    from madm_amd import data
    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    base = tempfile.mkdtemp(prefix="bench_data_")
    result = dict(tool="bench_data", files=args.files, images=args.images, workers=args.workers, dtype=args.dtype,
                  cpus=len(os.sched_getaffinity(0)))
    try:
        t0 = time.perf_counter()
        json_path, src, tgt = write_tree(base, args.files, args.images)
        result["write_tree_s"] = round(time.perf_counter() - t0, 2)
        train = data.CrossModalityDataset(json_path, src, tgt, source_resize_h_w=[512, 1024], source_crop_size_h_w=[512, 512],
                                          target_resize_h_w=[712, 712], target_crop_size_h_w=[512, 512], train_or_test="train")
        tl = data.build_train_loader(train, local_batch_size=2, num_workers=args.workers, seed=0, prefetch=2)
        result["train_samples_per_s"] = round(2 * max(loader_rate(tl, args.train_batches, 2 if r == 0 else 0)
                                                      for r in range(args.repeats)), 2)
        tl.close()
        test = data.CrossModalityDataset(json_path, src, tgt, test_resize_h_w=[512, 512], train_or_test="test")
        el = data.build_test_loader(test, num_workers=args.workers, prefetch=4)
        rates = []
        for _ in range(args.repeats):
            it = iter(el)
            rates.append(loader_rate(it, args.images - 4, 4))
            for _rest in it:
                pass
        result["test_images_per_s"] = round(max(rates), 2)
        if not args.no_eval:
            import bench
            dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
            model = bench.build_eval_model(dtype, device)
            prebuilt = [[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in s[0].items()}] for s in el]
            torch.cuda.synchronize()
            eval_run(model, prebuilt)                                   # warm-up, untimed
            runs = {"prebuilt": [], "loader": []}
            for rep in range(args.repeats):                             # interleaved: drift hits both
                for name, items in (("prebuilt", prebuilt), ("loader", el)):
                    row = eval_run(model, items)
                    runs[name].append(row)
                    print(f"# {name} #{rep}: {row}", flush=True)
            assert len({repr(r["mIoU"]) for v in runs.values() for r in v}) == 1, "the loader changed the metrics"
            best = {k: max(r["steady_images_per_s"] for r in v) for k, v in runs.items()}
            result["eval"] = dict(runs=runs, best_steady_images_per_s=best, ratio=round(best["loader"] / best["prebuilt"], 4))
        el.close()
    finally:
        shutil.rmtree(base, ignore_errors=True)
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
