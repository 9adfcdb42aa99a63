#!/usr/bin/env python3
"""What the evaluator's exports cost the pipelined eval loop: ``inference_on_dataset`` over N seeded synthetic 512 x 512
images on the DEPTH eval model (bench.py's), three configurations in ONE process on one box --

  off        DSECSemSegEvaluator without an output directory (the default path),
  sheet10    one ``image | pred | gt`` sheet for every 10th image (what the shipped configs do during training),
  eval_only  the four files for every image (the README's eval command),

each run ``--repeats`` times after one untimed warm-up call.  Per run two rates: ``whole`` = N / the time of the whole call
(graph capture of the call's runner included) and ``steady`` = (N - 8) / the time from the loader handing out image 8 to the
call's return (capture excluded; the drain and the wait for the last files included).  The ratios to ``off`` use the best
steady rate of each configuration.  Boxes differ by a few percent, so nothing here is comparable across boxes.

    python tools/eval_export_bench.py [--images 64] [--workers 6] [--json profiles/eval_export_bench.json]
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

import torch  # noqa: E402

PALETTE = [70, 130, 180, 70, 70, 70, 190, 153, 153, 220, 20, 60, 153, 153, 153, 128, 64, 128, 244, 35, 232,
           107, 142, 35, 0, 0, 142, 102, 102, 156, 250, 170, 30]
NAMES = ['sky', 'building', 'fence', 'person', 'pole', 'road', 'sidewalk', 'vegetation', 'car', 'wall', 'traffic sign']
SKIP = 8


def make_images(n, size, device):
    """Photo-like rather than white noise (zlib's cost depends on it): a smooth field + a little sensor noise, in [0, 255];
    labels in 16 x 16 blocks with some ignored."""
    g = torch.Generator().manual_seed(4242)
    out = []
    for _ in range(n):
        low = 255.0 * torch.rand((1, 3, size // 16, size // 16), generator=g)
        img = torch.nn.functional.interpolate(low, size=(size, size), mode="bicubic", align_corners=False)[0]
        img = (img + 4.0 * torch.randn((3, size, size), generator=g)).clamp_(0.0, 255.0)
        lab = torch.randint(0, 12, (1, size // 16, size // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
        lab[lab == 11] = 255
        out.append([{"target_second_modality": img.to(device), "target_label": lab.to(device)}])
    return out


class TimedLoader:
    def __init__(self, items):
        self.items, self.t = items, []

    def __iter__(self):
        self.t = []
        for it in self.items:
            self.t.append(time.perf_counter())
            yield it


def evaluator(out_dir, step, eval_only, workers):
    from madm_amd.evaluation import DSECSemSegEvaluator
    return DSECSemSegEvaluator(dataset_name="synthetic", stuff_classes=NAMES, palette=PALETTE, ignore_label=255,
                               output_dir=out_dir, save_predictions_json=False, save_eval_results_step=step,
                               eval_only=eval_only, export_workers=workers)


def one_run(model, items, ev):
    from madm_amd.evaluation import inference_on_dataset
    loader = TimedLoader(items)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = inference_on_dataset(model, loader, ev)
    t1 = time.perf_counter()
    n = len(items)
    row = dict(whole_images_per_s=round(n / (t1 - t0), 2), steady_images_per_s=round((n - SKIP) / (t1 - loader.t[SKIP]), 2),
               mIoU=float(res["default"]["sem_seg_default"]["synthetic/mIoU"]))
    if ev.exporter is not None:
        row["stats"] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in ev.exporter.stats.items()}
    ev.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", type=int, default=6, help="export_workers of the evaluator")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--out-dir", default=None, help="parent of the (temporary) output directories; default: the system's "
                                                     "temporary directory, i.e. local disk")
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()
    assert args.images > SKIP + 8
    import bench
    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    model = bench.build_eval_model(dtype, device)
    items = make_images(args.images, args.size, device)
    model(items[0])
    torch.cuda.synchronize()
    base = tempfile.mkdtemp(prefix="eval_export_bench_", dir=args.out_dir)
    configs = [("off", None, -1, False), ("sheet10", "sheet10", 10, False), ("eval_only", "eval_only", 1, True)]
    result = dict(tool="eval_export_bench", images=args.images, size=args.size, dtype=args.dtype, workers=args.workers,
                  cpus=len(os.sched_getaffinity(0)), runs={})
    try:
        one_run(model, items, evaluator(None, -1, False, args.workers))                 # warm-up, untimed
        for rep in range(args.repeats):
            for name, sub, step, eval_only in configs:                                    # interleaved: drift hits all three
                out = None if sub is None else os.path.join(base, f"{sub}_{rep}")
                row = one_run(model, items, evaluator(out, step, eval_only, args.workers))
                if out is not None:
                    files = sum(len(f) for _r, _d, f in os.walk(out))
                    size = sum(os.path.getsize(os.path.join(r, n)) for r, _d, f in os.walk(out) for n in f)
                    row.update(files=files, megabytes=round(size / 1e6, 2))
                result["runs"].setdefault(name, []).append(row)
                print(f"# {name} #{rep}: {row}", flush=True)
    finally:
        shutil.rmtree(base, ignore_errors=True)
    best = {k: max(r["steady_images_per_s"] for r in v) for k, v in result["runs"].items()}
    result["best_steady_images_per_s"] = best
    result["ratio_to_off"] = {k: round(best[k] / best["off"], 4) for k in best if k != "off"}
    assert len({repr(r["mIoU"]) for v in result["runs"].values() for r in v}) == 1, "the exports changed the metrics"
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
