#!/usr/bin/env python3
"""What the periodic training picture (vis_period, madm_amd/vis.py) costs the training loop, on the bench's training graph
(bench_mic.build: configs[3], 512 x 512, bs 2, the shipped 'st' tile set with reg_uncertain and rev_noise_sup: 15 tiles).

One process runs ONE mode and prints one JSON line: ``--steps`` MadmTrainer steps, each synchronised, with one dump inside
the middle step --

  none        no dump (vis_period off): the baseline.  ``--root DIR`` imports the package from another checkout (the parent
              commit, built there), so the same tool measures "steps without a dump" on both sides
  async       MTMADISE's dump with the writer thread (vis_async=True)
  sync        the same code in line (vis_async=False)
  comparator  the reference's approach in line, built here: per logits tile F.interpolate + softmax + max, ``.cpu()`` of
              every tile, numpy palette / denorm, paste, PNG encoding, write (cmdise.py:238-305 without matplotlib)

-- and reports, for the dump: the host time of the call and the event bracket on the training stream, both WITHOUT the
reference's extra picture-only teacher pass, and that pass on its own; for the run: wall time, median / max step.

``--alternate N`` is the driver: N rounds of fresh child processes in the order ``--modes`` gives (default
baseline,none,async,comparator; ``baseline`` = none at ``--baseline-root``), then a summary: per mode the walls of its
processes, the baseline's process-to-process spread, and async's training-thread cost against the comparator's.
Usage: python tools/bench_vis.py --alternate 3 --baseline-root /path/to/parent [--dtype f16] [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


class HostComparator:
    """Stands in for ``model.vis_writer``: the same tiles, drawn the reference's way on the training thread."""

    def __init__(self, out_dir):
        self.out_dir, self.canvas, self.last_host_ms = out_dir, None, None

    def path(self, iteration, ext="png"):
        return os.path.join(self.out_dir, "vis_results", f"{int(iteration):06d}_cmp.{ext}")

    def wait(self):
        pass

    def submit(self, iteration, tiles, cols_max=5, palette=None, denorm=(0.5, 0.5)):
        import numpy as np
        import torch
        import torch.nn.functional as F
        from madm_amd import vis
        t0 = time.perf_counter()
        pal = np.asarray(list(palette) + [0] * (768 - len(palette)), dtype=np.uint8).reshape(256, 3)
        B, (H, W) = tiles[0]["data"].shape[0], tiles[0]["data"].shape[-2:]
        rows, cols, cells = vis.layout(len(tiles), B, cols_max)
        sheet = np.full((rows * H, cols * W, 3), 255, dtype=np.uint8)
        for i, t in enumerate(tiles):
            d = t["data"]
            if t["data_type"] == "logits":
                if tuple(d.shape[-2:]) != (H, W):
                    d = F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False)
                d = torch.softmax(d, dim=1).max(dim=1)[1]
            d = d.cpu().numpy()
            if t["data_type"] in ("logits", "label"):
                pic = pal[d.reshape(B, H, W) & 255]
            elif t["data_type"] == "image":
                sc, sh = t.get("denorm", denorm)
                pic = (np.clip(d * sc + sh, 0, 1) * 255 + 0.5).astype(np.uint8).transpose(0, 2, 3, 1)
            else:
                u = (np.clip(d.reshape(B, H, W), 0, 1) * 255).astype(np.uint8) / np.float32(255)
                pic = np.stack([np.clip(1.5 - np.abs(4 * u - k), 0, 1) * 255 + 0.5 for k in (3, 2, 1)], -1).astype(np.uint8)
            for j in range(B):
                r, c = cells[i][j]
                sheet[r * H:(r + 1) * H, c * W:(c + 1) * W] = pic[j]
        os.makedirs(os.path.dirname(self.path(iteration)), exist_ok=True)
        with open(self.path(iteration), "wb") as f:
            f.write(vis.encode_png(sheet))
        self.last_host_ms = (time.perf_counter() - t0) * 1e3
        return None


def child(args):
    root = os.path.abspath(args.root) if args.root else os.path.dirname(HERE)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import torch
    import bench
    from bench_mic import build
    from madm_amd.train import MadmTrainer
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = build(dtype, dev, "off")
    trainer = MadmTrainer(model, lr=5e-6, weight_decay=0.05, grad_clip=0.01, dist=None, amp=True)
    data = bench.train_inputs(args.batch, args.size, dev)
    out_dir = tempfile.mkdtemp(prefix="madm_vis_bench_", dir=args.tmp)
    writer = None
    if args.mode in ("async", "sync"):
        from madm_amd import vis
        writer = model.vis_writer = vis.VisWriter(out_dir, async_write=(args.mode == "async"))
    elif args.mode == "comparator":
        writer = model.vis_writer = HostComparator(out_dir)
    try:
        for _ in range(max(1, args.warmup)):
            trainer.run_step(data)
        torch.cuda.synchronize()
        per, info = [], {}
        dump_at = args.steps // 2 if writer is not None else -1
        t_all = time.perf_counter()
        for i in range(args.steps):
            if i == dump_at:
                model.vis_period = model.train_iter_index + 1          # this step's forward dumps
            t0 = time.perf_counter()
            trainer.run_step(data)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
            if i == dump_at:
                model.vis_period = None
                lv = model.last_vis
                ev = lv["events"]
                info.update(tiles=len(lv["infos"]), dump_step_ms=round(per[-1], 2),
                            extra_pass_host_ms=round(lv["host_ms"][0], 2), extra_pass_device_ms=round(ev[0].elapsed_time(ev[1]), 2),
                            dump_host_ms_without_extra_pass=round(lv["host_ms"][1], 2),
                            dump_device_bracket_ms_without_extra_pass=round(ev[1].elapsed_time(ev[2]), 3))
        wall = (time.perf_counter() - t_all) * 1e3
        t0 = time.perf_counter()
        if writer is not None:
            writer.wait()
        info["writer_tail_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        if args.mode in ("async", "sync"):
            info.update(compose_launch_device_ms=round(writer.last_compose_device_ms, 3), writer_ms=round(writer.last_write_ms, 1),
                        png_mb=round(os.path.getsize(lv["path"]) / 1e6, 2))
        if args.mode == "comparator":
            info["comparator_host_ms"] = round(writer.last_host_ms, 1)
        others = per[:dump_at] + per[dump_at + 1:] if dump_at >= 0 else per
        info.update(mode=args.mode, root=args.root or ".", dtype=args.dtype, steps=args.steps, wall_ms=round(wall, 1),
                    step_ms_median=round(statistics.median(others), 2), step_ms_min=round(min(others), 2),
                    step_ms_max=round(max(others), 2))
        print(json.dumps(info), flush=True)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def driver(args):
    rows = []
    for rnd in range(args.alternate):
        for mode in args.modes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", "none" if mode == "baseline" else mode, "--dtype", args.dtype,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch), "--size", str(args.size)]
            if mode == "baseline":
                cmd += ["--root", args.baseline_root]
            if args.tmp:
                cmd += ["--tmp", args.tmp]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
            if out.returncode != 0:             # nothing more is started on the device after a failed child
                print(json.dumps(dict(mode=mode, round=rnd, failed=out.returncode)), flush=True)
                return out.returncode
            row = json.loads(out.stdout.strip().splitlines()[-1])
            row.update(round=rnd, mode=mode)
            rows.append(row)
            print(json.dumps(row), flush=True)
    by = {}
    for r in rows:
        by.setdefault(r["mode"], []).append(r)
    summary = {m: dict(wall_ms=[r["wall_ms"] for r in rs], step_ms_median=[r["step_ms_median"] for r in rs]) for m, rs in by.items()}
    if "baseline" in by:
        w = summary["baseline"]["step_ms_median"]
        summary["baseline"]["spread_step_ms"] = round(max(w) - min(w), 2)
    if "async" in by and "comparator" in by:
        a = [r["dump_host_ms_without_extra_pass"] + r["dump_device_bracket_ms_without_extra_pass"] for r in by["async"]]
        c = [r["dump_host_ms_without_extra_pass"] for r in by["comparator"]]
        summary["training_thread_ms"] = dict(async_host_plus_device=[round(v, 2) for v in a], comparator_host=[round(v, 2) for v in c])
    print(json.dumps(dict(summary=summary)), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="async", choices=["none", "async", "sync", "comparator"])
    ap.add_argument("--root", default=None, help="import madm_amd / bench from this checkout (mode none only)")
    ap.add_argument("--alternate", type=int, default=0, help="driver: this many rounds of fresh child processes")
    ap.add_argument("--modes", default="baseline,none,async,comparator")
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--child-timeout", type=float, default=420.0)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--tmp", default=None, help="parent of the temporary directory (default: the system's)")
    args = ap.parse_args()
    if args.alternate:
        if "baseline" in args.modes.split(",") and not args.baseline_root:
            ap.error("--alternate with a baseline needs --baseline-root")
        sys.exit(driver(args))
    if args.root and args.mode != "none":
        ap.error("--root goes with --mode none")
    child(args)


if __name__ == "__main__":
    main()
