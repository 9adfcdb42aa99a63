#!/usr/bin/env python3
"""What a checkpoint costs the training loop, on the bench's training graph (bench.build_train_model's pieces: configs[3],
512 x 512, bs 2, all 866 M UNet parameters trainable): MadmTrainer steps, eager launches, one process.

Per mode -- ``async`` (MadmCheckpointer(async_save=True)), ``sync`` (async_save=False) and ``torch_save`` (a plain
``torch.save`` of ``model.state_dict()`` plus the two moments at the step boundary: what is possible without
madm_amd/checkpoint.py, the comparator) -- the tool runs ``--steps`` steps with ONE save after the middle step and prints one
JSON line: host time inside the save call, device time of the snapshot launches on the training stream (events around them),
wall time of the steps against the same number of steps without a save, the time the writer needed after the last step,
peak device memory.  ``async`` runs twice: the first save allocates the staging buffers.  Every file goes into a fresh
temporary directory that is removed at the end.
Usage: python tools/bench_checkpoint.py [--dtype f16] [--steps 20] [--warmup 3] [--modes async,async,sync,torch_save]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--modes", default="async,async,sync,torch_save")
    ap.add_argument("--tmp", default=None, help="parent of the temporary directory (default: the system's)")
    args = ap.parse_args()
    import bench
    from bench_mic import build
    from madm_amd.train import MadmTrainer
    from madm_amd.checkpoint import MadmCheckpointer
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = build(dtype, dev, "off")
    trainer = MadmTrainer(model, lr=5e-6, weight_decay=0.05, grad_clip=0.01, dist=None, amp=True)
    data = bench.train_inputs(args.batch, args.size, dev)
    state_gb = sum(b[0].numel() for b in trainer.flat_buffers().values()) * 4 / 1e9
    for _ in range(max(1, args.warmup)):
        trainer.run_step(data)
    torch.cuda.synchronize()
    out_dir = tempfile.mkdtemp(prefix="madm_ckpt_bench_", dir=args.tmp)
    savers = {}

    def run(save):
        """``--steps`` steps, each synchronised; ``save`` (or None) is called after the middle step."""
        per, info = [], {}
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for i in range(args.steps):
            t0 = time.perf_counter()
            trainer.run_step(data)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
            if save is not None and i == args.steps // 2 - 1:
                t0 = time.perf_counter()
                save(info)
                info["save_call_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                info["sync_after_save_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        return (time.perf_counter() - t_all) * 1e3, per, info

    try:
        torch.cuda.reset_peak_memory_stats()
        base_ms, per, _ = run(None)
        base = dict(mode="no_save", dtype=args.dtype, steps=args.steps, wall_ms=round(base_ms, 1),
                    step_ms_median=round(statistics.median(per), 2), step_ms_min=round(min(per), 2),
                    step_ms_max=round(max(per), 2), flat_state_gb=round(state_gb, 2),
                    peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))
        print(json.dumps(base), flush=True)
        for n, mode in enumerate(args.modes.split(",")):
            name = f"model_{n:07d}"
            if mode not in savers:                 # one checkpointer (one set of staging buffers) alive at a time
                for old in savers.values():
                    old.wait()
                savers.clear()
                torch.cuda.empty_cache()
            if mode in ("async", "sync"):
                ck = savers.get(mode)
                if ck is None:
                    ck = savers[mode] = MadmCheckpointer(model, out_dir, async_save=(mode == "async"), trainer=trainer)

                def save(info, ck=ck, name=name):
                    ck.save(name, iteration=trainer.iter - 1)
            else:
                ck = None

                def save(info, name=name):
                    torch.save({"model": model.state_dict(), "exp_avg": trainer.opt.m, "exp_avg_sq": trainer.opt.v},
                               os.path.join(out_dir, name + ".pth"))
            torch.cuda.reset_peak_memory_stats()
            wall_ms, per, info = run(save)
            t0 = time.perf_counter()
            if ck is not None:
                ck.wait()
            info["writer_tail_ms"] = round((time.perf_counter() - t0) * 1e3, 1)       # what was still pending after the last step
            path = os.path.join(out_dir, name + ".pth")
            info.update(mode=mode, first_use=(mode in ("async", "sync") and args.modes.split(",").index(mode) == n),
                        wall_ms=round(wall_ms, 1), extra_wall_ms=round(wall_ms - base_ms, 1),
                        step_ms_median=round(statistics.median(per), 2), step_ms_max=round(max(per), 2),
                        snapshot_device_ms=None if ck is None else round(ck.last_save_device_ms, 3),
                        file_gb=round(os.path.getsize(path) / 1e9, 2),
                        peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))
            if ck is not None:
                info["training_thread_ms"] = round(info["save_call_host_ms"] + (ck.last_save_device_ms if mode == "async" else 0.0), 2)
            print(json.dumps(info), flush=True)
            os.remove(path)
    finally:
        for ck in savers.values():
            try:
                ck.wait()
            except Exception as e:
                print("writer error:", repr(e), flush=True)
        shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
