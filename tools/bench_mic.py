#!/usr/bin/env python3
"""Training-step time and peak memory of the bench's training graph (bench.build_train_model: configs[3], 512 x 512, bs 2)
with masked image consistency off, ``mic`` and ``mic_reg``.  MadmTrainer steps, eager launches, one process.
Usage: python tools/bench_mic.py [--dtype f16] [--steps 10] [--warmup 3] [--modes off,mic,mic_reg]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dtype, dev, mode):
    import bench
    from madm_amd.mtmadise import MTMADISE
    from madm_amd.criterion import CmdiseCriterion
    ev = bench.build_eval_model(dtype, dev, finetune_unet='all')
    palette = [int(v) for v in torch.randint(0, 256, (33,), generator=torch.Generator().manual_seed(99))]
    extra = {"off": {}, "mic": dict(mic=True), "mic_reg": dict(mic_reg=1.0)}[mode]
    model = MTMADISE(ev.backbone, ev.sem_seg_head, CmdiseCriterion(num_classes=11), target_modality="Depth",
                     train_palette=palette, vae_decoder_loss='st', vae_decoder_loss_type='L1',
                     vae_decoder_loss_weight=[1.0, 1.0], reg_uncertain=True, rev_noise_sup=True, rev_noise_end_iter=5000,
                     rev_noise_gradually=True, denoise_timestep_range=[60, 61], max_iter=10000, color_aug_flag=False, **extra)
    return model.train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--modes", default="off,mic,mic_reg")
    args = ap.parse_args()
    import bench
    from madm_amd.train import MadmTrainer
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    dev = torch.device("cuda")
    for mode in args.modes.split(","):
        torch.manual_seed(0)
        model = build(dtype, dev, mode)
        trainer = MadmTrainer(model, lr=5e-6, weight_decay=0.05, grad_clip=0.01, dist=None, amp=True)
        data = bench.train_inputs(args.batch, args.size, dev)
        for _ in range(max(1, args.warmup)):
            losses, _, _ = trainer.run_step(data)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            losses, _, _ = trainer.run_step(data)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        print(json.dumps(dict(mode=mode, dtype=args.dtype, batch=args.batch, size=args.size, step_ms=round(ms, 2),
                              peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
                              losses=sorted(losses))), flush=True)
        del model, trainer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
