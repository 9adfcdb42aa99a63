#!/usr/bin/env python3
"""The deterministic mode's measurements.

  python tools/bench_det.py kernels [--dtype f16]
      every ordered reduction of libmadm_det.so against the atomic kernel it replaces, same process, same buffers, at the
      head's largest tensor (2 x 512^2 pixels x 1024 channels) and at one UNet shape (2 x 64^2 x 320).  Differenced event
      brackets: [K] and [K K] between three events, the difference is one launch with the event pair's cost cancelled;
      median of --reps.  Bytes = what the algorithm has to read once (both kernels of a pair are charged the same).
  python tools/bench_det.py step [--deterministic 0|1] [--steps 10] [--warmup 3]
      one fresh process: the bench's training step (tools/bench_mic.py's model, mode off) with MadmTrainer's ``deterministic``
      keyword; prints one JSON line with the median, the extremes and every step's time (a host clock around a synchronised step).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def differenced_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        fn()
        e[1].record()
        fn()
        fn()
        e[2].record()
        torch.cuda.synchronize()
        out.append((e[1].elapsed_time(e[2]) - e[0].elapsed_time(e[1])) * 1e3)
    return statistics.median(out)


def kernels(args):
    from madm_amd import ops, _lib
    ops.set_deterministic(True)          # loads the library; the flag itself is switched per call below
    ops.set_deterministic(False)
    det = ops._det
    lib, dlib = _lib.lib, det.lib
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    code, es = ops.dtype_code(dtype), torch.empty(0, dtype=dtype).element_size()
    s = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    rows = []

    def pair(name, shape, nbytes, atomic, ordered):
        ta, to = differenced_us(atomic, args.reps), differenced_us(ordered, args.reps)
        rows.append((name, shape, nbytes, ta, to))
        print(f"{name:22s} {shape:26s} atomic {ta:9.1f} us ({nbytes / ta / 1e6:5.2f} TB/s)   ordered {to:9.1f} us "
              f"({nbytes / to / 1e6:5.2f} TB/s)   ratio {to / ta:5.2f}", flush=True)

    def mode(flag, fn):
        def run():
            with ops.deterministic(flag):
                fn()
        return run

    for tag, B, H, W, C, G in (("head", 2, 512, 512, 1024, 32), ("unet", 2, 64, 64, 320, 32)):
        HW = H * W
        shape = f"{tag} {B}x{H}x{W}x{C}"
        x = torch.randn((B * HW, C), device="cuda").to(dtype)
        dy = torch.randn((B * HW, C), device="cuda").to(dtype)
        one = x.numel() * es
        # colsum, groupnorm_stats, dwconv3x3_wgrad: one launch each way through ops
        out = torch.zeros((B, C), device="cuda")
        pair("colsum", shape, one, mode(False, lambda: ops.colsum(x, B, HW, out=out)), mode(True, lambda: ops.colsum(x, B, HW, out=out)))
        st = torch.zeros((B, C, 2), dtype=torch.float64, device="cuda")
        pair("groupnorm_stats", shape, one, mode(False, lambda: ops.groupnorm_stats(x, B, HW, st)),
             mode(True, lambda: ops.groupnorm_stats(x, B, HW, st)))
        dw = torch.zeros((9, C), device="cuda")
        for dil in (6, 18):
            pair(f"dwconv3x3_wgrad d{dil}", shape, 2 * one, mode(False, lambda: ops.dwconv3x3_wgrad(x, dy, B, H, W, dil, dw=dw)),
                 mode(True, lambda: ops.dwconv3x3_wgrad(x, dy, B, H, W, dil, dw=dw)))
        # groupnorm_bwd_sums: the two entry points on the same arguments
        stats = torch.zeros((B, C, 2), dtype=torch.float64, device="cuda")
        ops.groupnorm_stats(x, B, HW, stats)
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        bsums = torch.zeros((B, C, 2), dtype=torch.float64, device="cuda")
        nws = dlib.mdet_groupnorm_bwd_sums_workspace_bytes(B, HW, C)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        common = (code, x.data_ptr(), dy.data_ptr(), C, B, HW, C, 0, C, G, stats.data_ptr(), C, None, gamma.data_ptr(),
                  beta.data_ptr(), 1e-5, 1, bsums.data_ptr())
        pair("groupnorm_bwd_sums", shape, 2 * one, lambda: _lib.check(lib.madm_groupnorm_bwd_sums(*common, s()), "bwd_sums"),
             lambda: det.check(dlib.mdet_groupnorm_bwd_sums(*common, ws.data_ptr(), nws, s()), "bwd_sums"))
        del x, dy, ws
        torch.cuda.empty_cache()
    # LayerNorm: the dx kernel with its atomic parameter sums against the dx kernel without + the ordered parameter kernel
    for M, C in ((2 * 4096, 320), (2 * 1024, 640)):
        x = torch.randn((M, C), device="cuda").to(dtype)
        dy = torch.randn((M, C), device="cuda").to(dtype)
        g = torch.ones(C, device="cuda")
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        pair("layernorm_backward", f"unet {M}x{C}", 2 * x.numel() * es,
             mode(False, lambda: ops.layernorm_backward(x, dy, g, 1e-5, dgamma=dg, dbeta=db)),
             mode(True, lambda: ops.layernorm_backward(x, dy, g, 1e-5, dgamma=dg, dbeta=db)))
    print(json.dumps([dict(kernel=r[0], shape=r[1], bytes=r[2], atomic_us=round(r[3], 1), ordered_us=round(r[4], 1)) for r in rows]))


def step(args):
    import bench
    import bench_mic
    from madm_amd.train import MadmTrainer
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = bench_mic.build(dtype, dev, "off")
    kw = dict(deterministic=True) if args.deterministic else {}      # (the keyword is left out when off: older trees lack it)
    trainer = MadmTrainer(model, lr=5e-6, weight_decay=0.05, grad_clip=0.01, dist=None, amp=True, **kw)
    data = bench.train_inputs(args.batch, args.size, dev)
    for _ in range(max(1, args.warmup)):
        trainer.run_step(data)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        trainer.run_step(data)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(deterministic=bool(args.deterministic), dtype=args.dtype, batch=args.batch, size=args.size,
                          median_ms=round(statistics.median(ms), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2),
                          steps_ms=[round(v, 2) for v in ms])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step"])
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--deterministic", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_det.py needs the GPU: there is no CPU path")
    kernels(args) if args.what == "kernels" else step(args)


if __name__ == "__main__":
    main()
