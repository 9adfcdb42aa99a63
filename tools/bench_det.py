#!/usr/bin/env python3
"""The deterministic mode's measurements (DESIGN.md sections 24 and 28).

  python tools/bench_det.py kernels [--dtype f16] [--only reductions|wgrad]
      every ordered reduction of libmadm_det.so against the atomic kernel it replaces, same process, same buffers, at the
      head's largest tensor (2 x 512^2 pixels x 1024 channels) and at one UNet shape (2 x 64^2 x 320).  Differenced event
      brackets: [K] and [K K] between three events, the difference is one launch with the event pair's cost cancelled;
      median of --reps.  Bytes = what the algorithm has to read once (both kernels of a pair are charged the same).
      Then the weight-gradient table: one MadmTrainer(deterministic=True) step of the bench's model with every
      ops.conv2d_wgrad call bracketed by events, the ten geometries that cost most per step in that one-slice profile, and for
      each the three paths on the same buffers: atomic (default mode), one slice (True), slab kernel + fold ("slabs").
      Every timed call switches the mode and launches eagerly: rows of a few microseconds are bounded by the host and rank
      nothing -- time those in a hipGraph (tools/bench_backward.py [--slabs]).
  python tools/bench_det.py step [--deterministic 0|1|slabs] [--steps 10] [--warmup 3]
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


def wgrad_table(args):
    """The ten weight-gradient geometries that cost most in a one-slice step, each on the three paths"""
    import bench
    import bench_mic
    from madm_amd import ops
    from madm_amd.train import MadmTrainer
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = bench_mic.build(dtype, dev, "off")
    trainer = MadmTrainer(model, lr=5e-6, weight_decay=0.05, grad_clip=0.01, dist=None, amp=True, deterministic=True)
    data = bench.train_inputs(args.batch, args.size, dev)
    trainer.run_step(data)
    torch.cuda.synchronize()
    calls, real = [], ops.conv2d_wgrad

    def recorded(x1, dout, B, IH, IW, *, x2=None, KH=1, KW=1, stride=1, pad_t=0, pad_l=0, OH=None, OW=None, upsample=False,
                 dw=None, splitm=0, dbias=None, slabs=None):
        key = (x1.dtype, B, IH, IW, x1.shape[1], 0 if x2 is None else x2.shape[1], dout.shape[1], KH, KW, stride, pad_t, pad_l, OH, OW,
               bool(upsample), dbias is not None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real(x1, dout, B, IH, IW, x2=x2, KH=KH, KW=KW, stride=stride, pad_t=pad_t, pad_l=pad_l, OH=OH, OW=OW,
                   upsample=upsample, dw=dw, splitm=splitm, dbias=dbias, slabs=slabs)
        e1.record()
        calls.append((key, e0, e1))
        return out

    ops.conv2d_wgrad = recorded
    try:
        trainer.run_step(data)
        torch.cuda.synchronize()
    finally:
        ops.conv2d_wgrad = real
    per = {}
    for key, e0, e1 in calls:
        n, ms = per.get(key, (0, 0.0))
        per[key] = (n + 1, ms + e0.elapsed_time(e1))
    total = sum(ms for _n, ms in per.values())
    top = sorted(per.items(), key=lambda kv: -kv[1][1])[:10]
    print(f"# one-slice step: {len(calls)} conv2d_wgrad calls, {len(per)} geometries, {total:.1f} ms by event pairs; the ten "
          f"below: {sum(ms for _k, (_n, ms) in top):.1f} ms", flush=True)
    del model, trainer, data, calls
    torch.cuda.empty_cache()
    wl = None
    rows = []
    for key, (n, ms) in top:
        dt, B, IH, IW, C1, C2, N, KH, KW, stride, pad_t, pad_l, OH, OW, ups, bias = key
        oh, ow = (OH, OW) if OH is not None else (IH * (2 if ups else 1), IW * (2 if ups else 1))
        x1 = torch.randn((B * IH * IW, C1), device="cuda").to(dt)
        x2 = torch.randn((B * IH * IW, C2), device="cuda").to(dt) if C2 else None
        dout = torch.randn((B * oh * ow, N), device="cuda").to(dt)
        dw = torch.zeros((N, KH * KW * (C1 + C2)), device="cuda")
        db = torch.zeros(N, device="cuda") if bias else None
        kw = dict(x2=x2, KH=KH, KW=KW, stride=stride, pad_t=pad_t, pad_l=pad_l, OH=OH, OW=OW, upsample=ups, dw=dw, dbias=db)

        def mode(flag):
            def run():
                with ops.deterministic(flag):
                    ops.conv2d_wgrad(x1, dout, B, IH, IW, **kw)
            return run

        ta, t1, ts = (differenced_us(mode(f), args.reps) for f in (False, True, "slabs"))
        if wl is None:
            from madm_amd import _lib_wslab as wl
        a = wl.Conv2dWgradArgs(dtype=ops.dtype_code(dt), B=B, IH=IH, IW=IW, OH=oh, OW=ow, KH=KH, KW=KW, stride=stride, C1=C1, C2=C2, N=N)
        sl = wl.lib.mws_conv2d_wgrad_slices(ctypes.byref(a))
        shape = f"M{B * oh * ow} N{N} K{KH * KW * (C1 + C2)} k{KH} s{stride}{' up' if ups else ''}"
        rows.append(dict(shape=shape, calls=n, one_slice_step_ms=round(ms, 2), atomic_us=round(ta, 1), one_slice_us=round(t1, 1),
                         slabs_us=round(ts, 1), slices=sl))
        print(f"{shape:34s} x{n:3d} {ms:7.2f} ms/step   atomic {ta:8.1f} us   one slice {t1:8.1f} us   slabs + fold {ts:8.1f} us "
              f"({sl:3d} slices)   slabs / one slice {ts / t1:5.2f}", flush=True)
    print(json.dumps(rows))


def step(args):
    import bench
    import bench_mic
    from madm_amd.train import MadmTrainer
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = bench_mic.build(dtype, dev, "off")
    det = {"0": False, "1": True, "slabs": "slabs"}[args.deterministic]
    kw = dict(deterministic=det) if det else {}      # (the keyword is left out when off: older trees lack it)
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
    print(json.dumps(dict(deterministic=det, dtype=args.dtype, batch=args.batch, size=args.size,
                          median_ms=round(statistics.median(ms), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2),
                          steps_ms=[round(v, 2) for v in ms])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step"])
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--deterministic", choices=["0", "1", "slabs"], default="0")
    ap.add_argument("--only", choices=["reductions", "wgrad"], default=None, help="kernels: one of the two tables")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_det.py needs the GPU: there is no CPU path")
    if args.what == "step":
        return step(args)
    if args.only != "wgrad":
        kernels(args)
    if args.only != "reductions":
        wgrad_table(args)


if __name__ == "__main__":
    main()
