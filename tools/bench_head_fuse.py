"""Times ``DAFormerHead`` alone at the evaluation size (s0 128 x 512 x 512, s3 / s4 / s5 512 x 64 x 64 / 32 x 32 / 16 x 16,
bs 1, eval mode, f16, seeded weights and features) in three forms, alternating them round by round in one process:

  off        final_fuse_vae_decoder_feat=False: the head as it was (fusion at 512 x 512)
  composed   the flag on, classifier by the composed path (resize to 512 x 512 + two-source conv)
  fused      the flag on, classifier by ops.upsample_cat_classify (libmadm_headfuse.so)

Each sample is a device-event bracket around ``--calls`` forward_tokens calls on the current stream, ended by a synchronise;
``--rounds`` samples per form, the median and the spread (min .. max) per call are printed and, with ``--json``, written as one
JSON line.  Needs a GPU: there is no other way to obtain these numbers.

``--eval-images N`` adds, for information, ``inference_on_dataset`` over N seeded synthetic 512 x 512 images on the DEPTH eval
model (bench.py's) with the head as it was and with a flagged head -- two different models, not a regression pair -- as steady
images/s (tools/eval_export_bench.py's loader, evaluator and definition), alternated ``--eval-repeats`` times after a warm-up.

    python tools/bench_head_fuse.py [--size 512] [--dtype f16] [--rounds 15] [--calls 10] [--eval-images 0] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32"])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--classes", type=int, default=11)
    ap.add_argument("--eval-images", type=int, default=0)
    ap.add_argument("--eval-repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_head_fuse: needs a GPU")
    from madm_amd import ops, weights
    from madm_amd.head import DAFormerHead
    from madm_amd.nn import Tok
    from oracle import madm_path
    dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]
    S = args.size
    sizes = [(S, S), (S // 8, S // 8), (S // 16, S // 16), (S // 32, S // 32)]
    chans = [128, 512, 512, 512]
    toks = []
    for i, ((h, w), c) in enumerate(zip(sizes, chans)):
        x = torch.randn((h * w, c), generator=torch.Generator().manual_seed(100 + i))
        toks.append(Tok(x.to(dtype).cuda(), 1, h, w))

    def build(flag):
        head = DAFormerHead(in_channels=chans, in_keys=["s0", "s3", "s4", "s5"], in_index=[0, 1, 2, 3], channels=256,
                            num_classes=args.classes, norm_cfg=dict(type='BN'), decoder_params=madm_path.head_decoder_params(),
                            final_fuse_vae_decoder_feat=flag)
        weights.synth_init_(head, 7, "head.")
        weights.synth_buffers_(head, 7, "head.")
        return head.cuda().eval()

    off, on = build(False), build(True)

    def run(form):
        if form == "off":
            return off.forward_tokens(toks)
        on.fused_classifier = form == "fused"
        out = on.forward_tokens(toks)
        assert on.last_route == form
        return out

    forms = ["off", "composed", "fused"]
    samples = {f: [] for f in forms}
    with torch.no_grad(), ops.tuning_profile("throughput", pin=True):
        outs = {f: run(f).t.float() for f in forms}           # warm-up of every shape, and the two routes against each other
        torch.cuda.synchronize()
        diff = (outs["fused"] - outs["composed"]).abs().max().item() / outs["composed"].abs().max().item()
        for f in forms:
            for _ in range(3):
                run(f)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for f in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _c in range(args.calls):
                    run(f)
                e1.record()
                e1.synchronize()
                samples[f].append(e0.elapsed_time(e1) / args.calls)
    res = {"size": S, "dtype": args.dtype, "classes": args.classes, "rounds": args.rounds, "calls": args.calls,
           "device": torch.cuda.get_device_name(0), "fused_vs_composed_max_rel": diff}
    for f in forms:
        v = samples[f]
        res[f] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        print(f"{f:9s} median {res[f]['median_ms']:.3f} ms  (min {min(v):.3f} .. max {max(v):.3f}) per head call")
    print(f"fused against composed logits: max |difference| / max |logit| = {diff:.2e}")
    if args.eval_images:
        res["inference_on_dataset"] = eval_rates(args, dtype, build)
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


def eval_rates(args, dtype, build_head):
    """steady images/s of inference_on_dataset with the plain and with the flagged head (best of --eval-repeats, alternated)"""
    import bench
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import eval_export_bench as eb
    device = torch.device("cuda:0")
    models = {}
    with torch.no_grad():
        for name, flag in (("off", False), ("on", True)):
            m = bench.build_eval_model(dtype, device, num_classes=args.classes)
            if flag:
                m.sem_seg_head = m.sem_seg_head_sec_modal = build_head(True)
            models[name] = m
        items = eb.make_images(args.eval_images, args.size, device)
        rates = {k: [] for k in models}
        for k, m in models.items():                                           # warm-up, untimed
            eb.one_run(m, items, eb.evaluator(None, -1, False, 1))
        for _ in range(args.eval_repeats):
            for k, m in models.items():
                row = eb.one_run(m, items, eb.evaluator(None, -1, False, 1))
                rates[k].append(row["steady_images_per_s"])
                print(f"# inference_on_dataset, flag {k}: {row}", flush=True)
    return {k: max(v) for k, v in rates.items()}


if __name__ == "__main__":
    main()
