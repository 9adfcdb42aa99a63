"""Records what the runners of madm_amd/pipeline.py enqueue per submit -- events, waits, asynchronous copies, graph replays -- as
a list of ``[operation, stream role, object role]``, for tests/test_pipeline_order_gpu.py.  Uses nothing of a runner but its
constructor arguments, ``submit``, ``drain``, ``n_slots`` and its stream list, so the same code traces any revision of the runners
(``python tests/pipeline_trace.py`` on a GPU box prints the traces of every case as JSON: that is how
tests/golden/pipeline_submit_order.json was written)."""
import contextlib
from unittest import mock

import torch

IMAGE_HW = (64, 64)       # inference runners: the smallest image MadmInference pads to (one 64-multiple; the backbone resizes to 512 x 512)


def _key(stream):
    return (stream.device.index, stream.cuda_stream)


class Trace:
    def __init__(self, runner):
        streams = getattr(runner, "streams", None) or runner.streams_
        self.n_slots = runner.n_slots
        self.stream_roles = {_key(s): i for i, s in enumerate(streams)}
        self.stream_roles.setdefault(_key(torch.cuda.current_stream()), "caller")
        self.events, self.graphs = {}, {}        # id -> (object kept alive, role)
        self.log = []
        self.submit_no, self.replays = -1, 0
        self.depth = 0

    def stream(self, s=None):
        return self.stream_roles.get(_key(s if s is not None else torch.cuda.current_stream()), "other")

    def event(self, ev):
        return self.events.setdefault(id(ev), (ev, len(self.events)))[1]

    def graph(self, g):
        name = [self.submit_no % self.n_slots, self.replays]      # (slot, stage) at its FIRST replay; the object keeps the name
        self.replays += 1
        return self.graphs.setdefault(id(g), (g, name))[1]

    def next_submit(self):
        self.submit_no, self.replays = self.submit_no + 1, 0

    @contextlib.contextmanager
    def recording(self):
        def wrap(cls, name, entry):
            orig = getattr(cls, name)

            def wrapper(obj, *a, **k):
                if self.depth == 0:           # Stream.wait_stream is built on record + wait_event: log the outermost call only
                    e = entry(obj, *a, **k)
                    if e is not None:
                        self.log.append(list(e))
                self.depth += 1
                try:
                    return orig(obj, *a, **k)
                finally:
                    self.depth -= 1
            return mock.patch.object(cls, name, wrapper)

        def copy_entry(dst, src, non_blocking=False):
            if non_blocking:
                return "copy_", self.stream(), f"{src.device.type}->{dst.device.type}"

        patches = [
            wrap(torch.cuda.Event, "record", lambda ev, stream=None: ("record", self.stream(stream), self.event(ev))),
            wrap(torch.cuda.Stream, "wait_event", lambda s, ev: ("wait_event", self.stream(s), self.event(ev))),
            wrap(torch.cuda.Stream, "wait_stream", lambda s, other: ("wait_stream", self.stream(s), self.stream(other))),
            wrap(torch.cuda.Stream, "synchronize", lambda s: ("synchronize", self.stream(s), None)),
            wrap(torch.cuda.CUDAGraph, "replay", lambda g: ("replay", self.stream(), self.graph(g))),
            wrap(torch.Tensor, "copy_", copy_entry),
            wrap(torch.Tensor, "record_stream", lambda t, s: ("record_stream", self.stream(s), None)),
        ]
        with contextlib.ExitStack() as stack:
            for p in patches:
                stack.enter_context(p)
            yield self


def trace_submits(runner, inputs):
    """``2 * n_slots + 1`` submits (slot reuse and the wrap of the ready ring are inside) of ``inputs[i % len(inputs)]``, then
    ``drain()``.  Construction (warm-up, capture) happened before and is not part of the trace."""
    torch.cuda.synchronize()
    tr = Trace(runner)
    held = []
    with tr.recording():
        for i in range(2 * runner.n_slots + 1):
            tr.next_submit()
            held.append(runner.submit(inputs[i % len(inputs)]))
        runner.drain()
    return tr.log


def extractor_batches(n, B=2, H=64, W=64):
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(5000 + i)
        out.append({"img": torch.rand((B, 3, H, W), generator=g).cuda(),
                    "cond_inputs": (0.02 * torch.randn((B, 77, 768), generator=g)).cuda(),
                    "cond_emb": (0.02 * torch.randn((B, 1, 1280), generator=g)).cuda()})
    return out


def host_batches(batches):
    """Pinned image, pageable prompt tokens, device time residual (tests/test_parity_gpu.py::test_staged_pipeline_matches_forward)."""
    return [{"img": b["img"].cpu().pin_memory(), "cond_inputs": b["cond_inputs"].cpu(), "cond_emb": b["cond_emb"]} for b in batches]


def images(n, device_of=lambda i: True):
    g = torch.Generator().manual_seed(61)
    out = []
    for i in range(n):
        im = 255.0 * torch.rand((3, *IMAGE_HW), generator=g)
        out.append([{"target_second_modality": im.cuda() if device_of(i) else im}])
    return out


def build_extractor():
    """The ``extractor`` fixture of tests/test_parity_gpu.py, at f16 (the reference's autocast type)."""
    from madm_amd.ldm_rocm import LdmRocm
    m = LdmRocm("", encoder_block_indices=[], unet_block_indices=[5, 8, 11], decoder_block_indices=[], input_range='-1+1',
                unet_block_indices_type='after', finetune_unet='all', compute_dtype=torch.float32, weights='synthetic', seed=0)
    m.compute_dtype = m.vae.compute_dtype = m.unet.compute_dtype = torch.float16
    return m


def extractor_cases(ldm):
    """name -> trace, for the StagedExtractor cases (``ldm``: an LdmRocm with its compute dtype set)."""
    from madm_amd.pipeline import StagedExtractor
    dev = extractor_batches(3)
    with torch.no_grad():
        return {
            "extractor_u3_device": trace_submits(StagedExtractor(ldm, dev[0], unet_streams=3), dev),
            "extractor_u3_host": trace_submits(StagedExtractor(ldm, dev[0], unet_streams=3), host_batches(dev)),
            "extractor_u3_slots6": trace_submits(StagedExtractor(ldm, dev[0], unet_streams=3, slots=6), dev),
            "extractor_u2_nosync_norange": trace_submits(
                StagedExtractor(ldm, dev[0], unet_streams=2, sync_inputs=False, range_check=False), dev),
        }


def inference_cases(model):
    """name -> trace, for the whole-model runners (``model``: the product MadmInference of tests/test_eval_gpu.py)."""
    from madm_amd.pipeline import GraphedInference, StagedInference
    mixed = images(4, device_of=lambda i: i % 2 == 1)          # host, device, host, device, ...
    dev = images(3)
    return {
        "graphed_s4_host_device": trace_submits(GraphedInference(model, mixed[1], streams=4), mixed),
        "staged_inference_u2_slots6": trace_submits(StagedInference(model, dev[0], unet_streams=2, slots=6), dev),
    }


if __name__ == "__main__":       # prints the golden file
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from test_eval_gpu import _build_product
    cases = extractor_cases(build_extractor())
    cases.update(inference_cases(_build_product("DEPTH", torch.float16)))
    print(json.dumps({"image_hw": list(IMAGE_HW), "cases": cases}, indent=None, separators=(",", ":")))
