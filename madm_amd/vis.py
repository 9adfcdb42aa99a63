"""The periodic training picture: ``<output_dir>/vis_results/{iter:06d}_rank{r}.png`` every ``vis_period`` iterations, as
the reference's ``vis_results`` writes it (modeling/meta_arch/cmdise.py:238-305, called from mtmadise.py:552-653) -- source
image / prediction / label, target image, the teacher's pseudo labels, the mixed image with its prediction and label, the
VAE-decoder outputs -- for people who watch whether the pseudo labels collapse.

The reference builds the figure inside ``forward`` on the host: ``.cpu()`` copies, ``F.interpolate`` + softmax + max per
logits tile, PIL palettes, matplotlib.  Here the sheet is ONE ``madm_vis_compose`` launch (csrc/vis.hip) on the training
stream into a device canvas that is kept and reused; an event is recorded and everything else -- the copy to a pinned host
buffer, the PNG encoding (``zlib`` + ``struct``: no PIL / matplotlib in the product path), the write under a temporary name,
the rename -- runs on ONE writer thread with ONE stream of its own (``VisWriter``, the pattern of checkpoint.py).  The call
never synchronises the training stream.  A sidecar ``{iter:06d}_rank{r}.json`` lists every tile's ``info``, kind and
rectangles: it stands in for matplotlib's subplot titles.

Tiles are the reference's dicts: ``{'data_type': 'image' | 'label' | 'logits' | 'heatmap', 'info': str, 'data': tensor}``
(+ ``'denorm': (scale, shift)`` on an image tile to override the sheet's).  All tiles have the spatial size of tile 0; only
logits are resized (bilinear, align_corners=False, inside the kernel)."""
import atexit
import json
import logging
import os
import struct
import threading
import time
import weakref
import zlib

import numpy as np
import torch

from . import _lib

logger = logging.getLogger("madm_amd.vis")

KINDS = {"image": _lib.VIS_IMAGE, "label": _lib.VIS_LABEL, "logits": _lib.VIS_LOGITS, "heatmap": _lib.VIS_HEAT}
MAX_TILES = _lib.VIS_MAX_TILES


def layout(n, B, cols_max=5):
    """(rows, cols, cells) of a sheet of ``n`` tiles for ``B`` images: cols = min(cols_max, n), rows = B * ceil(n /
    cols_max), ``cells[i][j]`` = (row, column) of tile i of image j (cmdise.py:250,261)."""
    n, B, cols_max = int(n), int(B), int(cols_max)
    if n < 1 or B < 1 or cols_max < 1:
        raise ValueError(f"layout: n, B and cols_max must be positive, got {n}, {B}, {cols_max}")
    per_img = -(-n // cols_max)
    cells = [[(j * per_img + i // cols_max, i % cols_max) for j in range(B)] for i in range(n)]
    return B * per_img, min(cols_max, n), cells


def _device_tensor(tile):
    """The tile's tensor in the layout the kernel reads (f32 NCHW / i64 [B, H, W] / f32 [B, H, W])."""
    kind, t = tile["data_type"], tile["data"]
    if kind not in KINDS:
        raise ValueError(f"tile {tile.get('info')!r}: unknown data_type {kind!r} (one of {sorted(KINDS)})")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"tile {tile.get('info')!r}: needs a device tensor (the HIP path has no CPU fallback)")
    if kind in ("label", "heatmap"):
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if t.dim() != 3:
            raise ValueError(f"tile {tile.get('info')!r}: a {kind} tile is [B, H, W] or [B, 1, H, W], got {tuple(t.shape)}")
        return t.to(torch.int64 if kind == "label" else torch.float32).contiguous()
    if t.dim() != 4 or (kind == "image" and t.shape[1] != 3):
        raise ValueError(f"tile {tile.get('info')!r}: a {kind} tile is [B, {'3' if kind == 'image' else 'K'}, H, W], "
                         f"got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def compose(tiles, cols_max=5, palette=None, denorm=(0.5, 0.5), out=None):
    """The RGB8 sheet of ``tiles`` as a device tensor u8 [rows*H, cols*W, 3], written by one launch on the current stream.
    ``palette``: list of up to 768 ints (zero-padded like ``labels.pad_palette``); ``denorm`` = (scale, shift) of the image
    tiles: byte = round(255 * clip(x * scale + shift, 0, 1)), (0.5, 0.5) for [-1, 1] images, (1, 0) for [0, 1] images.
    ``out``: a canvas of the right size to reuse."""
    from . import ops, labels
    if not 1 <= len(tiles) <= MAX_TILES:
        raise ValueError(f"a sheet holds 1 .. {MAX_TILES} tiles, got {len(tiles)}")
    if palette is None:
        raise ValueError("compose needs the class palette")
    ts = [_device_tensor(t) for t in tiles]
    B, (H, W) = ts[0].shape[0], ts[0].shape[-2:]
    dev = ts[0].device
    rows, cols, _ = layout(len(tiles), B, cols_max)
    if out is None or tuple(out.shape) != (rows * H, cols * W, 3) or out.device != dev:
        out = torch.empty((rows * H, cols * W, 3), dtype=torch.uint8, device=dev)
    table = []
    for tile, t in zip(tiles, ts):
        sc, sh = tile.get("denorm", denorm)
        table.append((KINDS[tile["data_type"]], t, float(sc), float(sh)))
    pal = palette if isinstance(palette, torch.Tensor) else labels._device_palette(list(palette), dev)
    return ops.vis_compose(table, B, H, W, int(cols_max), pal, out)


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(array):
    """u8 [H, W, 3] (numpy array or CPU tensor) -> the bytes of an RGB8 PNG: filter 0 on every row, zlib level 1."""
    a = array.numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_png: needs a uint8 [H, W, 3] array, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    raw = np.zeros((H, 1 + W * 3), dtype=np.uint8)          # column 0: the filter byte of each row
    raw[:, 1:] = a.reshape(H, W * 3)
    return b"".join((_PNG_MAGIC, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)),
                     _chunk(b"IDAT", zlib.compress(raw.tobytes(), 1)), _chunk(b"IEND", b"")))


class VisWriter:
    """Writes ``<output_dir>/vis_results/{iteration:06d}_rank{rank}.png`` + ``.json``.  ``submit`` composes on the caller's
    current stream and returns; the file work runs on a writer thread (``async_write=True``) or in line (the same code).
    One sheet is in flight at a time: a second ``submit`` first waits for the pending one (one canvas, one host buffer).
    What the writer raised is re-raised by the next ``submit``, ``wait()`` or ``close()``; the object waits at interpreter
    exit."""
    subdir = "vis_results"

    def __init__(self, output_dir, rank=0, async_write=True):
        if not output_dir:
            raise ValueError("VisWriter needs an output directory")
        self.output_dir = os.fspath(output_dir)
        self.rank = int(rank)
        self.async_write = bool(async_write)
        self.canvas = None            # device sheet, kept and reused
        self._host = None             # pinned host copy
        self._copy_stream = None
        self._thread = None
        self._error = None
        self.closed = False
        self.last_compose_device_ms = None
        self.last_write_ms = None
        ref = weakref.ref(self)
        atexit.register(lambda: ref() is not None and ref()._wait_at_exit())

    def path(self, iteration, ext="png"):
        return os.path.join(self.output_dir, self.subdir, f"{int(iteration):06d}_rank{self.rank}.{ext}")

    # ------------------------------------------------------------------ waiting
    def wait(self):
        """Blocks until the pending sheet is on disk; re-raises what the writer raised."""
        t = self._thread
        if t is not None:
            t.join()
            self._thread = None
        err, self._error = self._error, None
        if err is not None:
            raise err

    def close(self):
        self.closed = True
        self.wait()

    def _wait_at_exit(self):
        try:
            self.wait()
        except BaseException as e:       # the interpreter is going down: say it, there is nobody left to raise to
            logger.error("vis writer failed: %r", e)

    # ------------------------------------------------------------------ the caller's share
    def submit(self, iteration, tiles, cols_max=5, palette=None, denorm=(0.5, 0.5)):
        """Composes ``tiles`` into the kept canvas on the current stream, records an event and hands the sheet to the
        writer.  Returns the device canvas (valid until the next ``submit``)."""
        self.wait()                   # one canvas: the pending sheet leaves it first (and reports its error)
        if self.closed:
            raise RuntimeError("VisWriter is closed")
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        self.canvas = compose(tiles, cols_max, palette, denorm, out=self.canvas)
        ev[1].record()
        first = tiles[0]["data"]
        B, (H, W) = first.shape[0], first.shape[-2:]
        meta = self.describe(tiles, B, H, W, cols_max)
        self._start(dict(iteration=int(iteration), canvas=self.canvas, meta=meta, event=ev,
                         lazy=[t.get("info_value") for t in tiles]))
        return self.canvas

    def submit_canvas(self, iteration, canvas, meta):
        """The writer's half alone: a finished u8 [H, W, 3] sheet (CPU tensors too: tests, tools) and its sidecar dict."""
        self.wait()
        if self.closed:
            raise RuntimeError("VisWriter is closed")
        ev = None
        if canvas.is_cuda:
            ev = (None, torch.cuda.Event())
            ev[1].record()
        self._start(dict(iteration=int(iteration), canvas=canvas, meta=meta, event=ev, lazy=[]))

    @staticmethod
    def describe(tiles, B, H, W, cols_max):
        """The sidecar: per tile its info, kind and one [x, y, w, h] rectangle per image."""
        rows, cols, cells = layout(len(tiles), B, cols_max)
        return dict(tile_size=[int(H), int(W)], rows=rows, cols=cols, cols_max=int(cols_max), batch=int(B),
                    tiles=[dict(info=str(t["info"]), kind=t["data_type"],
                                rects=[[c * int(W), r * int(H), int(W), int(H)] for r, c in cells[i]])
                           for i, t in enumerate(tiles)])

    def _start(self, job):
        if self.async_write:
            self._thread = threading.Thread(target=self._writer_entry, args=(job,), name="madm-vis-writer")
            self._thread.start()
        else:
            self._write(job)

    # ------------------------------------------------------------------ the writer's share
    def _writer_entry(self, job):
        try:
            self._write(job)
        except BaseException as e:
            self._error = e

    def _write(self, job):
        t0 = time.perf_counter()
        canvas, meta = job["canvas"], dict(job["meta"])
        values = []
        if canvas.is_cuda:
            torch.cuda.set_device(canvas.device)
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=canvas.device)
            if self._host is None or self._host.shape != canvas.shape:
                self._host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(self._copy_stream):
                self._copy_stream.wait_event(job["event"][1])     # the sheet is complete; the training stream is not touched
                self._host.copy_(canvas, non_blocking=True)
                values = [None if v is None else v.to("cpu", non_blocking=False) for v in job["lazy"]]
                self._copy_stream.synchronize()
            if job["event"][0] is not None:
                self.last_compose_device_ms = job["event"][0].elapsed_time(job["event"][1])
            host = self._host
        else:
            host = canvas
        # titles that hold a device value (the share of confident pseudo labels): formatted here, off the training thread
        if any(v is not None for v in values):
            meta["tiles"] = [dict(t, info=t["info"].format(float(v))) if v is not None else t
                             for t, v in zip(meta["tiles"], values)]
        meta.update(iteration=job["iteration"], rank=self.rank)
        png = self._encode(host)
        final_png, final_json = self.path(job["iteration"]), self.path(job["iteration"], "json")
        os.makedirs(os.path.dirname(final_png), exist_ok=True)
        # the sidecar first: whoever sees the picture finds its sidecar; neither name ever holds a partial file
        for final, data in ((final_json, json.dumps(meta, indent=1).encode()), (final_png, png)):
            tmp = os.path.join(os.path.dirname(final), "." + os.path.basename(final) + ".tmp")
            try:
                with open(tmp, "wb") as f:
                    f.write(data)
                os.replace(tmp, final)
            except BaseException:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise
        self.last_write_ms = (time.perf_counter() - t0) * 1e3

    @staticmethod
    def _encode(host):
        return encode_png(host)
