"""The evaluator's exports (evaluation/d2_evaluator.py:131-183 of the reference): for every ``save_eval_results_step``-th
evaluated image either one ``image | pred | gt`` sheet (during training) or, with ``eval_only``, the four files ``image/``,
``pred/`` (16-bit class ids), ``pred_color/`` and ``gt/`` that the README's eval command leaves behind.

The reference makes them inside ``process`` with ``.cpu()``, numpy, PIL and matplotlib, once per image.  Here
``inference_on_dataset`` keeps four whole-forward graphs in flight and ``process`` is chained on a slot's stream without a
host sync, so the export is built like vis.py and checkpoint.py: ONE launch on the caller's stream
(``madm_eval_export_pack``, csrc/eval_export.hip: all four files' pixel data already as PNG scanlines in one buffer; a
sheet is one ``vis.compose`` launch), an event, and everything else off the submitting thread: a small pool of worker threads waits for
the event on the exporter's own copy stream, copies to a pinned host buffer, runs ``zlib`` on slices of it, writes each
file under a temporary name and renames it.  A ring of slots (device buffer + pinned buffer + event) bounds what is in flight: a full ring blocks ``submit``
on the oldest job (back-pressure, counted in ``stats``), no file is ever dropped.

Sheets: three tiles in the fixed order image, pred, gt (the reference's subplot order); no titles or margins."""
import atexit
import logging
import os
import queue
import struct
import threading
import time
import weakref
import zlib

import numpy as np
import torch

from .vis import _PNG_MAGIC, _chunk, compose, encode_png

logger = logging.getLogger("madm_amd.eval_export")

# (directory, bit depth, PNG colour type, bytes per pixel) of the planes of the pack buffer, in buffer order
PLANES = (("image", 8, 2, 3), ("pred", 16, 0, 2), ("pred_color", 8, 2, 3), ("gt", 8, 2, 3))
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def pack_bytes(H, W):
    return int(H) * (4 + 11 * int(W))


def plane_slices(H, W):
    """[(offset, nbytes)] of the four planes inside the pack buffer of an H x W image."""
    out, off = [], 0
    for _name, _depth, _colour, bpp in PLANES:
        n = int(H) * (1 + bpp * int(W))
        out.append((off, n))
        off += n
    return out


def encode_png_rows(rows, W, H, bit_depth, colour_type):
    """The PNG file around already filtered scanlines: ``rows`` (bytes-like) holds H rows of one filter byte + the row's
    samples (16-bit samples big-endian).  zlib level 1, one IDAT chunk."""
    W, H, bit_depth, colour_type = int(W), int(H), int(bit_depth), int(colour_type)
    if W < 1 or H < 1 or bit_depth not in (8, 16) or colour_type not in _CHANNELS:
        raise ValueError(f"encode_png_rows: bad header W={W} H={H} bit_depth={bit_depth} colour_type={colour_type}")
    rows = memoryview(rows).cast("B")
    want = H * (1 + W * _CHANNELS[colour_type] * bit_depth // 8)
    if len(rows) != want:
        raise ValueError(f"encode_png_rows: {len(rows)} bytes of scanlines, {W} x {H} needs {want}")
    return b"".join((_PNG_MAGIC, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, colour_type, 0, 0, 0)),
                     _chunk(b"IDAT", zlib.compress(rows, 1)), _chunk(b"IEND", b"")))


class _Job:
    __slots__ = ("kind", "paths", "H", "W", "nbytes", "slot", "event", "host", "done")

    def __init__(self, kind, paths, H, W, nbytes, slot, event=None, host=None):
        self.kind, self.paths, self.H, self.W, self.nbytes = kind, paths, H, W, nbytes
        self.slot, self.event, self.host = slot, event, host
        self.done = threading.Event()


class _Slot:
    __slots__ = ("dev", "host", "event", "job")

    def __init__(self):
        self.dev = self.host = self.event = self.job = None


class EvalExporter:
    """``submit`` / ``submit_sheet`` launch on the CURRENT stream, record an event and return; ``workers`` threads do the
    rest.  ``depth`` ring slots (default 2 * workers), each with one device buffer, one pinned host buffer and one event;
    a slot is reused only after its job has finished on the host.  What a worker raised is re-raised by the next
    ``submit*``, ``wait()`` or ``close()``; the object waits at interpreter exit.  Nothing is allocated and no thread is
    started before the first job."""

    def __init__(self, output_dir, rank=0, workers=6, depth=None):
        if not output_dir:
            raise ValueError("EvalExporter needs an output directory")
        self.output_dir = os.fspath(output_dir)
        self.rank = int(rank)
        self.workers = int(workers)
        self.depth = 2 * self.workers if depth is None else int(depth)
        if self.workers < 1 or self.depth < 1:
            raise ValueError(f"EvalExporter: workers and depth must be positive, got {workers}, {depth}")
        self._slots = [_Slot() for _ in range(self.depth)]
        self._next = 0
        self._queue = queue.Queue()
        self._threads = []
        self._lock = threading.Lock()
        self._error = None
        self._copy_stream = None
        self.closed = False
        self.stats = dict(images=0, stalls=0, stall_ms=0.0, encode_ms=0.0, write_ms=0.0, files=0, bytes=0)
        ref = weakref.ref(self)
        atexit.register(lambda: ref() is not None and ref()._wait_at_exit())

    # ------------------------------------------------------------------ names
    def name(self, eval_index):
        return f"{int(eval_index):06d}_rank{self.rank}.png"

    def plane_paths(self, eval_index):
        """The four files of an ``eval_only`` image, in the pack buffer's plane order."""
        return [os.path.join(self.output_dir, d, self.name(eval_index)) for d, _b, _c, _p in PLANES]

    def sheet_path(self, eval_index, save_name=None):
        return os.path.join(self.output_dir, save_name if save_name else self.name(eval_index))

    # ------------------------------------------------------------------ waiting
    def _raise_pending(self):
        with self._lock:
            err, self._error = self._error, None
        if err is not None:
            raise err

    def wait(self):
        """Blocks until every submitted file is on disk; re-raises what a worker raised."""
        for s in self._slots:
            if s.job is not None:
                s.job.done.wait()
                s.job = None
        self._raise_pending()

    def close(self):
        """Waits, then ends the worker threads."""
        self.closed = True
        try:
            self.wait()
        finally:
            threads, self._threads = self._threads, []
            for _ in threads:
                self._queue.put(None)
            for t in threads:
                t.join()

    def _wait_at_exit(self):
        try:
            self.close()
        except BaseException as e:       # the interpreter is going down: say it, there is nobody left to raise to
            logger.error("eval exporter failed: %r", e)

    # ------------------------------------------------------------------ the caller's share
    def _acquire(self):
        """The next ring slot, free: blocks on the job that still holds it (the oldest one)."""
        if self.closed:
            raise RuntimeError("EvalExporter is closed")
        self._raise_pending()
        slot = self._slots[self._next]
        self._next = (self._next + 1) % self.depth
        job = slot.job
        if job is not None:
            if not job.done.is_set():
                t0 = time.perf_counter()
                self._wait_for(job)
                with self._lock:
                    self.stats["stalls"] += 1
                    self.stats["stall_ms"] += (time.perf_counter() - t0) * 1e3
            slot.job = None
            self._raise_pending()
        return slot

    @staticmethod
    def _wait_for(job):
        job.done.wait()

    def _start(self, job):
        job.slot.job = job
        while len(self._threads) < self.workers:
            t = threading.Thread(target=self._worker, name=f"madm-eval-export-{len(self._threads)}", daemon=True)
            self._threads.append(t)
            t.start()
        self.stats["images"] += 1
        self._queue.put(job)

    @staticmethod
    def _device_buffer(slot, nbytes, device):
        if slot.dev is None or slot.dev.numel() < nbytes or slot.dev.device != device:
            slot.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if slot.event is None:
            slot.event = torch.cuda.Event()
        return slot.dev[:nbytes]

    def submit(self, paths, pred, gt, image, palette, num_classes, ignore_label):
        """One ``eval_only`` image: pred, gt i64 [H, W], image f32 / u8 [3, H, W] (device tensors), ``palette`` the padded
        u8 [768] device palette; ``paths``: the four file names in plane order (``plane_paths``)."""
        from . import ops
        assert len(paths) == len(PLANES)
        H, W = pred.shape
        slot = self._acquire()
        buf = self._device_buffer(slot, pack_bytes(H, W), pred.device)
        ops.eval_export_pack(pred, gt, image, palette, num_classes, ignore_label, out=buf)
        slot.event.record()
        self._start(_Job("packed", list(paths), H, W, buf.numel(), slot, event=slot.event))

    def submit_sheet(self, path, image, pred, gt, palette):
        """One ``image | pred | gt`` sheet (RGB8, H x 3W): a ``vis.compose`` launch of three tiles -- the image with denorm
        (1/255, 0), the prediction and the ground truth as palette tiles -- into a ring slot."""
        H, W = pred.shape[-2:]
        slot = self._acquire()
        buf = self._device_buffer(slot, H * 3 * W * 3, pred.device)
        compose(self.sheet_tiles(image, pred, gt), cols_max=3, palette=palette, out=buf.view(H, 3 * W, 3))
        slot.event.record()
        self._start(_Job("sheet", [path], H, 3 * W, buf.numel(), slot, event=slot.event))

    @staticmethod
    def sheet_tiles(image, pred, gt):
        H, W = pred.shape[-2:]
        return [dict(data_type="image", info="image", data=image.reshape(1, 3, H, W), denorm=(1.0 / 255.0, 0.0)),
                dict(data_type="label", info="pred", data=pred.reshape(1, H, W)),
                dict(data_type="label", info="gt", data=gt.reshape(1, H, W))]

    def submit_packed(self, paths, packed_cpu, H, W):
        """The writer's half alone: a finished pack buffer on the CPU (u8 tensor / array / bytes of H * (4 + 11 W) bytes)."""
        host = memoryview(packed_cpu.numpy() if isinstance(packed_cpu, torch.Tensor) else packed_cpu).cast("B")
        if len(host) != pack_bytes(H, W) or len(paths) != len(PLANES):
            raise ValueError(f"submit_packed: {len(host)} bytes / {len(paths)} names for a {H} x {W} image")
        slot = self._acquire()
        self._start(_Job("packed", list(paths), int(H), int(W), len(host), slot, host=host))

    # ------------------------------------------------------------------ the workers' share
    def _worker(self):
        while True:
            job = self._queue.get()
            if job is None:
                return
            try:
                self._process(job)
            except BaseException as e:
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                job.done.set()

    def _fetch(self, job):
        """The job's bytes on the host: waits for the launch's event on the exporter's copy stream, never on the caller's,
        and copies into the slot's pinned buffer."""
        if job.host is not None:
            return job.host
        slot = job.slot
        dev = slot.dev[:job.nbytes]
        torch.cuda.set_device(dev.device)
        with self._lock:
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=dev.device)
        if slot.host is None or slot.host.numel() < job.nbytes:
            slot.host = torch.empty(slot.dev.numel(), dtype=torch.uint8, pin_memory=True)
        host = slot.host[:job.nbytes]
        copied = torch.cuda.Event()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(job.event)
            host.copy_(dev, non_blocking=True)
            copied.record()
        copied.synchronize()
        return memoryview(host.numpy())

    def _process(self, job):
        host = self._fetch(job)
        t0 = time.perf_counter()
        if job.kind == "sheet":
            files = [(job.paths[0], encode_png(np.frombuffer(host, dtype=np.uint8).reshape(job.H, job.W, 3)))]
        else:
            files = [(path, encode_png_rows(host[off:off + n], job.W, job.H, depth, colour))
                     for path, (off, n), (_d, depth, colour, _b) in zip(job.paths, plane_slices(job.H, job.W), PLANES)]
        t1 = time.perf_counter()
        for path, data in files:
            self._write_file(path, data)
        t2 = time.perf_counter()
        with self._lock:
            self.stats["encode_ms"] += (t1 - t0) * 1e3
            self.stats["write_ms"] += (t2 - t1) * 1e3
            self.stats["files"] += len(files)
            self.stats["bytes"] += sum(len(d) for _p, d in files)

    @staticmethod
    def _write_file(final, data):
        """``data`` under a temporary name, then the rename: the final name never holds a partial file."""
        os.makedirs(os.path.dirname(final), exist_ok=True)
        tmp = os.path.join(os.path.dirname(final), "." + os.path.basename(final) + ".tmp")
        try:
            with open(tmp, "wb") as f:
                f.write(data)
            os.replace(tmp, final)
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise
