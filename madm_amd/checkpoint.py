"""Training checkpoints: ``MadmCheckpointer`` / ``PeriodicCheckpointer`` with the surface and the on-disk conventions of
the reference's ``ODISECheckpointer`` (checkpoint/odise_checkpointer.py, fvcore's ``Checkpointer`` through detectron2) and
``hooks.PeriodicCheckpointer`` (main.py:296-343, config_files/common/train.py:15).  Neither package is a dependency here:
this is a restatement of their file conventions --

    <save_dir>/<name>.pth      {"model": model.state_dict(), "<key>": obj.state_dict() per checkpointable, **extra}
    <save_dir>/last_checkpoint the base name of the file written last

-- so a file written here loads into the reference model by name and a released ``model_RGB2*.pth`` loads here.

What is new is WHEN the bytes are taken.  The bulk of the state lives in a handful of flat fp32 device buffers
(``MadmTrainer.flat_buffers``: parameters, AdamW's two moments, the EMA teacher); ``save`` snapshots each of them with one
``madm_snapshot_f32`` launch (copy into a device staging buffer + the buffer's fingerprint, in the same read) on the
training stream, clones the model's buffers (BatchNorm running statistics: the next step changes them), takes the
host-side state (counters, loss scale, generator states) and records an event.  Everything after that -- the copy to the
host, the per-name views, ``torch.save``, the rename, ``last_checkpoint``, pruning -- runs on ONE writer thread with ONE
stream of its own (``async_save=True``) or in line (``async_save=False``: the same code).  Call ``wait()`` before the
process exits or the file is read."""
import atexit
import copy
import logging
import os
import threading
import weakref

import torch

logger = logging.getLogger("madm_amd.checkpoint")

class LoadResult(dict):
    """What ``load`` returns: the file's extra entries (``iteration``, ...) as a dict, with the model's key report."""
    missing_keys = ()
    unexpected_keys = ()


def _strip_module_prefix(sd):
    """A DistributedDataParallel-wrapped model's file: every key starts with ``module.``."""
    if sd and all(k.startswith("module.") for k in sd):
        return {k[len("module."):]: v for k, v in sd.items()}
    return sd


def _owns_compact_storage(t):
    return t.untyped_storage().nbytes() == t.numel() * t.element_size()


class MadmCheckpointer:
    def __init__(self, model, save_dir="", *, save_to_disk=None, async_save=True, keep=None, **checkpointables):
        """``keep``: callable(name, tensor) -> bool restricting which model entries ``save`` writes (what it leaves out comes
        back as missing keys on load).  ``save_to_disk`` None: rank 0 of the trainer's process group, True without one."""
        self.model = model
        self.save_dir = save_dir
        self.checkpointables = dict(checkpointables)
        self.keep = keep
        self.async_save = bool(async_save)
        self._trainer = next((o for o in self.checkpointables.values() if hasattr(o, "flat_buffers")), None)
        if save_to_disk is None:
            d = getattr(self._trainer, "dist", None)
            save_to_disk = True if d is None or not d.is_initialized() else d.get_rank() == 0
        self.save_to_disk = bool(save_to_disk)
        self._staging = {}            # buffer name -> device copy (allocated on first use, kept)
        self._host = {}               # buffer name -> pinned host copy
        self._fp = None               # one int64 per flat buffer (uint64 bit patterns)
        self._copy_stream = None
        self._thread = None
        self._error = None
        self.last_save_device_ms = None
        ref = weakref.ref(self)
        atexit.register(lambda: ref() is not None and ref()._wait_at_exit())

    # ------------------------------------------------------------------ file conventions
    def has_checkpoint(self):
        return self.has_checkpoint_in_dir(self.save_dir)

    @staticmethod
    def has_checkpoint_in_dir(save_dir):
        return os.path.exists(os.path.join(save_dir, "last_checkpoint"))

    def get_checkpoint_file(self):
        try:
            with open(os.path.join(self.save_dir, "last_checkpoint")) as f:
                last = f.read().strip()
        except IOError:
            return ""
        return os.path.join(self.save_dir, last)

    def tag_last_checkpoint(self, basename):
        tmp = os.path.join(self.save_dir, ".last_checkpoint.tmp")
        with open(tmp, "w") as f:
            f.write(basename)
        os.replace(tmp, os.path.join(self.save_dir, "last_checkpoint"))

    def model_entries(self):
        """{key: shape} of the ``model`` entry a file written now would hold (``keep`` applied)."""
        return {k: tuple(t.shape) for k, t in self.model.state_dict().items() if self.keep is None or self.keep(k, t)}

    # ------------------------------------------------------------------ save
    def wait(self):
        """Blocks until the pending write is on disk; re-raises what the writer raised."""
        t = self._thread
        if t is not None:
            t.join()
            self._thread = None
        err, self._error = self._error, None
        if err is not None:
            raise err

    def _wait_at_exit(self):
        try:
            self.wait()
        except BaseException as e:       # the interpreter is going down: say it, there is nobody left to raise to
            logger.error("checkpoint writer failed: %r", e)

    def save(self, name, **extra):
        self._save(name, extra, None)

    def _save(self, name, extra, on_written):
        self.wait()                   # one set of staging buffers: a pending write finishes first (and reports its error)
        if not self.save_to_disk:
            return
        job = self._capture(name, extra, on_written)
        if self.async_save:
            self._thread = threading.Thread(target=self._writer_entry, args=(job,), name="madm-checkpoint-writer")
            self._thread.start()
        else:
            self._write(job)

    def _capture(self, name, extra, on_written):
        """The training thread's share: everything that has to be consistent with the step boundary."""
        tr = self._trainer
        flats = {}
        if tr is not None:
            flats = {k: v for k, v in tr.flat_buffers().items()}
        cuda_flats = {k: v for k, v in flats.items() if v[0].is_cuda}
        job = dict(name=name, extra=extra, on_written=on_written, event=None, device=None, flats=flats, host_now={})
        ev = None
        if cuda_flats:
            from . import optim
            dev = next(iter(cuda_flats.values()))[0].device
            job["device"] = dev
            if self._fp is None or self._fp.numel() != len(cuda_flats):
                self._fp = torch.zeros(len(cuda_flats), dtype=torch.int64, device=dev)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            self._fp.zero_()
            for j, (k, (t, _n, _o, _s)) in enumerate(cuda_flats.items()):
                st = self._staging.get(k)
                if st is None or st.numel() != t.numel() or st.device != t.device:
                    st = self._staging[k] = torch.empty_like(t)
                optim.snapshot(t, st, self._fp[j:j + 1])
            job["fp_order"] = list(cuda_flats)
        for k, (t, _n, _o, _s) in flats.items():
            if not t.is_cuda:         # a CPU trainer (tests, gloo): a plain copy stands in for the snapshot launch
                job["host_now"][k] = t.detach().clone()
        # the model's entries: views of a flat buffer are re-viewed from the snapshot by the writer; what the next step
        # changes outside them (BatchNorm running statistics, counters; trainable or teacher tensors that are in no flat
        # buffer) is cloned here; the rest is frozen and the writer reads it directly
        spans = []
        for k, (t, _n, _o, _s) in flats.items():
            if k in ("param", "teacher"):
                spans.append((k, t.data_ptr(), t.data_ptr() + t.numel() * 4))
        # (by storage address, not by name: a module registered under two names -- sem_seg_head_sec_modal -- appears under both
        # in state_dict() but once in named_buffers())
        moving = {b.data_ptr() for b in self.model.buffers()}
        teacher = {id(p) for m in getattr(self.model, "ema_parms", ()) for p in m.parameters()}
        moving |= {p.data_ptr() for p in self.model.parameters() if id(p) in teacher or p.requires_grad}
        plan = []
        for key, t in self.model.state_dict().items():
            if self.keep is not None and not self.keep(key, t):
                continue
            where = next((s for s in spans if s[1] <= t.data_ptr() < s[2]), None) if t.dtype == torch.float32 and t.numel() else None
            if where is not None:
                assert t.is_contiguous()
                plan.append((key, "flat", where[0], (t.data_ptr() - where[1]) // 4, tuple(t.shape)))
            elif t.data_ptr() in moving or tr is None:
                plan.append((key, "value", t.detach().clone(), None, None))
            else:
                plan.append((key, "value", t.detach(), None, None))
        job["plan"] = plan
        # host-side state of the checkpointables; the trainer's moments come from the snapshot
        others = {}
        for key, obj in self.checkpointables.items():
            if obj is tr:
                others[key] = obj.state_dict(tensors=False)
            else:
                others[key] = copy.deepcopy(obj.state_dict())
        job["others"] = others
        job["layout"] = tr.flat_layout_signature() if tr is not None else None
        if ev is not None:
            ev[1].record()
            job["event"] = ev
        return job

    def _writer_entry(self, job):
        try:
            self._write(job)
        except BaseException as e:
            self._error = e

    def _write(self, job):
        tr = self._trainer
        host = dict(job["host_now"])
        fps = {}
        if job["event"] is not None:
            dev = job["device"]
            torch.cuda.set_device(dev)
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=dev)
            job["event"][1].synchronize()
            self.last_save_device_ms = job["event"][0].elapsed_time(job["event"][1])
            with torch.cuda.stream(self._copy_stream):
                for k in job["fp_order"]:
                    st = self._staging[k]
                    hb = self._host.get(k)
                    if hb is None or hb.numel() != st.numel():
                        hb = self._host[k] = torch.empty(st.numel(), dtype=torch.float32, pin_memory=True)
                    hb.copy_(st, non_blocking=True)
                    host[k] = hb
                fp_host = self._fp.to("cpu", non_blocking=False)
                self._copy_stream.synchronize()
            fps = {k: "0x%016x" % (int(v) & ((1 << 64) - 1)) for k, v in zip(job["fp_order"], fp_host.tolist())}
        if job["host_now"]:
            from . import optim
            for k, t in job["host_now"].items():
                fps[k] = "0x%016x" % optim.fingerprint_host(t)
        compact = self.keep is not None      # a filtered file must not carry the whole flat storage behind a small view
        model_sd = {}
        ctx = torch.cuda.stream(self._copy_stream) if job["event"] is not None else _Null()
        with ctx:
            for key, kind, a, off, shape in job["plan"]:
                if kind == "flat":
                    numel = 1
                    for s in shape:
                        numel *= s
                    v = host[a][off:off + numel].view(shape)
                    model_sd[key] = v.clone() if compact else v
                else:
                    v = a.cpu()
                    model_sd[key] = v if _owns_compact_storage(v) else v.clone()
        payload = {"model": model_sd}
        for key, sd in job["others"].items():
            if self.checkpointables[key] is tr:
                mom = tr.opt.state_dict(tr.param_names, m=host["exp_avg"], v=host["exp_avg_sq"])["state"]
                for n, row in sd["optimizer"]["state"].items():
                    row["exp_avg"], row["exp_avg_sq"] = mom[n]["exp_avg"], mom[n]["exp_avg_sq"]
            payload[key] = sd
        if fps:
            payload["fingerprints"] = fps
            payload["flat_layout"] = job["layout"]
        payload.update(job["extra"])
        os.makedirs(self.save_dir, exist_ok=True)
        basename = f"{job['name']}.pth"
        final = os.path.join(self.save_dir, basename)
        tmp = os.path.join(self.save_dir, f".{basename}.tmp")
        try:
            self._torch_save(payload, tmp)
            os.replace(tmp, final)        # an interrupted save never leaves a truncated file under the final name
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise
        self.tag_last_checkpoint(basename)
        if job["on_written"] is not None:
            job["on_written"](final)

    @staticmethod
    def _torch_save(payload, path):
        torch.save(payload, path)

    # ------------------------------------------------------------------ load
    def resume_or_load(self, path, *, resume=True):
        """``resume`` and a ``last_checkpoint`` in ``save_dir``: load that file with every checkpointable; otherwise the
        model only from ``path`` (main.py:331-337)."""
        if resume and self.has_checkpoint():
            return self.load(self.get_checkpoint_file())
        return self.load(path, checkpointables=[])

    def load(self, path, checkpointables=None):
        self.wait()
        if not path:
            logger.info("no checkpoint given: the model keeps its initialisation")
            return LoadResult()
        if not os.path.isfile(path):
            raise FileNotFoundError(f"checkpoint {path} not found")
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        if "model" not in ckpt:           # a bare state_dict
            ckpt = {"model": ckpt}
        missing, unexpected = self._load_model(ckpt.pop("model"))
        loaded_trainer = False
        for key in (self.checkpointables if checkpointables is None else checkpointables):
            if key in ckpt:
                self.checkpointables[key].load_state_dict(ckpt.pop(key))
                loaded_trainer |= self.checkpointables[key] is self._trainer
        fps, layout = ckpt.pop("fingerprints", None), ckpt.pop("flat_layout", None)
        if fps is not None and loaded_trainer:
            self._verify(fps, layout, set(missing))
        out = LoadResult(ckpt)
        out.missing_keys, out.unexpected_keys = missing, unexpected
        return out

    def _load_model(self, sd):
        sd = _strip_module_prefix(dict(sd))
        live = self.model.state_dict()        # detached aliases of the live storage: copy_ writes INTO it
        touched = []
        with torch.no_grad():
            for k, dst in live.items():
                if k not in sd:
                    continue
                src = sd[k]
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"checkpoint entry {k} has shape {tuple(src.shape)}, the model's is {tuple(dst.shape)}")
                dst.copy_(src)
                touched.append(dst)
        # (copy_ through an alias moves the shared version counter already; raw-pointer consumers -- packed operands keyed
        # on the counter -- get one more move, as TableAdamW.step does after its kernel)
        params = [p for p in self.model.parameters()]
        if params:
            torch.autograd.graph.increment_version(params)
        missing = [k for k in live if k not in sd]
        unexpected = [k for k in sd if k not in live]
        if missing and hasattr(self.model, "ignored_state_dict"):
            ignored = set(self.model.ignored_state_dict().keys())
            removed = [k for k in missing if k in ignored]
            if removed:
                logger.warning("removed %d ignored_state_dict keys from the missing keys", len(removed))
            missing = [k for k in missing if k not in ignored]
        if missing:
            logger.warning("keys of the model that the checkpoint does not hold: %d (%s ...)", len(missing), missing[:3])
        if unexpected:
            logger.warning("keys of the checkpoint that the model does not have: %d (%s ...)", len(unexpected), unexpected[:3])
        return missing, unexpected

    def _verify(self, stored, layout, missing):
        """Recomputes the fingerprints from the LIVE buffers after a load and compares them with the file's."""
        tr = self._trainer
        mine = tr.flat_layout_signature()
        live = None
        for k, want in stored.items():
            if k not in mine or layout is None or layout.get(k) != mine[k]:
                logger.info("flat layout of buffer %r differs from the checkpoint's: fingerprint check skipped", k)
                continue
            if k in ("param", "teacher") and missing & set(tr.flat_buffers()[k][1]):
                logger.info("buffer %r was loaded in part only: fingerprint check skipped", k)
                continue
            if live is None:
                live = tr.state_fingerprints()
            if int(want, 16) != live[k]:
                raise RuntimeError(f"checkpoint verification failed: fingerprint of buffer {k!r} after the load is "
                                   f"0x{live[k]:016x}, the file recorded {want}")


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class PeriodicCheckpointer:
    """hooks.PeriodicCheckpointer / fvcore's PeriodicCheckpointer: ``<prefix>_{iteration:07d}.pth`` whenever
    ``(iteration + 1) % period == 0``, ``<prefix>_final.pth`` at ``max_iter - 1``, ``iteration`` stored in the file, older
    periodic files removed beyond ``max_to_keep`` (never the final one).  Every rank calls ``step``."""

    def __init__(self, checkpointer, period, max_iter=None, max_to_keep=None, file_prefix="model"):
        if max_to_keep is not None:
            assert max_to_keep > 0
        self.checkpointer = checkpointer
        self.period = int(period)
        self.max_iter = max_iter
        self.max_to_keep = max_to_keep
        self.file_prefix = file_prefix
        self.recent_checkpoints = []

    def _check_replicas(self):
        tr = self.checkpointer._trainer
        if tr is not None and getattr(tr, "dist", None) is not None and not tr.replicas_in_sync():
            raise RuntimeError("data-parallel replicas hold different parameters (parameter fingerprints differ between "
                               "ranks): nothing was written")

    def _written(self, path):
        if self.max_to_keep is None:
            return
        self.recent_checkpoints.append(path)
        while len(self.recent_checkpoints) > self.max_to_keep:
            old = self.recent_checkpoints.pop(0)
            if os.path.exists(old) and not old.endswith(f"{self.file_prefix}_final.pth"):
                os.remove(old)

    def step(self, iteration, **extra):
        iteration = int(iteration)
        state = {"iteration": iteration}
        state.update(extra)
        if (iteration + 1) % self.period == 0:
            self._check_replicas()
            self.checkpointer._save(f"{self.file_prefix}_{iteration:07d}", state, self._written)
        if self.max_iter is not None and iteration >= self.max_iter - 1:
            self._check_replicas()
            self.checkpointer._save(f"{self.file_prefix}_final", state, None)

    def save(self, name, **extra):
        self.checkpointer.save(name, **extra)
