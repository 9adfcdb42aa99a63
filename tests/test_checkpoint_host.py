"""Checkpointing without a GPU (madm_amd/checkpoint.py, the state_dict / load_state_dict of optim.py and train.py): file
conventions of the reference's checkpointer, key matching, optimizer state by parameter name, in-place loads, the writer
thread's error path, argument checks of madm_snapshot_f32 and a two-rank gloo run.  Small stand-in modules on CPU tensors;
the device side is tests/test_checkpoint_gpu.py."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOWN_ANSWER = 0x4ca95a287634fdef          # default_rng(0).standard_normal(1027) as float32, index_base 0


def fingerprint_numpy(values, index_base=0):
    """The fingerprint of include/madm_hip.h (madm_snapshot_f32), restated: uint64 arithmetic wraps modulo 2^64."""
    w = np.ascontiguousarray(values, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    x = ((np.arange(w.size, dtype=np.uint64) + np.uint64(index_base)) << np.uint64(32)) | w
    h = x * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(32)
    h = h * np.uint64(0xD6E8FEB86659FD93)
    h ^= h >> np.uint64(32)
    return int(h.sum(dtype=np.uint64))


class TinyModel(torch.nn.Module):
    """MTMADISE's parameter-name families (what MadmTrainer's flat order keys on), a frozen tensor, an EMA teacher and a
    BatchNorm with running statistics."""

    def __init__(self, seed=3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g))
        self.backbone = torch.nn.Module()
        self.backbone.clip_project_rgb = torch.nn.ParameterDict({"prompt_embed": mk(7, 5)})
        unet = torch.nn.Module()
        unet.conv_in = torch.nn.ParameterDict({"weight": mk(40, 50)})
        unet.time_embedding = torch.nn.ParameterDict({"weight": mk(300)})
        unet.frozen = torch.nn.ParameterDict({"weight": mk(64, 64)})
        unet.frozen["weight"].requires_grad = False
        self.backbone.unet = unet
        self.sem_seg_head = torch.nn.ParameterDict({"weight": mk(30, 50), "bias": mk(11)})
        self.bn = torch.nn.BatchNorm1d(6)
        self.bn_sec_modal = self.bn               # one module under two names, as MadmInference.sem_seg_head_sec_modal
        self.ema_sem_seg_head = torch.nn.ParameterDict({"weight": mk(30, 50), "bias": mk(11)})
        for p in self.ema_sem_seg_head.parameters():
            p.requires_grad = False
        self.ema_parms = [self.ema_sem_seg_head]
        self.train_iter_index = 0

    def ignored_state_dict(self):
        return {"backbone.unet.frozen.weight": None}


def make_trainer(model, **kw):
    from madm_amd.train import MadmTrainer
    return MadmTrainer(model, lr=1e-3, weight_decay=0.05, unet_lr=2e-4, **kw)


def scramble_(trainer, seed):
    """Training-like state without a device: moments, step counts, counters, BatchNorm statistics."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for row in trainer.opt.state_dict(trainer.param_names)["state"].values():    # (the alignment padding stays zero)
            row["exp_avg"].copy_(torch.randn(row["exp_avg"].shape, generator=g))
            row["exp_avg_sq"].copy_(torch.rand(row["exp_avg_sq"].shape, generator=g))
        for p in trainer.model.parameters():
            p.add_(torch.randn(p.shape, generator=g))
        trainer.model.bn.running_mean.copy_(torch.randn(6, generator=g))
        trainer.model.bn.num_batches_tracked.fill_(seed)
    trainer.opt.steps = np.arange(len(trainer.opt.params), dtype=np.int64) + seed
    trainer.iter, trainer.scale, trainer._growth_tracker = 40 + seed, 1024.0, 17
    trainer.model.train_iter_index = 41 + seed


def full_state(trainer):
    out = {"model." + k: v.clone() for k, v in trainer.model.state_dict().items()}
    for n, row in trainer.opt.state_dict(trainer.param_names)["state"].items():
        out["m." + n], out["v." + n], out["step." + n] = row["exp_avg"].clone(), row["exp_avg_sq"].clone(), row["step"]
    out.update(iter=trainer.iter, scale=trainer.scale, tracker=trainer._growth_tracker, model_step=trainer.model.train_iter_index)
    return out


def assert_same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


# ----------------------------------------------------------------------------- 1. file conventions
@pytest.mark.parametrize("async_save", [False, True], ids=["inline", "async"])
def test_file_conventions(tmp_path, async_save):
    from madm_amd.checkpoint import MadmCheckpointer, PeriodicCheckpointer
    model = TinyModel()
    trainer = make_trainer(model)
    scramble_(trainer, 1)
    d = str(tmp_path / "out")
    ck = MadmCheckpointer(model, d, async_save=async_save, trainer=trainer)
    assert not ck.has_checkpoint() and ck.get_checkpoint_file() == "" and not MadmCheckpointer.has_checkpoint_in_dir(d)
    per = PeriodicCheckpointer(ck, period=3, max_iter=10, max_to_keep=2)
    for it in range(10):
        per.step(it, note="n%d" % it)
    ck.wait()
    files = sorted(f for f in os.listdir(d) if not f.startswith("."))
    assert files == ["last_checkpoint", "model_0000005.pth", "model_0000008.pth", "model_final.pth"], files   # 0000002 pruned
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
    assert open(os.path.join(d, "last_checkpoint")).read() == "model_final.pth"
    assert ck.has_checkpoint() and ck.get_checkpoint_file() == os.path.join(d, "model_final.pth")
    assert MadmCheckpointer.has_checkpoint_in_dir(d)
    raw = torch.load(os.path.join(d, "model_0000008.pth"), weights_only=True)
    assert raw["iteration"] == 8 and raw["note"] == "n8"
    assert set(raw) == {"model", "trainer", "iteration", "note", "fingerprints", "flat_layout"}
    assert list(raw["model"]) == list(model.state_dict())
    assert set(raw["trainer"]) == {"iteration", "optimizer", "grad_scaler", "model_step", "rng"}
    assert set(raw["trainer"]["rng"]) >= {"python", "numpy", "torch_cpu"}
    assert torch.load(os.path.join(d, "model_final.pth"), weights_only=True)["iteration"] == 9
    # resume_or_load: with resume the file last_checkpoint names and every checkpointable; without: the model only
    want = full_state(trainer)
    m2 = TinyModel(seed=5)
    t2 = make_trainer(m2)
    ck2 = MadmCheckpointer(m2, d, trainer=t2)
    extra = ck2.resume_or_load("/nonexistent/init.pth", resume=True)
    assert extra["iteration"] == 9 and extra["note"] == "n9" and not extra.missing_keys and not extra.unexpected_keys
    assert_same_state(full_state(t2), want)
    m3 = TinyModel(seed=6)
    t3 = make_trainer(m3)
    ck3 = MadmCheckpointer(m3, d, trainer=t3)
    ck3.resume_or_load(os.path.join(d, "model_0000005.pth"), resume=False)
    got = full_state(t3)
    assert all(torch.equal(got[k], want[k]) for k in want if k.startswith("model."))
    assert t3.iter == 0 and all(int(s) == 0 for s in t3.opt.steps) and not bool(t3.opt.m.any())
    assert ck3.resume_or_load("", resume=False) == {}
    with pytest.raises(FileNotFoundError):
        ck3.load(os.path.join(d, "model_0000002.pth"))


def test_failed_write_leaves_no_file_and_non_writing_rank_writes_nothing(tmp_path, monkeypatch):
    from madm_amd.checkpoint import MadmCheckpointer
    model = TinyModel()
    d = str(tmp_path / "a")

    def broken(payload, path):
        with open(path, "wb") as f:
            f.write(b"half a file")
        raise OSError("disk full")

    ck = MadmCheckpointer(model, d, async_save=False)
    monkeypatch.setattr(MadmCheckpointer, "_torch_save", staticmethod(broken))
    with pytest.raises(OSError, match="disk full"):
        ck.save("model_0000001")
    assert not os.path.exists(os.path.join(d, "model_0000001.pth")) and not ck.has_checkpoint()
    assert not [f for f in os.listdir(d) if "model_0000001" in f]
    monkeypatch.undo()
    quiet = MadmCheckpointer(model, str(tmp_path / "b"), save_to_disk=False)
    quiet.save("model_0000001")
    quiet.wait()
    assert not os.path.exists(str(tmp_path / "b"))


# ----------------------------------------------------------------------------- 2. key matching
def test_key_matching_and_keep_filter(tmp_path):
    from madm_amd.checkpoint import MadmCheckpointer
    model = TinyModel()
    sd = {"module." + k: v.clone() + 1 for k, v in model.state_dict().items()}        # a DDP-wrapped model's file
    sd.pop("module.backbone.unet.frozen.weight")                                      # ignored_state_dict: not "missing"
    sd.pop("module.sem_seg_head.bias")
    sd["module.not.in.the.model"] = torch.zeros(2)
    torch.save({"model": sd, "iteration": 7}, str(tmp_path / "ddp.pth"))
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ck = MadmCheckpointer(model, str(tmp_path))
    res = ck.load(str(tmp_path / "ddp.pth"))
    assert res == {"iteration": 7}
    assert res.missing_keys == ["sem_seg_head.bias"] and res.unexpected_keys == ["not.in.the.model"]
    for k, v in model.state_dict().items():
        moved = k not in ("backbone.unet.frozen.weight", "sem_seg_head.bias")
        assert torch.equal(v, before[k] + 1 if moved else before[k]), k
    bad = {k: v.clone() for k, v in model.state_dict().items()}
    bad["backbone.unet.conv_in.weight"] = torch.zeros(50, 40)
    torch.save({"model": bad}, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError, match=r"backbone\.unet\.conv_in\.weight"):
        ck.load(str(tmp_path / "bad.pth"))
    # keep: what it leaves out comes back as missing keys
    kept = MadmCheckpointer(model, str(tmp_path / "k"), async_save=False, keep=lambda n, t: n.startswith("sem_seg_head."))
    assert set(kept.model_entries()) == {"sem_seg_head.weight", "sem_seg_head.bias"}
    kept.save("m")
    assert set(torch.load(str(tmp_path / "k" / "m.pth"), weights_only=True)["model"]) == set(kept.model_entries())
    res = kept.load(str(tmp_path / "k" / "m.pth"))
    assert "bn.running_mean" in res.missing_keys and "sem_seg_head.weight" not in res.missing_keys
    assert "backbone.unet.frozen.weight" not in res.missing_keys


@pytest.mark.parametrize("async_save", [False, True], ids=["inline", "async"])
def test_keep_filter_shrinks_the_file_of_flat_views(tmp_path, async_save):
    """torch.save writes the whole storage behind a view: a kept 11-element bias that is a view of a ~4 MB flat buffer must
    cost its own bytes plus the pickle's overhead, not the buffer's."""
    from madm_amd.checkpoint import MadmCheckpointer
    model = TinyModel()
    model.backbone.unet.conv_in["weight"] = torch.nn.Parameter(torch.zeros(1000, 1000))
    trainer = make_trainer(model)
    assert trainer.opt.flat.flat.numel() * 4 > 4_000_000
    p = model.sem_seg_head["bias"]
    assert p.untyped_storage().nbytes() == trainer.opt.flat.flat.numel() * 4       # (it IS a view of the flat buffer)
    ck = MadmCheckpointer(model, str(tmp_path), async_save=async_save, keep=lambda n, t: n == "sem_seg_head.bias")
    ck.save("small")
    ck.wait()
    size = os.path.getsize(str(tmp_path / "small.pth"))
    assert p.numel() * 4 <= size <= p.numel() * 4 + 8192, size
    got = torch.load(str(tmp_path / "small.pth"), weights_only=True)["model"]
    assert list(got) == ["sem_seg_head.bias"] and torch.equal(got["sem_seg_head.bias"], p.detach())


# ----------------------------------------------------------------------------- 3. optimizer state by name
def _table(params, order):
    return [(params[n], 1e-3 * (1 + i), 0.01 * i) for i, n in order]


def test_table_adamw_state_is_keyed_by_name():
    from madm_amd.optim import TableAdamW
    shapes = {"a.weight": (3, 500), "b.bias": (7,), "c.weight": (40, 40), "d.gate": (1,)}
    hyper = {n: i for i, n in enumerate(shapes)}

    def build(order, seed):
        g = torch.Generator().manual_seed(seed)
        params = {n: torch.nn.Parameter(torch.randn(*s, generator=g)) for n, s in shapes.items()}
        opt = TableAdamW(_table(params, [(hyper[n], n) for n in order]))
        return opt, params

    order_a, order_b = list(shapes), ["c.weight", "d.gate", "a.weight", "b.bias"]
    a, _ = build(order_a, 0)
    g = torch.Generator().manual_seed(9)
    a.m.copy_(torch.randn(a.m.shape, generator=g))
    a.v.copy_(torch.rand(a.v.shape, generator=g))
    a.steps = np.asarray([5, 0, 12, 3], dtype=np.int64)
    sd = a.state_dict(order_a)
    assert set(sd) == {"state", "betas", "eps", "lr", "weight_decay"} and set(sd["state"]) == set(shapes)
    assert all(set(row) == {"exp_avg", "exp_avg_sq", "step"} for row in sd["state"].values())
    b, _ = build(order_b, 1)
    assert dict(zip(order_b, b.flat.offsets)) != dict(zip(order_a, a.flat.offsets))      # every tensor sits elsewhere
    m_ptr, v_ptr = b.m.data_ptr(), b.v.data_ptr()
    b.load_state_dict(sd, order_b)
    assert (b.m.data_ptr(), b.v.data_ptr()) == (m_ptr, v_ptr)
    back = b.state_dict(order_b)
    for n in shapes:
        assert torch.equal(back["state"][n]["exp_avg"], sd["state"][n]["exp_avg"]), n
        assert torch.equal(back["state"][n]["exp_avg_sq"], sd["state"][n]["exp_avg_sq"]), n
        assert back["state"][n]["step"] == sd["state"][n]["step"]
        assert back["state"][n]["exp_avg"].shape == shapes[n]
    assert dict(zip(order_b, b.steps.tolist())) == dict(zip(order_a, [5, 0, 12, 3]))
    # hyper-parameter mismatches and foreign names raise
    for key, val in (("eps", 1e-6), ("betas", [0.8, 0.999])):
        with pytest.raises(ValueError, match=key):
            b.load_state_dict(dict(sd, **{key: val}), order_b)
    with pytest.raises(ValueError, match="lr"):
        b.load_state_dict(dict(sd, lr=dict(sd["lr"], **{"b.bias": 0.5})), order_b)
    with pytest.raises(ValueError, match="weight_decay"):
        b.load_state_dict(dict(sd, weight_decay=dict(sd["weight_decay"], **{"b.bias": 0.5})), order_b)
    with pytest.raises(ValueError, match="names"):
        b.load_state_dict(sd, ["c.weight", "d.gate", "a.weight", "x.bias"])


def test_flat_adamw_state_round_trip():
    from madm_amd.optim import FlatParams, FlatAdamW
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(9))]
    a = FlatAdamW(FlatParams(ps, with_grad=False), lr=1e-3)
    a.m.normal_()
    a.v.uniform_()
    a.step_count = 4
    sd = a.state_dict(["w", "b"])
    qs = [torch.nn.Parameter(torch.randn(9)), torch.nn.Parameter(torch.randn(5, 3))]
    b = FlatAdamW(FlatParams(qs, with_grad=False), lr=1e-3)
    b.load_state_dict(sd, ["b", "w"])
    assert b.step_count == 4 and torch.equal(b.state_dict(["b", "w"])["state"]["w"]["exp_avg"], sd["state"]["w"]["exp_avg"])
    with pytest.raises(ValueError, match="lr"):
        FlatAdamW(FlatParams(qs, with_grad=False), lr=2e-3).load_state_dict(sd, ["b", "w"])


# ----------------------------------------------------------------------------- 4. in-place load
def test_load_writes_into_the_flat_storage(tmp_path):
    from madm_amd.checkpoint import MadmCheckpointer
    src_model = TinyModel()
    src = make_trainer(src_model)
    scramble_(src, 2)
    ck = MadmCheckpointer(src_model, str(tmp_path), async_save=False, trainer=src)
    ck.save("model_0000001", iteration=1)
    model = TinyModel(seed=8)
    trainer = make_trainer(model)
    flat = trainer.opt.flat.flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    ptrs = {n: p.data_ptr() for n, p in model.named_parameters()}
    versions = {n: p._version for n, p in model.named_parameters()}
    bversions = {n: b._version for n, b in model.named_buffers()}
    grads = {n: p.grad.data_ptr() for n, p in model.named_parameters() if p.requires_grad}
    MadmCheckpointer(model, str(tmp_path), trainer=trainer).resume_or_load("", resume=True)
    for n, p in model.named_parameters():
        assert p.data_ptr() == ptrs[n], n
        assert p._version > versions[n], n
        if p.requires_grad:
            assert lo <= p.data_ptr() < hi and p.grad.data_ptr() == grads[n], n
    assert all(b._version > bversions[n] for n, b in model.named_buffers())
    assert_same_state(full_state(trainer), full_state(src))
    # the optimizer still owns the model: a write through the flat buffer is seen by the parameters
    with torch.no_grad():
        flat.fill_(0.25)
    assert all(bool((p == 0.25).all()) for p in model.parameters() if p.requires_grad)
    assert trainer.state_fingerprints() != src.state_fingerprints()
    # RNG states came back: the next draws of the four host-visible generators agree
    import random
    src_rng = torch.load(str(tmp_path / "model_0000001.pth"), weights_only=True)["trainer"]["rng"]
    trainer.set_rng_state(src_rng)
    a = (random.random(), np.random.rand(), torch.rand(3))
    trainer.set_rng_state(src_rng)
    b = (random.random(), np.random.rand(), torch.rand(3))
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])


def test_load_time_verification_names_the_buffer(tmp_path):
    from madm_amd.checkpoint import MadmCheckpointer
    model = TinyModel()
    trainer = make_trainer(model)
    scramble_(trainer, 3)
    ck = MadmCheckpointer(model, str(tmp_path), async_save=False, trainer=trainer)
    ck.save("m")
    raw = torch.load(str(tmp_path / "m.pth"), weights_only=True)
    assert raw["fingerprints"]["param"] == "0x%016x" % fingerprint_numpy(trainer.opt.flat.flat.numpy())
    raw["trainer"]["optimizer"]["state"]["sem_seg_head.bias"]["exp_avg_sq"][3] += 1.0
    torch.save(raw, str(tmp_path / "altered.pth"))
    with pytest.raises(RuntimeError, match="'exp_avg_sq'"):
        ck.load(str(tmp_path / "altered.pth"))
    ck.load(str(tmp_path / "m.pth"))


# ----------------------------------------------------------------------------- 5. the product model's keys
def test_checkpoint_model_keys_match_the_reference_names():
    from test_bridge import _product_model, reference_names
    from madm_amd.checkpoint import MadmCheckpointer
    got = MadmCheckpointer(_product_model(), "").model_entries()
    want = {k: tuple(v) for k, v in reference_names()["meta_arch_depth"].items()}
    skip = ("shared_noise", "uncond_inputs", "num_batches_tracked")
    for k, shp in want.items():
        if any(s in k for s in skip):
            continue
        assert k in got, f"missing key {k}"
        assert got[k] == shp, (k, got[k], shp)
    extra = [k for k in got if k not in want and not any(s in k for s in skip)]
    assert not extra, extra[:8]


# ----------------------------------------------------------------------------- 6. writer-thread failure
def test_writer_thread_failure_surfaces(tmp_path):
    from madm_amd.checkpoint import MadmCheckpointer
    blocker = tmp_path / "dir"
    blocker.write_text("a plain file where the save directory should be")
    model = TinyModel()
    ck = MadmCheckpointer(model, str(blocker), async_save=True)
    ck.save("model_0000001")                       # returns: the failure happens on the writer thread
    with pytest.raises(OSError):
        ck.wait()
    ck.wait()                                      # reported once
    ck.save("model_0000002")
    with pytest.raises(OSError):
        ck.save("model_0000003")                   # the next save reports the previous one's failure
    ck.wait()


def test_async_save_holds_the_state_of_the_call(tmp_path):
    """What ``save`` returns with is what the file holds, whatever the caller overwrites next -- also for a buffer that
    state_dict() lists under two names."""
    from madm_amd.checkpoint import MadmCheckpointer
    model = TinyModel()
    trainer = make_trainer(model)
    scramble_(trainer, 6)
    want = full_state(trainer)
    ck = MadmCheckpointer(model, str(tmp_path), async_save=True, trainer=trainer)
    ck.save("m")
    with torch.no_grad():
        trainer.opt.flat.flat.fill_(7.0)
        trainer.opt.m.fill_(-3.0)
        trainer.opt.v.fill_(9.0)
        for t in list(model.buffers()) + list(model.ema_sem_seg_head.parameters()):
            t.fill_(2)
    ck.wait()
    raw = torch.load(str(tmp_path / "m.pth"), weights_only=True)
    assert "bn_sec_modal.running_mean" in raw["model"]
    for k, v in raw["model"].items():
        if k != "backbone.unet.frozen.weight":
            assert torch.equal(v, want["model." + k]), k
    for n, row in raw["trainer"]["optimizer"]["state"].items():
        assert torch.equal(row["exp_avg"], want["m." + n]) and torch.equal(row["exp_avg_sq"], want["v." + n]), n


# ----------------------------------------------------------------------------- 7. the C ABI's argument checks
def test_snapshot_export_refuses_bad_arguments():
    from madm_amd._lib import lib
    buf = (ctypes.c_float * 16)()
    fp = ctypes.c_ulonglong(0)
    a = ctypes.addressof(buf)
    a += (-a) % 16
    f = ctypes.addressof(fp)
    ok_src, ok_dst = ctypes.c_void_p(a), ctypes.c_void_p(a + 16)
    cases = {
        "null src": (None, ok_dst, 4, 0, f),
        "no output": (ok_src, None, 4, 0, None),
        "n == 0": (ok_src, ok_dst, 0, 0, f),
        "misaligned src": (ctypes.c_void_p(a + 4), ok_dst, 4, 0, f),
        "misaligned dst": (ok_src, ctypes.c_void_p(a + 20), 4, 0, f),
        "index overflow": (ok_src, ok_dst, 4, (1 << 32) - 3, f),
        "index_base beyond 2^32": (ok_src, ok_dst, 4, (1 << 63), f),
    }
    for what, (src, dst, n, base, fpp) in cases.items():
        rc = lib.madm_snapshot_f32(src, dst, n, base, ctypes.c_void_p(fpp) if fpp else None, None)
        assert rc == -1, what
        assert b"snapshot_f32" in lib.madm_last_error(), what
    assert fp.value == 0 and lib.madm_abi_version() == 6


def test_fingerprint_known_answer_and_properties():
    from madm_amd.optim import fingerprint_host
    x = np.random.default_rng(0).standard_normal(1027).astype(np.float32)
    assert fingerprint_numpy(x) == KNOWN_ANSWER
    assert fingerprint_host(x) == KNOWN_ANSWER and fingerprint_host(torch.from_numpy(x)) == KNOWN_ANSWER
    assert fingerprint_host(x, 12345) == fingerprint_numpy(x, 12345) != KNOWN_ANSWER
    # the sum of the pieces, with their index_base
    assert (fingerprint_numpy(x[:500]) + fingerprint_numpy(x[500:], 500)) % (1 << 64) == KNOWN_ANSWER
    # bit patterns: -0.0 differs from 0.0, a swap of unequal elements is seen
    z = np.zeros(8, dtype=np.float32)
    nz = z.copy()
    nz[3] = -0.0
    assert fingerprint_numpy(z) != fingerprint_numpy(nz)
    y = x.copy()
    y[[10, 900]] = y[[900, 10]]
    assert fingerprint_numpy(y) != KNOWN_ANSWER


# ----------------------------------------------------------------------------- 8. two ranks, gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ckpt_worker(rank, world, port, save_dir, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from madm_amd import dist as mdist
    from madm_amd.checkpoint import MadmCheckpointer, PeriodicCheckpointer
    d = mdist.init(backend="gloo")
    model = TinyModel(seed=3 + rank)
    tr = make_trainer(model, dist=d)               # rank 0's parameters and buffers are broadcast
    scramble_(tr, 4)                               # (the same seed on both ranks: replicas agree)
    in_sync = tr.replicas_in_sync()
    my_dir = os.path.join(save_dir, "run")
    ck = MadmCheckpointer(model, my_dir, trainer=tr)
    per = PeriodicCheckpointer(ck, period=2, max_iter=4)
    for it in range(4):
        per.step(it)
    ck.wait()
    wrote = ck.save_to_disk
    d.barrier()
    listing = sorted(os.listdir(my_dir))
    # both ranks load rank 0's file into a fresh, DIFFERENT state
    m2 = TinyModel(seed=20 + rank)
    from madm_amd.train import MadmTrainer
    t2 = MadmTrainer(m2, lr=1e-3, weight_decay=0.05, unet_lr=2e-4)
    scramble_(t2, 10 + rank)
    res = MadmCheckpointer(m2, my_dir, save_to_disk=False, trainer=t2).resume_or_load("", resume=True)
    fps = t2.state_fingerprints()
    # a diverged replica is caught on every rank before anything is written
    if rank == 1:
        with torch.no_grad():
            model.sem_seg_head["bias"][2] += 1e-3
    diverged_seen = not tr.replicas_in_sync()
    raised = False
    try:
        PeriodicCheckpointer(ck, period=1).step(100)
    except RuntimeError as e:
        raised = "replicas" in str(e)
    ck.wait()
    q.put((rank, in_sync, wrote, listing, res["iteration"], {k: int(v) for k, v in fps.items()}, t2.iter, diverged_seen, raised,
           sorted(os.listdir(my_dir))))
    d.barrier()
    d.destroy_process_group()


def test_two_rank_gloo_checkpoint(tmp_path):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ckpt_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    r0, r1 = res
    assert r0[1] and r1[1]                                   # replicas in sync after the start-up broadcast
    assert r0[2] and not r1[2]                               # only rank 0 writes
    assert r0[3] == r1[3] == ["last_checkpoint", "model_0000001.pth", "model_0000003.pth", "model_final.pth"]
    assert r0[4] == r1[4] == 3
    assert r0[5] == r1[5] and r0[6] == r1[6] == 44           # equal state on both ranks after the load
    assert r0[7] and r1[7] and r0[8] and r1[8]               # divergence seen and raised on BOTH ranks ...
    assert r0[9] == r1[9] == r0[3]                           # ... and nothing was written
