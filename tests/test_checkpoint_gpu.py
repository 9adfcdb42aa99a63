"""Checkpointing on the device: the snapshot / fingerprint kernel against its numpy restatement, a bitwise round trip of
the whole training state, continuity of a resumed run, isolation of an asynchronous save from the steps that follow it,
load-time verification and the process-group path.  The trainer tests use the adapters-only variant
(``train_depth_lora_only``) with a ``keep`` filter that leaves the frozen pretrained tensors out, so every file stays small;
everything is written under ``tmp_path``."""
import os
import random

import numpy as np
import pytest
import torch

from golden_util import TRAIN_CASE, train_inputs
from test_train_gpu import build_product_train
from test_checkpoint_host import fingerprint_numpy, KNOWN_ANSWER

pytestmark = pytest.mark.gpu
MASK = (1 << 64) - 1


# ----------------------------------------------------------------------------- 1. the kernel
def _launch(x, dst, base):
    from madm_amd import optim
    fp = torch.zeros(1, dtype=torch.int64, device="cuda")
    optim.snapshot(x, dst, fp, base)
    return fp.item() & MASK


@pytest.mark.parametrize("n", [4, 1027, 1 << 20, (1 << 26) + 4])
def test_snapshot_kernel_matches_the_restatement(cuda, n):
    from madm_amd import optim
    host = np.random.default_rng(n % 1000).standard_normal(n).astype(np.float32)
    host[n // 3] = -0.0
    host.view(np.uint32)[n // 2] = 0x7fc01234                          # a NaN payload counts
    x = torch.from_numpy(host).cuda()
    for base in (0, 12345):
        want = fingerprint_numpy(host, base)
        dst = torch.full_like(x, 3.0)
        assert _launch(x, dst, base) == want, (n, base)
        assert torch.equal(dst.view(torch.int32), x.view(torch.int32))              # bit-exact copy
        assert _launch(x, None, base) == want                                       # fingerprint only
        dst2 = torch.full_like(x, 3.0)
        optim.snapshot(x, dst2, None, base)                                         # copy only
        assert torch.equal(dst2.view(torch.int32), x.view(torch.int32))
    want = fingerprint_numpy(host)
    assert optim.fingerprints([x]) == [want]
    # ten launches, one value
    assert {_launch(x, None, 0) for _ in range(10)} == {want}
    # a single flipped bit; a swap of two unequal elements
    y = x.clone()
    y.view(torch.int32)[n - 1] ^= 1
    assert _launch(y, None, 0) != want
    i, j = 1, n - 2
    assert host[i] != host[j]
    z = x.clone()
    z[i], z[j] = x[j], x[i]
    assert _launch(z, None, 0) != want
    # the halves, with their index_base, sum to the whole (the split keeps both pieces 16-byte aligned)
    h = (n // 2) // 4 * 4
    if h:
        assert (_launch(x[:h], None, 0) + _launch(x[h:], None, h)) & MASK == want
    torch.cuda.synchronize()


def test_snapshot_known_answer(cuda):
    from madm_amd import optim
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(1027).astype(np.float32)).cuda()
    assert optim.fingerprints([x]) == [KNOWN_ANSWER]


# ----------------------------------------------------------------------------- helpers of the trainer tests
def keep_filter(model):
    """Everything but the frozen pretrained tensors (UNet base weights, VAE): trainable tensors, the EMA teacher, buffers."""
    teacher = {id(p) for m in model.ema_parms for p in m.parameters()}
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad and id(p) not in teacher}
    return (lambda n, t: n not in frozen), frozen


def seed_all(s):
    random.seed(s)
    np.random.seed(s + 1)
    torch.manual_seed(s + 2)
    torch.cuda.manual_seed(s + 3)


def batch(i, B=None):
    data = train_inputs(**dict(TRAIN_CASE, input_seed=TRAIN_CASE["input_seed"] + i))
    return data if B is None else data[:B]


TRAINER_KW = dict(lr=1e-3, weight_decay=0.05, grad_clip=1.0, amp=True, init_scale=512.0, growth_interval=3)


def make(dtype=torch.float32, dist=None, **kw):
    from madm_amd.train import MadmTrainer
    model = build_product_train(dtype, "train_depth_lora_only")
    trainer = MadmTrainer(model, dist=dist, **dict(TRAINER_KW, **kw))
    return model, trainer


def checkpointer(model, trainer, save_dir, **kw):
    from madm_amd.checkpoint import MadmCheckpointer
    keep, frozen = keep_filter(model)
    return MadmCheckpointer(model, str(save_dir), keep=keep, trainer=trainer, **kw), frozen


def training_state(model, trainer):
    """Clones of everything a checkpoint has to bring back."""
    out = {"p." + n: p.detach().clone() for n, p in model.named_parameters()}
    out.update({"b." + n: b.detach().clone() for n, b in model.named_buffers()})
    out.update(m=trainer.opt.m.clone(), v=trainer.opt.v.clone(), steps=torch.from_numpy(np.asarray(trainer.opt.steps).copy()),
               scale=trainer.scale, tracker=trainer._growth_tracker, iter=trainer.iter, model_step=model.train_iter_index)
    rng = trainer.rng_state()
    out.update(rng_python=rng["python"], rng_numpy=rng["numpy"], rng_cpu=rng["torch_cpu"], rng_device=rng["torch_device"])
    out.update({"fp." + k: v for k, v in trainer.state_fingerprints().items()})
    return out


def assert_bitwise(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            x, y = a[k].contiguous(), b[k].contiguous()
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), k
        else:
            assert a[k] == b[k], k


def eval_logits(model, img):
    from madm_amd import ops
    model.eval()
    try:
        with ops.tuning_profile("throughput", pin=True):
            return model([{"target_second_modality": img}])[0]["sem_seg"].detach().clone()
    finally:
        model.train()


# ----------------------------------------------------------------------------- 2. round trip
def test_round_trip_is_bitwise(cuda, tmp_path):
    model, trainer = make()
    seed_all(7)
    for i in range(2):
        _, _, stepped = trainer.run_step(batch(i))
        assert stepped
    ck, frozen = checkpointer(model, trainer, tmp_path)
    ck.save("model_0000001", iteration=1)
    ck.wait()
    want = training_state(model, trainer)
    assert want["tracker"] == 2 and want["scale"] == 512.0 and want["iter"] == 2 and want["model_step"] == 2
    assert int(want["steps"].max()) == 2 and set(want) >= {"fp.param", "fp.exp_avg", "fp.exp_avg_sq", "fp.teacher"}
    assert len(frozen) > 600 and os.path.getsize(str(tmp_path / "model_0000001.pth")) < 500e6
    raw = torch.load(str(tmp_path / "model_0000001.pth"), weights_only=True)
    assert not set(raw["model"]) & frozen and raw["iteration"] == 1
    assert {k: int(v, 16) for k, v in raw["fingerprints"].items()} == trainer.state_fingerprints()

    model2, trainer2 = make()
    seed_all(1234)                                       # every generator somewhere else: the load has to bring them back
    ptrs = {n: p.data_ptr() for n, p in model2.named_parameters()}
    ck2, _ = checkpointer(model2, trainer2, tmp_path)
    res = ck2.resume_or_load("", resume=True)
    ignored = set(model2.ignored_state_dict()) if hasattr(model2, "ignored_state_dict") else set()
    assert res["iteration"] == 1 and set(res.missing_keys) == frozen - ignored and not res.unexpected_keys
    assert {n: p.data_ptr() for n, p in model2.named_parameters()} == ptrs          # loaded INTO the flat storage
    assert_bitwise(training_state(model2, trainer2), want)

    # an eval-mode forward under one tuning profile: a stale packed operand would be an O(1) error
    img = batch(9)[0]["target_second_modality"]
    a, b = eval_logits(model, img), eval_logits(model2, img)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    # the same gradient through both optimizers: parameters and moments stay bitwise equal
    g = torch.randn(trainer.opt.flat.grad.shape, generator=torch.Generator().manual_seed(5)).cuda() * 1e-2
    for tr in (trainer, trainer2):
        tr.opt.flat.grad.copy_(g)
        norm, stepped = tr.opt.step(clip_grad=None)
        assert stepped
    torch.cuda.synchronize()
    for x, y in ((trainer.opt.flat.flat, trainer2.opt.flat.flat), (trainer.opt.m, trainer2.opt.m), (trainer.opt.v, trainer2.opt.v)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert list(trainer.opt.steps) == list(trainer2.opt.steps) and int(trainer.opt.steps.max()) == 3
    assert not torch.equal(trainer.opt.m, want["m"])


# ----------------------------------------------------------------------------- 3. continuity of a resumed run
KEYS = ("ema_logits", "pseudo_label", "pseudo_weight", "mixed_lbl", "mixed_seg_weight", "source_logits", "target_logits")


def _record(model, losses, stepped):
    ls = model.last_step
    return dict(losses=dict(losses), stepped=stepped,
                **{k: (ls[k] if torch.is_tensor(ls[k]) else ls[k].t).detach().clone() for k in KEYS})


def _dist(ra, rb, k):
    if ra[k].dtype in (torch.int64, torch.uint8):
        return float((ra[k] != rb[k]).double().mean())
    return float((ra[k].double() - rb[k].double()).abs().max() / max(1e-6, float(rb[k].double().abs().max())))


@pytest.mark.parametrize("dtype,lr", [(torch.float32, 0.0), (torch.float16, 0.0), (torch.float32, 1e-4)],
                         ids=["f32-frozen", "f16-frozen", "f32-lr1e-4"])
def test_resumed_run_continues_the_interrupted_one(cuda, tmp_path, dtype, lr):
    """On the design of test_train_gpu.py::test_teacher_side_stream_is_bit_identical_over_steps.  Run A: five seeded steps.
    Run B: two steps, save, model and trainer deleted, both built afresh, resume_or_load, three steps.  No
    ``dropout_scale_override``: the Dropout2d masks come from the device generator, whose restored state is part of what is
    tested.  lr = 0: the forward of step k is a deterministic function of the restored state (EMA teacher, counters,
    generators, BatchNorm statistics), so steps 3 to 5 are BIT-identical.  lr = 1e-4: the backward's float atomics make two
    uninterrupted runs differ already; run A is run twice, both distances are printed per step, and the resumed run's first
    step after the load is held to that test's gate (1e-2 of a tensor's magnitude, 1 % of a discrete map)."""
    from madm_amd import ldm_rocm
    kw = dict(lr=lr, weight_decay=0.0 if lr == 0.0 else 0.01, grad_clip=None, amp=(dtype != torch.float32))
    batches = [batch(i) for i in range(5)]
    batches[3] = batches[3][:1]

    def fresh():
        ldm_rocm._const_cache.clear()
        ldm_rocm._noise_cache.clear()
        return make(dtype, **kw)

    def steps(model, trainer, todo):
        rec = []
        for data in todo:
            losses, _, stepped = trainer.run_step(data)
            rec.append(_record(model, losses, stepped))
        torch.cuda.synchronize()
        return rec

    runs = {}
    for tag in ["A"] + (["A2"] if lr > 0 else []):
        model, trainer = fresh()
        seed_all(97)
        runs[tag] = steps(model, trainer, batches)
        del model, trainer
        torch.cuda.empty_cache()
    model, trainer = fresh()
    seed_all(97)
    rec = steps(model, trainer, batches[:2])
    ck, _ = checkpointer(model, trainer, tmp_path)
    ck.save("model_0000001", iteration=1)
    ck.wait()
    del model, trainer, ck
    torch.cuda.empty_cache()
    model, trainer = fresh()
    seed_all(4321)
    ck, _ = checkpointer(model, trainer, tmp_path)
    assert ck.resume_or_load("", resume=True)["iteration"] == 1 and trainer.iter == 2 and model.train_iter_index == 2
    runs["B"] = rec + steps(model, trainer, batches[2:])

    for i in range(5):
        ra, rb = runs["A"][i], runs["B"][i]
        assert ra["stepped"] == rb["stepped"]
        if lr == 0.0:
            for k in KEYS:
                assert torch.equal(ra[k], rb[k]), f"step {i}: {k} differs between the uninterrupted and the resumed run"
            assert ra["losses"] == rb["losses"], (i, ra["losses"], rb["losses"])
        else:
            rc = runs["A2"][i]
            for k in KEYS:
                noise, d_ = _dist(ra, rc, k), _dist(ra, rb, k)
                print(f"   step {i} {k:18s} uninterrupted vs uninterrupted {noise:.2e}   uninterrupted vs resumed {d_:.2e}")
                if i <= 2:
                    assert d_ <= 1e-2, (i, k, d_, noise)
            if i <= 2:
                for n_, v in ra["losses"].items():
                    assert abs(v - rb["losses"][n_]) <= 1e-2 * max(abs(v), 1e-3), (i, n_, v, rb["losses"][n_], rc["losses"][n_])


# ----------------------------------------------------------------------------- 4. isolation of an asynchronous save
def _stir(trainer, seed):
    """Moments, step counts and BatchNorm statistics as after some training, without running a step."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for row in trainer.opt.state_dict(trainer.param_names)["state"].values():
            row["exp_avg"].copy_(torch.randn(row["exp_avg"].shape, generator=g))
            row["exp_avg_sq"].copy_(torch.rand(row["exp_avg_sq"].shape, generator=g))
        for b in trainer.model.buffers():
            if b.dtype.is_floating_point:
                b.add_(0.5)
    trainer.opt.steps = np.arange(len(trainer.opt.params), dtype=np.int64) % 5
    trainer.iter, trainer.model.train_iter_index = 11, 11


def test_async_save_is_isolated_from_what_follows(cuda, tmp_path):
    from madm_amd.checkpoint import PeriodicCheckpointer
    model, trainer = make()
    _stir(trainer, 1)
    ck, frozen = checkpointer(model, trainer, tmp_path, async_save=True)
    keep = ck.keep
    want_model = {k: v.detach().clone() for k, v in model.state_dict().items() if keep(k, v)}
    want_opt = {n: (row["exp_avg"].clone(), row["exp_avg_sq"].clone(), row["step"])
                for n, row in trainer.opt.state_dict(trainer.param_names)["state"].items()}
    torch.cuda.synchronize()
    ck.save("model_0000010", iteration=10)
    # the "next steps": every parameter, moment, teacher tensor and BatchNorm statistic is overwritten in place at once
    with torch.no_grad():
        trainer.opt.flat.flat.fill_(7.0)
        trainer.opt.m.fill_(-3.0)
        trainer.opt.v.fill_(9.0)
        model._ema_teacher_flat.flat.fill_(5.0)
        for b in model.buffers():
            b.fill_(2)
    trainer.opt.steps = trainer.opt.steps + 100
    trainer.iter = 999
    ck.wait()
    raw = torch.load(str(tmp_path / "model_0000010.pth"), weights_only=True)
    assert set(raw["model"]) == set(want_model) and raw["iteration"] == 10 and raw["trainer"]["iteration"] == 11
    for k, v in want_model.items():
        assert torch.equal(raw["model"][k], v.cpu()), k
    st = raw["trainer"]["optimizer"]["state"]
    assert set(st) == set(want_opt)
    for n, (m, v, step) in want_opt.items():
        assert torch.equal(st[n]["exp_avg"], m.cpu()) and torch.equal(st[n]["exp_avg_sq"], v.cpu()) and st[n]["step"] == step, n
    # two saves in a row: the second waits for the first, both files are complete
    ck.save("a")
    ck.save("b")
    ck.wait()
    for name in ("a", "b"):
        assert set(torch.load(str(tmp_path / f"{name}.pth"), weights_only=True)["model"]) == set(want_model)
    per = PeriodicCheckpointer(ck, period=1, max_to_keep=1)
    per.step(20)
    per.step(21)
    ck.wait()
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("model_00000")) == \
        ["model_0000010.pth", "model_0000021.pth"]
    assert open(str(tmp_path / "last_checkpoint")).read() == "model_0000021.pth"
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]


# ----------------------------------------------------------------------------- 5. load-time verification
def test_altered_file_fails_verification(cuda, tmp_path):
    model, trainer = make()
    _stir(trainer, 2)
    ck, _ = checkpointer(model, trainer, tmp_path, async_save=False)
    ck.save("m")
    raw = torch.load(str(tmp_path / "m.pth"), weights_only=True)
    name = trainer.param_names[len(trainer.param_names) // 2]
    raw["trainer"]["optimizer"]["state"][name]["exp_avg"].view(-1)[0] += 1.0
    torch.save(raw, str(tmp_path / "altered.pth"))
    with pytest.raises(RuntimeError, match="fingerprint of buffer 'exp_avg' "):
        ck.load(str(tmp_path / "altered.pth"))
    assert ck.load(str(tmp_path / "m.pth")) == {}


# ----------------------------------------------------------------------------- 6. through a process group
def test_save_and_resume_through_a_single_rank_group(cuda, tmp_path, monkeypatch):
    import torch.distributed as tdist
    from madm_amd import dist as mdist
    from madm_amd.checkpoint import PeriodicCheckpointer
    if tdist.is_initialized():
        pytest.skip("a default process group already exists in this process")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MADM_FORCE_PROCESS_GROUP", "1")
    d = mdist.init("nccl", torch.device("cuda", torch.cuda.current_device()))
    assert d is not None and d.get_world_size() == 1
    try:
        model, trainer = make(dist=d)
        assert trainer.reducer.active
        seed_all(3)
        _, _, stepped = trainer.run_step(batch(0))
        assert stepped and trainer.replicas_in_sync()
        ck, frozen = checkpointer(model, trainer, tmp_path)
        assert ck.save_to_disk
        per = PeriodicCheckpointer(ck, period=1, max_iter=1)
        per.step(0)
        ck.wait()
        assert sorted(os.listdir(str(tmp_path))) == ["last_checkpoint", "model_0000000.pth", "model_final.pth"]
        want = training_state(model, trainer)
        model2, trainer2 = make(dist=d)
        ck2, _ = checkpointer(model2, trainer2, tmp_path)
        assert ck2.resume_or_load("", resume=True)["iteration"] == 0
        assert_bitwise(training_state(model2, trainer2), want)
        assert trainer2.replicas_in_sync()
    finally:
        d.destroy_process_group()
