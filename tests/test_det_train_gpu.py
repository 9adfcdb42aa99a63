"""The deterministic training mode end to end (MadmTrainer(deterministic=True); madm_amd/ops.py: set_deterministic; DESIGN.md
section 24) on the 64 x 64 training case of the fixtures (golden_util.TRAIN_CASE):

1. two freshly built runs with a non-zero learning rate agree bit for bit -- losses, the flat gradient, parameters, both
   AdamW moments, the loss scale and the EMA teacher, after every step;
2. a resumed run lands where the uninterrupted one lands, with lr = 1e-4 (the construction of
   tests/test_checkpoint_gpu.py::test_resumed_run_continues_the_interrupted_one, which proves this with lr = 0 only);
3. the mode computes the same mathematics: the unchanged gates of tests/test_train_gpu.py::test_train_step_matches_fixture;
4. off means off: the library is not loaded by default steps, and the trainer restores the switch, also when a step raises;
5. test 1 with every uninitialised device buffer and workspace poisoned (MADM_DEBUG_POISON_HBM=1), in a child process.
"""
import os
import subprocess
import sys

import pytest
import torch

from golden_util import TRAIN_CASE, train_inputs
from test_train_gpu import build_product_train, test_train_step_matches_fixture as fixture_gates
import test_checkpoint_gpu as CK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.element_size() == 2 and t.is_floating_point() else t)


def _state(model, trainer, losses):
    """Clones of everything the step produced or changed"""
    out = {"grad": trainer.opt.flat.grad.clone(), "param": trainer.opt.flat.flat.clone(), "m": trainer.opt.m.clone(),
           "v": trainer.opt.v.clone(), "scale": trainer.scale, "losses": dict(losses)}
    tf = getattr(model, "_ema_teacher_flat", None)
    if tf is not None:
        out["teacher"] = tf.flat.clone()
    else:
        out.update({"teacher." + str(i): p.detach().clone() for i, m in enumerate(model.ema_parms) for p in m.parameters()})
    return out


def _assert_same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in {int((_bits(a[k]) != _bits(b[k])).sum())} elements"
        else:
            assert a[k] == b[k], f"{what}: {k}: {a[k]} != {b[k]}"


def _three_steps(dtype):
    """Two fresh (model, trainer) pairs, the same seeds, three steps each; returns the per-step states of both"""
    from madm_amd import ldm_rocm, ops
    from madm_amd.train import MadmTrainer
    batches = [CK.batch(i) for i in range(3)]
    runs = []
    for _ in range(2):
        ldm_rocm._const_cache.clear()
        ldm_rocm._noise_cache.clear()
        model = build_product_train(dtype, "train_depth")
        # f16: the loss scale of the fixture test (4096), so that the first steps are not skipped for overflow
        trainer = MadmTrainer(model, lr=1e-4, weight_decay=0.01, grad_clip=None, amp=(dtype != torch.float32), init_scale=4096.0,
                              deterministic=True)
        CK.seed_all(31)
        rec = []
        for data in batches:
            losses, norm, stepped = trainer.run_step(data)
            assert not ops.is_deterministic()
            rec.append(_state(model, trainer, losses))
            # the returned gradient norm is an f64 sum of f32 block partials (sumsq_f32: left as it is): the two
            # runs may differ in its last f64 digit (observed: 36.66526416263952 / ...948), so it is compared as an f32
            rec[-1].update(norm_f32=None if norm is None else float(torch.tensor(float(norm), dtype=torch.float32)), stepped=bool(stepped))
        torch.cuda.synchronize()
        runs.append(rec)
        del model, trainer
        torch.cuda.empty_cache()
    return runs


def _check_three_steps(dtype):
    a, b = _three_steps(dtype)
    for i in range(3):
        _assert_same(a[i], b[i], f"step {i + 1}")
    assert "teacher" in a[0] or any(k.startswith("teacher.") for k in a[0])
    assert any(r["stepped"] for r in a) and float(a[0]["grad"].abs().max()) > 0
    assert not torch.equal(a[0]["param"], a[2]["param"])                                          # it learned


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_two_runs_agree_with_learning(cuda, dtype):
    _check_three_steps(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_resumed_run_lands_where_the_uninterrupted_run_lands(cuda, tmp_path, dtype):
    from madm_amd import ldm_rocm
    kw = dict(lr=1e-4, weight_decay=0.01, grad_clip=None, amp=(dtype != torch.float32), deterministic=True)
    batches = [CK.batch(i) for i in range(5)]
    batches[3] = batches[3][:1]

    def fresh():
        ldm_rocm._const_cache.clear()
        ldm_rocm._noise_cache.clear()
        return CK.make(dtype, **kw)

    def steps(model, trainer, todo):
        rec = []
        for data in todo:
            losses, _, stepped = trainer.run_step(data)
            rec.append(CK._record(model, losses, stepped))
        torch.cuda.synchronize()
        return rec

    model, trainer = fresh()
    assert trainer.deterministic
    CK.seed_all(97)
    run_a = steps(model, trainer, batches)
    end_a = {k: v.clone() for k, v in (("param", trainer.opt.flat.flat), ("m", trainer.opt.m), ("v", trainer.opt.v))}
    del model, trainer
    torch.cuda.empty_cache()
    model, trainer = fresh()
    CK.seed_all(97)
    rec = steps(model, trainer, batches[:2])
    ck, _ = CK.checkpointer(model, trainer, tmp_path)
    ck.save("model_0000001", iteration=1)
    ck.wait()
    del model, trainer, ck
    torch.cuda.empty_cache()
    model, trainer = fresh()
    CK.seed_all(4321)
    ck, _ = CK.checkpointer(model, trainer, tmp_path)
    assert ck.resume_or_load("", resume=True)["iteration"] == 1 and trainer.iter == 2 and model.train_iter_index == 2
    run_b = rec + steps(model, trainer, batches[2:])
    for i in range(5):
        ra, rb = run_a[i], run_b[i]
        assert ra["stepped"] == rb["stepped"]
        for k in CK.KEYS:
            assert torch.equal(ra[k], rb[k]), f"step {i + 1}: {k} differs between the uninterrupted and the resumed run"
        assert ra["losses"] == rb["losses"], (i + 1, ra["losses"], rb["losses"])
    for k, v in (("param", trainer.opt.flat.flat), ("m", trainer.opt.m), ("v", trainer.opt.v)):
        assert torch.equal(_bits(v), _bits(end_a[k])), f"final {k} differs"
    assert not torch.equal(run_a[0]["source_logits"], run_a[4]["source_logits"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["depth-f32", "depth-f16"])
def test_same_mathematics(cuda, dtype):
    from madm_amd import ops
    with ops.deterministic():
        fixture_gates(cuda, "train_depth", dtype)
    assert not ops.is_deterministic()


_OFF = """
import random, sys
import numpy as np, torch
sys.path.insert(0, {tests!r})
from golden_util import TRAIN_CASE, train_inputs
from test_train_gpu import build_product_train
from madm_amd.train import MadmTrainer
from madm_amd import ops
model = build_product_train(torch.float32, "train_depth_lora_only")
trainer = MadmTrainer(model, lr=1e-3, weight_decay=0.05, grad_clip=None, amp=False)
random.seed(1); np.random.seed(2)
for i in range(2):
    trainer.run_step(train_inputs(**TRAIN_CASE))
torch.cuda.synchronize()
assert "madm_amd._lib_det" not in sys.modules and not ops.is_deterministic()
assert "libmadm_det" not in open("/proc/self/maps").read()
print("default steps left the library alone")
"""


def test_off_means_off(cuda):
    import random
    import numpy as np
    from madm_amd import ops
    from madm_amd.train import MadmTrainer
    r = subprocess.run([sys.executable, "-c", _OFF.format(tests=os.path.join(ROOT, "tests"))], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "left the library alone" in r.stdout, r.stderr[-3000:]
    # the trainer restores the switch: after a step, and after a step that raises (the input-range assert)
    model = build_product_train(torch.float32, "train_depth_lora_only")
    trainer = MadmTrainer(model, lr=1e-3, weight_decay=0.05, grad_clip=None, amp=False, deterministic=True)
    random.seed(1)
    np.random.seed(2)
    assert not ops.is_deterministic()
    trainer.run_step(train_inputs(**TRAIN_CASE))
    assert not ops.is_deterministic()
    bad = train_inputs(**TRAIN_CASE)
    bad[1]["source_rgb"] = bad[1]["source_rgb"] * 1.5
    with pytest.raises(AssertionError, match="input range check"):
        trainer.run_step(bad)
    assert not ops.is_deterministic()
    prev = ops.set_deterministic(True)          # and it restores whatever was set before, not "off"
    try:
        trainer.run_step(train_inputs(**TRAIN_CASE))
        assert ops.is_deterministic()
    finally:
        ops.set_deterministic(prev)
    assert not ops.is_deterministic()


_POISONED = """
import sys
sys.path.insert(0, {tests!r})
import torch
from madm_amd import _debug
assert _debug.MODE == 1
import test_det_train_gpu as T
T._check_three_steps(torch.float32)
assert _debug.COUNT["workspace"] > 0 and _debug.COUNT["tensors"] > 0
print("poisoned runs agree", _debug.COUNT)
"""


def test_two_runs_agree_with_poisoned_buffers(cuda):
    """Every torch.empty and every workspace hand-out NaN-filled: a partial or a workspace row read before it is written
    would put NaNs into the gradient (and the two runs would still have to agree)."""
    env = dict(os.environ, MADM_DEBUG_POISON_HBM="1")
    r = subprocess.run([sys.executable, "-c", _POISONED.format(tests=os.path.join(ROOT, "tests"))], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "poisoned runs agree" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
