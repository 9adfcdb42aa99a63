"""The deterministic training mode with the ordered-slab weight gradient end to end (MadmTrainer(deterministic="slabs");
DESIGN.md section 28) on the 64 x 64 training case of the fixtures, as tests/test_det_train_gpu.py does for the one-slice mode --
the same model builder, batches and seeds:

1. two freshly built f16 runs of three steps at lr = 1e-4 agree bit for bit -- losses, the flat gradient, parameters, both
   AdamW moments, the loss scale and the EMA teacher, after every step -- and the run learned;
2. the mode computes the same mathematics: the unchanged gates of tests/test_train_gpu.py::test_train_step_matches_fixture, f32.

The kernel-level tests (tests/test_wslab_gpu.py) carry the coverage; these two show that the trainer passes the value through
and that nothing between the kernels depends on the path."""
import pytest
import torch

from test_train_gpu import build_product_train, test_train_step_matches_fixture as fixture_gates
import test_checkpoint_gpu as CK
import test_det_train_gpu as DT

pytestmark = pytest.mark.gpu


def _three_steps(dtype, launches):
    """test_det_train_gpu._three_steps with deterministic="slabs": two fresh (model, trainer) pairs, the same seeds"""
    from madm_amd import ldm_rocm, ops
    from madm_amd.train import MadmTrainer
    batches = [CK.batch(i) for i in range(3)]
    runs = []
    for _ in range(2):
        ldm_rocm._const_cache.clear()
        ldm_rocm._noise_cache.clear()
        model = build_product_train(dtype, "train_depth")
        trainer = MadmTrainer(model, lr=1e-4, weight_decay=0.01, grad_clip=None, amp=(dtype != torch.float32), init_scale=4096.0,
                              deterministic="slabs")
        assert trainer.deterministic == "slabs"
        CK.seed_all(31)
        rec = []
        for data in batches:
            before = len(launches)
            losses, norm, stepped = trainer.run_step(data)
            assert not ops.is_deterministic() and ops.wgrad_path() == "atomic"
            assert len(launches) > before, "the step launched no slab weight gradient"
            rec.append(DT._state(model, trainer, losses))
            rec[-1].update(norm_f32=None if norm is None else float(torch.tensor(float(norm), dtype=torch.float32)), stepped=bool(stepped))
        torch.cuda.synchronize()
        runs.append(rec)
        del model, trainer
        torch.cuda.empty_cache()
    return runs


def test_two_runs_agree_with_learning(cuda, monkeypatch):
    from madm_amd import _lib_wslab as Lw
    from madm_amd import ops
    launches, real = [], Lw.lib.mws_conv2d_wgrad
    monkeypatch.setattr(Lw.lib, "mws_conv2d_wgrad", lambda *a: (launches.append(1), real(*a))[1])
    monkeypatch.setattr(ops.lib, "madm_conv2d_wgrad", _raise, raising=False)
    a, b = _three_steps(torch.float16, launches)
    for i in range(3):
        DT._assert_same(a[i], b[i], f"step {i + 1}")
    assert any(r["stepped"] for r in a) and float(a[0]["grad"].abs().max()) > 0
    assert not torch.equal(a[0]["param"], a[2]["param"])                                          # it learned


def _raise(*a):
    raise AssertionError("madm_conv2d_wgrad was launched under deterministic='slabs'")


def test_same_mathematics(cuda):
    from madm_amd import ops
    with ops.deterministic("slabs"):
        fixture_gates(cuda, "train_depth", torch.float32)
    assert not ops.is_deterministic() and ops.wgrad_path() == "atomic"
