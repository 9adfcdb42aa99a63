"""CPU tests of the evaluator's exports (madm_amd/eval_export.py, evaluation.DSECSemSegEvaluator): the PNG container
around ready scanlines, the plane layout against files PIL wrote from the reference's own four statements
(tests/golden/eval_export_pil.npz; d2_evaluator.py:169-183), file names and directories of both modes, the writer ring
(atomic files, error propagation, back-pressure) and ``evaluate()``."""
import ctypes
import io
import os
import threading

import numpy as np
import pytest
import torch

from eval_export_util import DELIVER_PALETTE, DIRS, decode_png, fixture, pack_ref, planes_ref, read_png

K = 11
NAMES = [f"c{i}" for i in range(K)]


def _evaluator(tmp_path=None, **kw):
    from madm_amd.evaluation import DSECSemSegEvaluator
    args = dict(dataset_name="DS", stuff_classes=NAMES, palette=DELIVER_PALETTE, ignore_label=255,
                output_dir=None if tmp_path is None else str(tmp_path), save_predictions_json=False)
    args.update(kw)
    return DSECSemSegEvaluator(**args)


def _case(seed, H=6, W=5):
    rng = np.random.default_rng(seed)
    image = (rng.random((3, H, W)) * 255).astype(np.float32)
    pred = rng.integers(0, K, (H, W)).astype(np.int64)
    gt = rng.integers(0, K, (H, W)).astype(np.int64)
    gt[0] = 255
    return image, pred, gt


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (48, 250), (64, 3)])
def test_encode_png_rows_round_trips(shape):
    from madm_amd import eval_export
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    gray = rng.integers(0, 65536, size=(H, W)).astype(np.uint16)
    gray.reshape(-1)[0] = 0x0102                       # the byte order shows
    rows_rgb = np.concatenate([np.zeros((H, 1), np.uint8), rgb.reshape(H, 3 * W)], axis=1)
    rows_gray = np.concatenate([np.zeros((H, 1), np.uint8), gray.astype(">u2").view(np.uint8).reshape(H, 2 * W)], axis=1)
    d_rgb = eval_export.encode_png_rows(rows_rgb.tobytes(), W, H, 8, 2)
    d_gray = eval_export.encode_png_rows(memoryview(rows_gray.reshape(-1)), W, H, 16, 0)
    a, ihdr = decode_png(d_rgb)
    assert ihdr == (8, 2) and np.array_equal(a, rgb)
    a, ihdr = decode_png(d_gray)
    assert ihdr == (16, 0) and np.array_equal(a, gray)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        im = Image.open(io.BytesIO(d_rgb))
        assert im.mode == "RGB" and im.size == (W, H) and np.array_equal(np.asarray(im), rgb)
        im = Image.open(io.BytesIO(d_gray))
        assert im.mode == "I;16" and im.size == (W, H) and np.array_equal(np.asarray(im), gray)
    for bad in (lambda: eval_export.encode_png_rows(rows_rgb.tobytes()[:-1], W, H, 8, 2),
                lambda: eval_export.encode_png_rows(rows_rgb.tobytes(), W, H, 16, 0),
                lambda: eval_export.encode_png_rows(rows_rgb.tobytes(), W, H, 4, 2),
                lambda: eval_export.encode_png_rows(rows_rgb.tobytes(), W, H, 8, 3)):
        with pytest.raises(ValueError):
            bad()


def test_product_path_needs_no_imaging_library():
    import madm_amd.eval_export as m
    src = open(m.__file__).read()
    for name in ("PIL", "matplotlib", "cv2", "imageio"):
        assert f"import {name}" not in src and f"from {name}" not in src
    assert "cpu_count" not in src


def test_plane_layout_reproduces_the_pil_fixture(tmp_path):
    """The numpy restatement of the pack buffer, written by ``submit_packed``, gives files whose pixels and IHDR fields are
    those of the files PIL wrote from the reference's statements."""
    from madm_amd import eval_export
    fx = fixture()
    image, pred, gt = fx["image_in"], fx["pred_in"], fx["gt_in"]
    assert image[0, 0, 0] == np.float32(0.4)              # the fixture holds the truncation probes and ignored pixels
    assert image[1, 0, 1] == np.float32(254.999) and image[2, 0, 2] == 255.0 and (gt == 255).any() and pred.max() == K - 1
    H, W = pred.shape
    packed = pack_ref(image, pred, gt, fx["palette"].tolist(), int(fx["num_classes"]), int(fx["ignore_label"]))
    assert packed.size == eval_export.pack_bytes(H, W) == sum(n for _o, n in eval_export.plane_slices(H, W))
    ex = eval_export.EvalExporter(tmp_path, rank=0, workers=2)
    ex.submit_packed(ex.plane_paths(7), torch.from_numpy(packed), H, W)
    ex.close()
    assert [os.path.relpath(p, tmp_path) for p in ex.plane_paths(7)] == [os.path.join(d, "000007_rank0.png") for d in DIRS]
    for d, path in zip(DIRS, ex.plane_paths(7)):
        a, ihdr = read_png(path)
        assert ihdr == tuple(fx[d + "_ihdr"].tolist()), d
        assert a.dtype == fx[d].dtype and np.array_equal(a, fx[d]), d
    # the truncation probes, and the ignored pixels black
    img = read_png(ex.plane_paths(7)[0])[0]
    assert (img[0, 0, 0], img[0, 1, 1], img[0, 2, 2]) == (0, 254, 255)
    assert not read_png(ex.plane_paths(7)[3])[0][gt == 255].any()
    assert ex.stats["images"] == 1 and ex.stats["files"] == 4 and ex.stats["encode_ms"] > 0


class _Recorder:
    """Stands in for the two launching calls of the exporter (they need a GPU): records what would be written."""

    def __init__(self, ex):
        self.ex, self.calls = ex, []
        ex.submit = lambda paths, *a: self.calls.append(("packed", list(paths)))
        ex.submit_sheet = lambda path, *a: self.calls.append(("sheet", path))


def _run(ev, records):
    for rec in records:
        image, pred, gt = _case(1)
        ev._after_image(dict(rec, target_second_modality=torch.from_numpy(image)), torch.from_numpy(pred),
                        torch.from_numpy(gt))


def test_file_names_and_directories(tmp_path, monkeypatch):
    monkeypatch.setenv("LOCAL_RANK", "3")
    # sheets: every 2nd image; pred_save_name where the record has one
    ev = _evaluator(tmp_path / "a", save_eval_results_step=2)
    ev.reset()
    assert (tmp_path / "a").is_dir()                      # reset() creates the output directory (d2_evaluator.py:87)
    rec = _Recorder(ev._exporter())
    _run(ev, [dict(pred_save_name="x/first.png"), dict(pred_save_name="second.png"), dict(), dict(), dict(pred_save_name="e.png")])
    out = str(tmp_path / "a")
    assert rec.calls == [("sheet", os.path.join(out, "x/first.png")), ("sheet", os.path.join(out, "000002_rank3.png")),
                         ("sheet", os.path.join(out, "e.png"))]
    assert ev.eval_index == 5
    ev.reset()                                            # eval_index lives on (d2_evaluator.py:40,133)
    assert ev.eval_index == 5
    _run(ev, [dict(), dict()])
    assert rec.calls[3:] == [("sheet", os.path.join(out, "000006_rank3.png"))] and ev.eval_index == 7
    # eval_only: four directories, the index name even where the record has a pred_save_name
    ev = _evaluator(tmp_path / "b", save_eval_results_step=3, eval_only=True)
    ev.reset()
    rec = _Recorder(ev._exporter())
    _run(ev, [dict(pred_save_name="n.png")] + [dict()] * 6)
    out = str(tmp_path / "b")
    assert rec.calls == [("packed", [os.path.join(out, d, f"{i:06d}_rank3.png") for d in DIRS]) for i in (0, 3, 6)]
    assert ev._exporter().rank == 3
    monkeypatch.delenv("LOCAL_RANK")
    assert _evaluator(tmp_path / "c", save_eval_results_step=1)._exporter().rank == 0


def _packed(seed, H=6, W=5):
    image, pred, gt = _case(seed, H, W)
    return pack_ref(image, pred, gt, DELIVER_PALETTE, K, 255), planes_ref(image, pred, gt, DELIVER_PALETTE, K, 255)


def test_writer_never_shows_a_partial_file(tmp_path):
    from madm_amd import eval_export
    ex = eval_export.EvalExporter(tmp_path, workers=2, depth=3)
    seen, lock = [], threading.Lock()
    real_replace = os.replace

    def spy_replace(src, dst):
        # nothing under the final name yet, and the temporary file is a complete PNG before it takes the name
        assert not os.path.exists(dst)
        with open(src, "rb") as f:
            decode_png(f.read())
        with lock:
            seen.append(os.path.relpath(dst, tmp_path))
        real_replace(src, dst)

    want = {}
    os.replace = spy_replace
    try:
        for i in range(5):
            packed, planes = _packed(i)
            want[i] = planes
            ex.submit_packed(ex.plane_paths(i), packed, 6, 5)
        ex.wait()
    finally:
        os.replace = real_replace
    assert sorted(seen) == sorted(os.path.join(d, f"{i:06d}_rank0.png") for d in DIRS for i in range(5))
    for d in DIRS:
        assert sorted(os.listdir(tmp_path / d)) == [f"{i:06d}_rank0.png" for i in range(5)]     # no temporary file is left
    for i in range(5):
        for path, a in zip(ex.plane_paths(i), want[i]):
            assert np.array_equal(read_png(path)[0], a), path
    ex.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("madm-eval-export")]
    with pytest.raises(RuntimeError):
        ex.submit_packed(ex.plane_paths(9), _packed(9)[0], 6, 5)


@pytest.mark.parametrize("nxt", ["submit_packed", "wait", "close"])
def test_worker_error_surfaces_from_the_next_call(tmp_path, nxt):
    """An output directory that cannot be made (its parent is a regular file): the submitting thread is not the one that
    fails, the next call reports it, once."""
    from madm_amd import eval_export
    (tmp_path / "plain").write_bytes(b"x")
    ex = eval_export.EvalExporter(tmp_path / "plain" / "out", workers=1)
    packed, _ = _packed(1)
    ex.submit_packed(ex.plane_paths(0), packed, 6, 5)
    with pytest.raises(OSError):
        {"submit_packed": lambda: (ex._slots[0].job.done.wait(), ex.submit_packed(ex.plane_paths(1), packed, 6, 5)),
         "wait": ex.wait, "close": ex.close}[nxt]()
    ex.wait()                                             # reported once
    if nxt != "close":
        ex.output_dir = str(tmp_path / "good")            # and the exporter is usable again
        ex.submit_packed(ex.plane_paths(2), packed, 6, 5)
        ex.wait()
        assert all(os.path.exists(p) for p in ex.plane_paths(2))
    ex.close()


def test_full_ring_blocks_counts_a_stall_and_loses_no_file(tmp_path):
    from madm_amd import eval_export
    ex = eval_export.EvalExporter(tmp_path, workers=1, depth=2)
    gate = threading.Event()
    real_write, real_wait = ex._write_file, ex._wait_for
    ex._write_file = lambda final, data: (gate.wait(), real_write(final, data))       # the workers are held here
    waited = []

    def stalled(job):                # submit found the ring full: only now are the workers let go
        waited.append(job)
        if len(waited) == 1:                                         # nothing is written or finished while the gate is shut
            assert not job.done.is_set() and not os.path.exists(tmp_path / "image")
        gate.set()
        real_wait(job)

    ex._wait_for = stalled
    want = {}
    for i in range(5):
        packed, want[i] = _packed(10 + i)
        ex.submit_packed(ex.plane_paths(i), packed, 6, 5)
        if i < 2:
            assert not waited and ex.stats["stalls"] == 0          # two slots: two jobs are taken without waiting
    assert len(waited) >= 1 and waited[0] is not None
    ex.wait()
    assert ex.stats["stalls"] == len(waited) >= 1 and ex.stats["stall_ms"] >= 0 and ex.stats["images"] == 5
    for i in range(5):
        for path, a in zip(ex.plane_paths(i), want[i]):
            assert np.array_equal(read_png(path)[0], a), path
    ex.close()


def test_exporter_waits_at_interpreter_exit(tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch; sys.path.insert(0, %r); from madm_amd import eval_export as e\n"
            "x = e.EvalExporter(%r, workers=2)\n"
            "H = W = 64\n"
            "for i in range(4): x.submit_packed(x.plane_paths(i), torch.zeros(e.pack_bytes(H, W), dtype=torch.uint8), H, W)\n"
            % (root, str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
    for d in DIRS:
        assert sorted(os.listdir(tmp_path / d)) == [f"{i:06d}_rank0.png" for i in range(4)]
    assert read_png(tmp_path / "pred" / "000003_rank0.png")[0].shape == (64, 64)


def test_evaluate_writes_the_metrics_file_and_keeps_the_numbers(tmp_path):
    from madm_amd.evaluation import SemSegEvaluator
    rng = np.random.default_rng(3)
    conf = torch.from_numpy(rng.integers(0, 1000, (K + 1, K + 1)).astype(np.int64))
    conf[K, :] = 0                                         # a prediction is never the ignore class
    conf[:, 4] = 0
    conf[4, :] = 0                                         # a class that never occurs: NaN IoU, as in the reference
    plain = SemSegEvaluator(K, class_names=NAMES, ignore_label=255)
    plain._conf = conf.clone()
    want = plain.evaluate()["sem_seg"]
    ev = _evaluator(tmp_path, prefix="val", save_eval_results_step=-1)
    ev.reset()
    ev._conf = conf.clone()
    got = ev.evaluate()
    assert list(got) == ["default"] and list(got["default"]) == ["sem_seg_default"]
    flat = got["default"]["sem_seg_default"]
    assert list(flat) == [f"DS/val_{k}" for k in want]
    for k, v in want.items():
        assert flat[f"DS/val_{k}"] == v or (np.isnan(v) and np.isnan(flat[f"DS/val_{k}"])), k
    assert np.isnan(want["IoU-c4"]) and not np.isnan(want["mIoU"])
    saved = torch.load(tmp_path / "sem_seg_default_evaluation.pth", weights_only=False)
    assert list(saved) == list(want)
    assert all(saved[k] == v or (np.isnan(v) and np.isnan(saved[k])) for k, v in want.items())
    assert sorted(os.listdir(tmp_path)) == ["sem_seg_default_evaluation.pth"]
    # no output directory: the same numbers, no prefix separator without a prefix, nothing written
    ev = _evaluator(None)
    ev.reset()
    ev._conf = conf.clone()
    assert ev.evaluate()["default"]["sem_seg_default"]["DS/mIoU"] == want["mIoU"]


def test_constructor_refusals(tmp_path):
    with pytest.raises(AssertionError):
        _evaluator(tmp_path, palette=DELIVER_PALETTE[:-3])
    with pytest.raises(NotImplementedError, match="save_predictions_json"):
        _evaluator(tmp_path, save_predictions_json=True)
    _evaluator(None, save_predictions_json=True)          # inert without an output directory, as in the reference
    with pytest.raises(NotImplementedError, match="target_modality"):
        _evaluator(tmp_path, target_modality=["default", "Depth"])
    with pytest.raises(NotImplementedError, match="target_modality"):
        _evaluator(tmp_path, target_modality=["Depth"])
    _evaluator(tmp_path, target_modality=["default"], enable_wandb=False)
    with pytest.raises(NotImplementedError, match="convert_pred_list"):
        _evaluator(tmp_path, convert_pred_list=[[1, 2]])
    with pytest.raises(ValueError):
        _evaluator(tmp_path, save_eval_results_step=0)
    with pytest.raises(TypeError):                        # keyword-only, as the reference's constructor
        from madm_amd.evaluation import DSECSemSegEvaluator
        DSECSemSegEvaluator("DS", NAMES, DELIVER_PALETTE, 255)


def test_exports_off_start_nothing(tmp_path):
    before = threading.active_count()
    for ev in (_evaluator(None, save_eval_results_step=1, eval_only=True), _evaluator(None, save_eval_results_step=2),
               _evaluator(tmp_path / "off", save_eval_results_step=-1, eval_only=True)):
        ev.reset()
        _run(ev, [dict(), dict(), dict()])
        assert ev.exporter is None and ev.eval_index == 3
        ev.wait()
        ev.close()
    assert threading.active_count() == before
    assert os.listdir(tmp_path / "off") == []
    # an exporter that has had no job holds no thread and no buffer either
    ev = _evaluator(tmp_path / "on", save_eval_results_step=1)
    ex = ev._exporter()
    assert (ex.workers, ex.depth) == (6, 12) and not ex._threads and all(s.dev is None and s.host is None for s in ex._slots)
    assert _evaluator(tmp_path / "on", save_eval_results_step=1, export_workers=2, export_depth=2)._exporter().depth == 2
    assert threading.active_count() == before


def test_pack_argument_checks_without_gpu():
    from madm_amd import _lib
    lib = _lib.lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    f = lib.madm_eval_export_pack
    assert f(None, p, p, 0, p, K, 255, 4, 4, p, None) == -1 and b"null" in lib.madm_last_error()
    assert f(p, p, p, 0, p, K, 255, 4, 4, None, None) == -1 and b"null" in lib.madm_last_error()
    assert f(p, p, p, 0, p, K, 255, 0, 4, p, None) == -1 and b"geometry" in lib.madm_last_error()
    assert f(p, p, p, 2, p, K, 255, 4, 4, p, None) == -1 and b"image kind" in lib.madm_last_error()
    assert f(p, p, p, 0, p, 0, 255, 4, 4, p, None) == -1 and b"classes" in lib.madm_last_error()
    assert f(p, p, p, 0, p, 256, 255, 4, 4, p, None) == -1 and b"classes" in lib.madm_last_error()
    assert f(p, p, p, 0, p, K, 255, 20000, 20000, p, None) == -1 and b"32-bit" in lib.madm_last_error()
    assert lib.madm_abi_version() == 6
