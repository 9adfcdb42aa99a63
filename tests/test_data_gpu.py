"""The dataset pipeline on the device (libmadm_data.so, madm_amd/data.py): both kernels bit for bit against the numpy
restatement of PIL's resizes (tests/data_util.py; tests/test_data_host.py holds that restatement to PIL itself), with every
output inside guard bands; the dataset against the fixture of the reference's outputs; the hand-over between streams; the
loaders; ``inference_on_dataset`` fed by the test loader."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import data_util as du
from window_util import PATTERN

pytestmark = pytest.mark.gpu

GUARD = 8       # guard rows above and below every plane; the same number of guard columns on both sides


class GuardedPlanes:
    """[planes, ch, cw] window inside a [planes, GUARD + ch + GUARD, GUARD + cw + GUARD + 3] buffer of the canary pattern
    (window_util.PATTERN: a NaN for f32): ``check`` proves that nothing outside the window was written."""

    def __init__(self, planes, ch, cw, dtype):
        self.itype, self.pattern = PATTERN[dtype]
        self.ld = GUARD + cw + GUARD + 3                        # an odd stride: rows start at every alignment the type allows
        self.rows = GUARD + ch + GUARD
        self.ibuf = torch.full((planes, self.rows, self.ld), self.pattern, dtype=self.itype, device="cuda")
        self.buf = self.ibuf.view(dtype)
        self.view = self.buf[:, GUARD:GUARD + ch, GUARD:GUARD + cw]
        self.outside = torch.ones_like(self.ibuf, dtype=torch.bool)
        self.outside[:, GUARD:GUARD + ch, GUARD:GUARD + cw] = False

    def check(self, what):
        hit = (self.ibuf != self.pattern) & self.outside
        assert not bool(hit.any()), f"{what}: write outside the window at (plane, row, column) {hit.nonzero()[0].tolist()}"
        assert not bool((self.ibuf == self.pattern)[~self.outside].any()), f"{what}: an element of the window was not written"


@functools.lru_cache(maxsize=None)
def _case(i, C, ids=False):
    """(source array incl. rows outside the window, window rows, bilinear-resized, nearest-resized): computed once."""
    (ih, iw), (oh, ow), window = du.RESIZE_CASES[i]
    a = np.random.RandomState(100 + 10 * i + C).randint(0, 256, size=(ih, iw) if C == 1 else (ih, iw, C)).astype(np.uint8)
    if ids:
        a = (a % 12).astype(np.uint8)               # class ids for the label path
        a[::7, ::5] = 255
        a[1::9, 2::4] = 0
    win = a if window is None else a[:window]
    return a, win.shape[0], du.resize_bilinear(win, oh, ow), du.resize_nearest(win if C == 1 else win[:, :, 0], oh, ow)


def _crops(rh, rw):
    ch, cw = min(rh, 19 if rh < 40 else 35), min(rw, 37 if rw < 100 else 70)       # no multiple of the 16 x 64 / 4 x 64 tiles
    return [(0, 0, ch, cw), (rh - ch, rw - cw, ch, cw), (0, 0, rh, rw)]


_TABLES = {}


def _dev_table(kind, i, o):
    from madm_amd import data
    key = (kind, i, o)
    if key not in _TABLES:
        if i == o:
            _TABLES[key] = None
        elif kind == "bilinear":
            _TABLES[key] = tuple(torch.from_numpy(t).cuda() for t in data.bilinear_table(i, o))
        else:
            _TABLES[key] = torch.from_numpy(data.nearest_table(i, o)).cuda()
    return _TABLES[key]


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _prep_image(src, C, in_h, in_w, rh, rw, y0, x0, ch, cw, flip, out_view, ld, plane):
    from madm_amd import _lib_data
    hb, vb = _dev_table("bilinear", in_w, rw), _dev_table("bilinear", in_h, rh)
    return _lib_data.lib.mdata_prep_image_u8(
        src.data_ptr(), C, src.shape[1] * C, in_h, in_w,
        _ptr(hb[0]) if hb else None, _ptr(hb[1]) if hb else None, hb[1].shape[1] if hb else 0,
        _ptr(vb[0]) if vb else None, _ptr(vb[1]) if vb else None, vb[1].shape[1] if vb else 0,
        rh, rw, y0, x0, ch, cw, flip, out_view.data_ptr(), ld, plane, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("i", range(len(du.RESIZE_CASES)), ids=lambda i: "{0[0]}x{0[1]}-{1[0]}x{1[1]}".format(*du.RESIZE_CASES[i]))
def test_prep_image_matches_the_restatement(cuda, i, C):
    a, in_h, resized, _ = _case(i, C)
    (_ih, in_w), (rh, rw), _w = du.RESIZE_CASES[i]
    src = torch.from_numpy(a).cuda()
    bad = 0
    for y0, x0, ch, cw in _crops(rh, rw):
        for flip in (0, 1):
            g = GuardedPlanes(3, ch, cw, torch.float32)
            rc = _prep_image(src, C, in_h, in_w, rh, rw, y0, x0, ch, cw, flip, g.view, g.ld, g.rows * g.ld)
            assert rc == 0
            want = du.prep_image_ref(resized, None, (y0, x0, ch, cw, flip))
            got = g.view.cpu().numpy()
            g.check(f"prep_image crop {ch} x {cw} at ({y0}, {x0}) flip {flip}")
            n = int((got != want).sum())
            print(f"C={C} crop {ch}x{cw}@({y0},{x0}) flip={flip}: {n} mismatching values")
            bad += n
    assert bad == 0


@pytest.mark.parametrize("luts", ["none", "lut1", "lut1+lut2"])
@pytest.mark.parametrize("i", range(len(du.RESIZE_CASES)), ids=lambda i: "{0[0]}x{0[1]}-{1[0]}x{1[1]}".format(*du.RESIZE_CASES[i]))
def test_prep_label_matches_the_restatement(cuda, i, luts):
    from madm_amd import _lib_data, data
    (_ih, in_w), (rh, rw), _w = du.RESIZE_CASES[i]
    lut1 = data.deliver_lut() if "lut1" in luts else None
    lut2 = data.convert_lut([[0, 255], [1, 0], [2, 7], [7, 2], [254, 3]]) if "lut2" in luts else None
    d1 = torch.from_numpy(lut1).cuda() if lut1 is not None else None
    d2 = torch.from_numpy(lut2).cuda() if lut2 is not None else None
    for px in (1, 3):                                           # HW, and channel 0 of HWC (the DELIVER labels)
        a, in_h, _b, resized = _case(i, px, px == 1)
        src = torch.from_numpy(a).cuda()
        yt, xt = _dev_table("nearest", in_h, rh), _dev_table("nearest", in_w, rw)
        for y0, x0, ch, cw in _crops(rh, rw):
            for flip in (0, 1):
                g = GuardedPlanes(1, ch, cw, torch.int64)
                hist = torch.full((64 + 256 + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                hist[64:320] = 0
                rc = _lib_data.lib.mdata_prep_label_u8(
                    src.data_ptr(), px, src.shape[1] * px, in_h, in_w, _ptr(yt), _ptr(xt), rh, rw, y0, x0, ch, cw, flip,
                    _ptr(d1), _ptr(d2), hist[64:].data_ptr(), g.view.data_ptr(), g.ld,
                    torch.cuda.current_stream().cuda_stream)
                assert rc == 0, _lib_data.last_error()
                want, want_hist = du.prep_label_ref(resized, None, (y0, x0, ch, cw, flip), lut1=du.deliver_lut() if lut1 is not None
                                                    else None, lut2=lut2)
                what = f"prep_label px={px} crop {ch} x {cw} at ({y0}, {x0}) flip {flip} {luts}"
                g.check(what)
                assert np.array_equal(g.view.cpu().numpy(), want), what
                h = hist.cpu().numpy()
                assert np.array_equal(h[64:320], want_hist) and h[64:320].sum() == ch * cw, what     # == np.bincount
                assert (h[:64] == 0x5A5A5A5A).all() and (h[320:] == 0x5A5A5A5A).all(), what


def test_entry_points_refuse_bad_arguments(cuda):
    from madm_amd import _lib_data
    a, in_h, _r, _n = _case(0, 3)
    (_ih, in_w), (rh, rw), _w = du.RESIZE_CASES[0]
    src = torch.from_numpy(a).cuda()
    g = GuardedPlanes(3, 8, 8, torch.float32)
    args = dict(y0=0, x0=0, ch=8, cw=8, flip=0)
    assert _prep_image(src, 3, in_h, in_w, rh, rw, out_view=g.view, ld=g.ld, plane=g.rows * g.ld, **args) == 0
    torch.cuda.synchronize()
    g = GuardedPlanes(3, 8, 8, torch.float32)
    INVALID = _lib_data.MDATA_ERR_INVALID_ARG
    assert _prep_image(src, 3, in_h, in_w, rh, rw, out_view=g.view, ld=g.ld, plane=g.rows * g.ld,
                       **dict(args, y0=rh - 7)) == INVALID and "leaves" in _lib_data.last_error()
    assert _prep_image(src, 2, in_h, in_w, rh, rw, out_view=g.view, ld=g.ld, plane=g.rows * g.ld, **args) == INVALID
    assert _prep_image(src, 3, in_h, in_w, rh, rw, out_view=g.view, ld=7, plane=g.rows * g.ld, **args) == INVALID

    class Odd:          # a float pointer two bytes off
        def data_ptr(self):
            return g.view.data_ptr() + 2
    assert _prep_image(src, 3, in_h, in_w, rh, rw, out_view=Odd(), ld=g.ld, plane=g.rows * g.ld, **args) == INVALID
    assert "aligned" in _lib_data.last_error()
    # a scale factor above 8: 18 taps
    hb = _dev_table("bilinear", in_w, rw)
    rc = _lib_data.lib.mdata_prep_image_u8(src.data_ptr(), 3, in_w * 3, in_h, in_w, _ptr(hb[0]), _ptr(hb[1]), 18, None, None, 0,
                                           in_h, rw, 0, 0, 8, 8, 0, g.view.data_ptr(), g.ld, g.rows * g.ld,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == INVALID and "above 8" in _lib_data.last_error()
    lab = GuardedPlanes(1, 8, 8, torch.int64)
    rc = _lib_data.lib.mdata_prep_label_u8(src.data_ptr(), 3, in_w * 3, in_h, in_w, None, None, rh, rw, 0, 0, 8, 8, 0, None, None,
                                           None, lab.view.data_ptr(), lab.ld, torch.cuda.current_stream().cuda_stream)
    assert rc == INVALID and "table" in _lib_data.last_error()          # a resize without its tables
    torch.cuda.synchronize()
    assert bool((g.ibuf == g.pattern).all()) and bool((lab.ibuf == lab.pattern).all())      # a refused call launches nothing


# ---- the dataset -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return du.make_tree(str(tmp_path_factory.mktemp("data_tree")))


def _seed(idx):
    random.seed(du.seed_of(idx))
    np.random.seed(du.seed_of(idx))


def test_dataset_equals_the_reference_fixture(cuda, tree):
    from madm_amd import data
    golden = np.load(du.GOLDEN)
    json_path, src, tgt = tree
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.train_kwargs())
    for idx in du.TRAIN_INDICES:
        _seed(idx)
        s = ds[idx]
        assert sorted(s) == sorted(["source_rgb", "source_label", "target_second_modality", "width", "height"])
        assert (s["width"], s["height"]) == tuple(golden[du.golden_key("train", idx, "meta")]) == (20, 16)
        for k in ("source_rgb", "source_label", "target_second_modality"):
            g = golden[du.golden_key("train", idx, k)]
            assert s[k].is_cuda and s[k].is_contiguous() and s[k].cpu().numpy().dtype == g.dtype
            assert np.array_equal(s[k].cpu().numpy(), g), (idx, k)
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.eval_kwargs())
    for idx in du.EVAL_INDICES:
        s = ds[idx]
        assert sorted(s) == sorted(["target_second_modality", "file_name", "width", "height", "pred_save_name", "target_label"])
        rel = ds.json["target_data"]["label"][idx % 2]
        assert s["file_name"] == os.path.join(tgt, rel)
        assert s["pred_save_name"] == "_".join(rel.split("/")[-4:]) == f"cloud_test_MAP_{idx % 2}_{idx % 2:06d}_semantic_front.png"
        assert (s["width"], s["height"]) == tuple(golden[du.golden_key("test", idx, "meta")])
        for k in ("target_second_modality", "target_label"):
            assert np.array_equal(s[k].cpu().numpy(), golden[du.golden_key("test", idx, k)]), (idx, k)
    # without test_resize_h_w: the file as it is, no label, width / height swapped as in the reference
    ds = data.CrossModalityDataset(json_path, src, tgt, train_or_test="test")
    s = ds[1]
    assert "target_label" not in s and tuple(s["target_second_modality"].shape) == (3, 64, 64)
    from madm_amd import png_read
    raw = png_read.read_png(os.path.join(tgt, ds.json["target_data"]["second_modality"][1]))
    assert np.array_equal(s["target_second_modality"].cpu().numpy(), du.prep_image_ref(raw, None))


def test_unsupported_files_are_refused_by_name(cuda, tmp_path):
    from madm_amd import data
    json_path, src, tgt = du.make_tree(str(tmp_path))
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.train_kwargs())
    rgb0 = os.path.join(src, ds.json["source_data"]["RGB"][0])
    du.write_png(rgb0, np.zeros((48, 96), dtype=np.uint16))
    with pytest.raises(ValueError, match="img_0.png.*uint16"):
        ds[0]
    rgba = np.random.RandomState(0).randint(0, 256, size=(48, 96, 4)).astype(np.uint8)
    du.write_png(rgb0, rgba)
    with pytest.raises(NotImplementedError, match="transparency"):
        ds[0]
    rgba[:, :, 3] = 255
    du.write_png(rgb0, rgba)
    _seed(0)
    plan = ds.plan(0)
    want = du.sample_from_plan(ds, plan)["source_rgb"]
    assert np.array_equal(ds.produce(plan)["source_rgb"].cpu().numpy(), want)       # opaque RGBA: alpha dropped
    du.write_png(os.path.join(src, ds.json["source_data"]["label"][1]), rgba[:, :, :3])
    with pytest.raises(ValueError, match="single-channel"):
        ds[1]


def test_sample_is_complete_on_another_stream(cuda, tree):
    """The hand-over is on the device: with the dataset's stream held back, a consumer stream that copies the sample right
    behind ``__getitem__`` -- no host sync anywhere -- still reads the finished tensors."""
    from madm_amd import data
    golden = np.load(du.GOLDEN)
    json_path, src, tgt = tree
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.train_kwargs())
    _seed(0)
    ds[0]                                   # tables uploaded, stream created
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    copies = []
    for idx in du.TRAIN_INDICES:
        _seed(idx)
        with torch.cuda.stream(ds._device_stream()):
            torch.cuda._sleep(4_000_000)    # a few milliseconds of delay in front of the sample's launches
        with torch.cuda.stream(side):
            s = ds[idx]
            copies.append({k: s[k].clone() for k in ("source_rgb", "source_label", "target_second_modality")})
            del s
    side.synchronize()
    for idx, c in zip(du.TRAIN_INDICES, copies):
        for k, v in c.items():
            assert np.array_equal(v.cpu().numpy(), golden[du.golden_key("train", idx, k)]), (idx, k)


def test_train_loader_stream_prefetch_and_resume(cuda, tree):
    from madm_amd import data
    json_path, src, tgt = tree
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.train_kwargs())

    def take(loader, n):
        out = []
        for _ in range(n):
            batch = next(loader)
            assert isinstance(batch, list) and len(batch) == 2
            out.append([{k: v.cpu().numpy() for k, v in s.items() if torch.is_tensor(v)} for s in batch])
        return out

    def same(a, b):
        return all(np.array_equal(x[k], y[k]) for ba, bb in zip(a, b) for x, y in zip(ba, bb) for k in x) and len(a) == len(b)

    _seed(5)
    l0 = data.build_train_loader(ds, local_batch_size=2, seed=3, prefetch=0, num_workers=2)
    ref = take(l0, 5)
    _seed(5)
    l2 = data.build_train_loader(ds, total_batch_size=2, seed=3, prefetch=2, num_workers=3)
    assert same(take(l2, 5), ref)           # drawing ahead changes when a draw happens, not which
    l2.close()
    # resume with prefetch = 0: the generator states and the sampler's position after 2 batches give batches 3 .. 5 again
    _seed(5)
    la = data.build_train_loader(ds, local_batch_size=2, seed=3, prefetch=0, num_workers=2)
    take(la, 2)
    state = (random.getstate(), np.random.get_state(), la.state_dict())
    assert state[2]["consumed"] == 4
    la.close()
    random.seed(0)
    np.random.seed(0)
    lb = data.build_train_loader(ds, local_batch_size=2, seed=3, prefetch=0, num_workers=2)
    random.setstate(state[0])
    np.random.set_state(state[1])
    lb.load_state_dict(state[2])
    assert same(take(lb, 3), ref[2:])
    lb.close()
    l0.close()


def test_inference_on_dataset_takes_the_test_loader(cuda, tmp_path):
    """Drop-in use, in the loader's steady state: 12 images with 12 different labels -- many more than are launched ahead, so
    samples are planned, launched, handed over, dropped and their memory reused while earlier images are still in flight --
    give the confusion matrix of the same images fed as host tensors.  Every slot stream is held back in front of
    ``process``, so the label is read long after the loop has dropped the sample: a label whose memory went back to the
    loader's stream too early would be counted with a later sample's values."""
    from madm_amd import data
    from madm_amd.evaluation import SemSegEvaluator, inference_on_dataset
    from test_eval_gpu import _build_product
    N = 12
    json_path, src, tgt = du.make_tree(str(tmp_path), n_target=N)
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.eval_kwargs())
    loader = data.build_test_loader(ds, num_workers=2, prefetch=2)
    assert len(loader) == N
    host = []
    for idx in range(len(ds)):
        ref = du.sample_from_plan(ds, ds.plan(idx))
        host.append([{k: torch.from_numpy(v) for k, v in ref.items()}])
    assert len({h[0]["target_label"].numpy().tobytes() for h in host}) == N

    class Late(SemSegEvaluator):
        def process(self, inputs, outputs):
            torch.cuda._sleep(2_000_000)        # the slot's stream reaches the label well after the host moved on
            super().process(inputs, outputs)

    model = _build_product("DEPTH", torch.float16)
    K = 11
    ev_dev, ev_host = Late(K, ignore_label=255), SemSegEvaluator(K, ignore_label=255)
    res_dev = inference_on_dataset(model, loader, ev_dev, streams=2)
    res_host = inference_on_dataset(model, host, ev_host, streams=2)
    loader.close()
    conf = ev_dev.confusion()
    valid = sum(int((h[0]["target_label"] != 255).sum()) for h in host)
    assert conf[:, :K].sum() == valid and conf.sum() == N * 32 * 32
    assert np.array_equal(conf, ev_host.confusion())
    assert res_dev["sem_seg"]["mIoU"] == res_host["sem_seg"]["mIoU"]
