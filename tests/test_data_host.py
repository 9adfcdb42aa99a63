"""Host-side checks of the dataset pipeline (madm_amd/data.py, madm_amd/png_read.py, libmadm_data.so's host function):
the resize recipe against PIL, the PNG reader, the draw order, the reference's own ``__getitem__`` against the recipe and the
recorded fixture, the constructor.  No GPU: what the kernels make of the same tables is tests/test_data_gpu.py."""
import inspect
import io
import json
import os
import random
import struct
import zlib

import numpy as np
import pytest

import data_util as du
import sidelib_util as su


def _random_image(rng, h, w, C):
    return rng.randint(0, 256, size=(h, w) if C == 1 else (h, w, C)).astype(np.uint8)


# ---- 1. the restatement against PIL; the product's tables against the restatement's ----------------------------------------

@pytest.mark.parametrize("case", du.RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
@pytest.mark.parametrize("C", [1, 3])
def test_restatement_equals_pil(case, C):
    Image = pytest.importorskip("PIL.Image")
    (ih, iw), (oh, ow), window = case
    a = _random_image(np.random.RandomState(ih * 7 + C), ih, iw, C)
    a = a if window is None else np.ascontiguousarray(a[:window])
    for name, fn, resample in (("BILINEAR", du.resize_bilinear, Image.BILINEAR), ("NEAREST", du.resize_nearest, Image.NEAREST)):
        pil = np.array(Image.fromarray(a).resize((ow, oh), resample))
        mine = fn(a, oh, ow)
        bad = int((pil != mine).sum())
        print(f"{name} {a.shape} -> {(oh, ow)}: {bad} mismatching samples")
        assert bad == 0, name


@pytest.mark.parametrize("case", du.RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_product_tables_equal_the_restatements(case):
    from madm_amd import data
    (ih, iw), (oh, ow), window = case
    ih = ih if window is None else window
    for i, o in ((ih, oh), (iw, ow)):
        if i == o:
            continue
        bounds, coef = data.bilinear_table(i, o)
        rb, rc, k = du.bilinear_coeffs(i, o)
        assert bounds.dtype == coef.dtype == np.int32 and coef.shape == (o, k) and k <= data.MAX_TAPS
        assert np.array_equal(bounds, np.asarray(rb)) and np.array_equal(coef, np.asarray(rc))
        tab = data.nearest_table(i, o)
        assert tab.dtype == np.int32 and np.array_equal(tab, np.asarray(du.nearest_index(i, o)))
        assert tab.min() >= 0 and tab.max() < i and (bounds[:, 0] + bounds[:, 1]).max() <= i


def test_scale_above_8_is_refused():
    from madm_amd import data
    data.bilinear_table(640, 80)
    with pytest.raises(ValueError, match="above 8"):
        data.bilinear_table(641, 80)


def test_label_tables():
    from madm_amd import data
    lut1 = data.deliver_lut()
    v = np.arange(256, dtype=np.uint8)
    ref = v.copy()
    mask = ref == 255
    ref -= 1                        # uint8 arithmetic, as the reference's tensor: 0 wraps to 255
    ref[mask] = 255
    assert np.array_equal(lut1, ref) and lut1[0] == 255 and lut1[255] == 255 and lut1[1] == 0
    pairs = [[1, 2], [2, 3], [7, 0], [300, 5], [1, 9]]
    out = v.astype(np.int64)
    for old, new in pairs:          # the reference's loop: every pair compares against the ORIGINAL labels
        out[v == old] = new
    assert np.array_equal(data.convert_lut(pairs), out.astype(np.uint8)) and np.array_equal(du.convert_lut(pairs), out)
    with pytest.raises(ValueError):
        data.convert_lut([[1, 256]])


# ---- 2. the PNG reader -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4, "mixed"])
def test_png_round_trip(filt):
    from madm_amd import png_read
    rng = np.random.RandomState(3)
    for shape, dtype in (((11, 7), np.uint8), ((11, 7, 3), np.uint8), ((11, 7, 4), np.uint8), ((6, 5), np.uint16), ((1, 1), np.uint8),
                         ((3, 1, 3), np.uint8)):
        a = rng.randint(0, 65536 if dtype == np.uint16 else 256, size=shape).astype(dtype)
        a.reshape(-1)[::5] = a.reshape(-1)[0]           # some runs: smooth rows exercise every predictor branch
        filters = [(3 * y + 1) % 5 for y in range(shape[0])] if filt == "mixed" else filt
        got = png_read.decode_png(du.png_bytes(a, filters=filters))
        assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a)
    idx = rng.randint(0, 256, size=(9, 13)).astype(np.uint8)
    got, colour = png_read.decode_png(du.png_bytes(idx, filters=filters, colour_type=3), with_colour_type=True)
    assert colour == 3 and np.array_equal(got, idx)         # palette files give their indices


def test_png_reader_agrees_with_pil():
    Image = pytest.importorskip("PIL.Image")
    from madm_amd import png_read
    rng = np.random.RandomState(4)
    for mode, shape in (("L", (17, 23)), ("RGB", (17, 23, 3)), ("RGBA", (17, 23, 4)), ("P", (17, 23))):
        a = rng.randint(0, 256, size=shape).astype(np.uint8)
        a[:, :12] = a[:, :1]
        img = Image.fromarray(a, mode="L" if mode == "P" else mode)
        if mode == "P":
            img = img.copy()
            img.putpalette([i % 256 for i in range(768)])       # 'L' data under a palette: mode 'P', the same indices
            assert img.mode == "P"
        buf = io.BytesIO()
        img.save(buf, format="PNG", optimize=True)              # PIL chooses the filters
        assert np.array_equal(png_read.decode_png(buf.getvalue()), np.array(img))
        if mode != "P":                                          # and PIL reads the test writer's files
            mine = du.png_bytes(a, filters=[y % 5 for y in range(17)])
            assert np.array_equal(np.array(Image.open(io.BytesIO(mine))), a)


def test_png_reader_refuses_bad_files(tmp_path):
    from madm_amd import png_read
    a = np.random.RandomState(5).randint(0, 256, size=(12, 9, 3)).astype(np.uint8)
    good = du.png_bytes(a, filters=4)
    assert np.array_equal(png_read.decode_png(good), a)
    with pytest.raises(ValueError, match="truncated"):
        png_read.decode_png(good[:len(good) - 20])
    with pytest.raises(ValueError, match="truncated|IDAT holds"):
        png_read.decode_png(good[:60])
    short = zlib.compress(du.filter_rows(a.reshape(12, 27), 3, 1).tobytes()[:-30])
    with pytest.raises(ValueError, match="IDAT holds"):     # well-formed chunks, too few scanline bytes
        png_read.decode_png(b"\x89PNG\r\n\x1a\n" + du._chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 12, 8, 2, 0, 0, 0))
                            + du._chunk(b"IDAT", short) + du._chunk(b"IEND", b""))
    flipped = bytearray(good)
    flipped[50] ^= 0x10
    with pytest.raises(ValueError, match="CRC"):
        png_read.decode_png(bytes(flipped))
    with pytest.raises(ValueError, match="filter type 5"):
        png_read.decode_png(du.png_bytes(a, filters=[0, 1, 5] + [2] * 9))
    with pytest.raises(ValueError, match="interlace"):
        png_read.decode_png(du.png_bytes(a, interlace=1))
    with pytest.raises(ValueError, match="bit depth 4"):
        png_read.decode_png(du.png_bytes(a[:, :, 0], bit_depth=4))
    with pytest.raises(ValueError, match="colour type 4"):
        png_read.decode_png(du.png_bytes(a[:, :, 0], colour_type=4))
    with pytest.raises(ValueError, match="signature"):
        png_read.decode_png(b"JFIF" + good[4:])
    path = tmp_path / "bad.png"
    path.write_bytes(du.png_bytes(a, interlace=1))
    with pytest.raises(ValueError, match="bad.png.*interlace"):     # the file and the field are named
        png_read.read_png(str(path))
    assert png_read.png_size(str(path)) == (9, 12)


def test_unfilter_native_status_and_containment():
    from madm_amd import _lib_data
    lib = _lib_data.lib
    a = np.random.RandomState(6).randint(0, 256, size=(6, 10)).astype(np.uint8)
    rows = du.filter_rows(a, 2, [1, 2, 3, 5, 4, 0])             # row 3 carries filter byte 5
    out = np.full(6 * 10 + 32, 0xA5, dtype=np.uint8)
    rc = lib.mdata_png_unfilter(rows.ctypes.data, rows.size, out.ctypes.data + 16, 60, 6, 10, 2)
    assert rc == _lib_data.MDATA_ERR_FORMAT and "row 3" in _lib_data.last_error()
    body = out[16:76].reshape(6, 10)
    assert np.array_equal(body[:3], a[:3])                      # the rows in front of it are decoded,
    assert (body[3:] == 0xA5).all()                             # the bad row and everything behind it untouched,
    assert (out[:16] == 0xA5).all() and (out[76:] == 0xA5).all()   # and nothing outside ``out``
    # inconsistent lengths: refused before anything is read or written
    for in_len, out_len, h, rb, bpp in ((rows.size - 1, 60, 6, 10, 2), (rows.size, 59, 6, 10, 2), (rows.size, 60, 6, 10, 0),
                                        (rows.size, 60, 6, 10, 9), (rows.size, 60, 0, 10, 2), (rows.size, 60, -1, 10, 2)):
        out[:] = 0xA5
        assert lib.mdata_png_unfilter(rows.ctypes.data, in_len, out.ctypes.data + 16, out_len, h, rb, bpp) == \
            _lib_data.MDATA_ERR_INVALID_ARG
        assert (out == 0xA5).all()
    good = du.filter_rows(a, 2, [4, 3, 2, 1, 0, 4])
    out[:] = 0xA5
    assert lib.mdata_png_unfilter(good.ctypes.data, good.size, out.ctypes.data + 16, 60, 6, 10, 2) == 0
    assert np.array_equal(out[16:76].reshape(6, 10), a) and (out[:16] == 0xA5).all() and (out[76:] == 0xA5).all()
    assert lib.mdata_abi_version() == _lib_data.ABI_VERSION


def test_data_header_keeps_out_of_the_main_abi():
    import ctypes
    from madm_amd import _cabi, _lib_data
    abi = _cabi.parse_packaged("madm_data.h")
    declared = {n for n, _r, _p in abi.prototypes}
    assert len(declared) == 5 and all(n.startswith("mdata_") for n in declared)        # no madm_* function,
    assert all(n.startswith("MDATA_") for n in abi.constants) and not abi.structs       # constant or struct
    assert declared == {n for n, _r, _a in _lib_data.SYMBOLS}
    built = ctypes.CDLL(_lib_data.LIB_PATH)
    assert all(hasattr(built, n) for n in declared) and not hasattr(built, "madm_abi_version")
    import madm_amd
    assert "_lib_data" not in open(madm_amd.__file__).read()        # package import does not load the second library


# ---- 3. draw order ---------------------------------------------------------------------------------------------------------

class _Tree:
    """Arrays instead of files: a stub decoder serves them by path."""

    def __init__(self, tmp_path, rcs):
        rng = np.random.RandomState(11)
        self.files = {}
        self.src, self.tgt = str(tmp_path / "src"), str(tmp_path / "tgt") + os.sep
        os.makedirs(self.src, exist_ok=True)
        js = {"source_data": {"RGB": [], "label": []}, "target_data": {"second_modality": [], "label": []}}
        stats, with_class = [], {}
        for i in range(4):
            rgb, lab = f"rgb/{i}.png", f"lab/{i}.png"
            self.files[os.path.join(self.src, rgb)] = rng.randint(0, 256, size=(48, 96, 3)).astype(np.uint8)
            label = rng.randint(0, 5, size=(6, 12)).astype(np.uint8).repeat(8, 0).repeat(8, 1)
            self.files[os.path.join(self.src, lab)] = label
            js["source_data"]["RGB"].append(rgb)
            js["source_data"]["label"].append(lab)
            counts = np.bincount(label.reshape(-1), minlength=5)
            stats.append({"file": lab, **{str(c): int(n) * (1 + 9 * c) for c, n in enumerate(counts) if n}})
            for c, n in enumerate(counts):
                if n:
                    with_class.setdefault(str(c), []).append([lab, int(n) * 100])
        for i in range(3):
            d = f"depth/{i}.png"
            self.files[os.path.join(self.tgt, d)] = rng.randint(0, 256, size=(64, 64)).astype(np.uint8)
            js["target_data"]["second_modality"].append(d)
            js["target_data"]["label"].append(f"a/b/c/{i}.png")
        self.json_path = str(tmp_path / "Cityscapes_RGB_to_DELIVER_Depth_stub.json")
        with open(self.json_path, "w") as f:
            json.dump(js, f)
        if rcs:
            with open(os.path.join(self.src, "sample_class_stats.json"), "w") as f:
                json.dump(stats, f)
            with open(os.path.join(self.src, "samples_with_class.json"), "w") as f:
                json.dump(with_class, f)

    def decoder(self, path):
        return self.files[path]


def _dataset_class():
    from madm_amd import data

    class HostCounted(data.CrossModalityDataset):
        """The rare-class count from the restatement instead of the device histogram: the draws are what is under test."""
        rcs_min_pixels = 60         # 30 pixels of the class inside a 16 x 20 crop: some tries pass, some do not

        def _rcs_count(self, plan, crop, c):
            lab, _ = plan.files["source_label"].array()
            crop5 = (crop.y, crop.x, self.source_crop_size_h_w[0], self.source_crop_size_h_w[1], crop.flip)
            return int(du.prep_label_ref(lab, self.source_resize_h_w, crop5)[1][c])
    return HostCounted


@pytest.mark.parametrize("rcs", [False, True])
def test_draw_order(tmp_path, rcs):
    tree = _Tree(tmp_path, rcs)
    kw = dict(du.train_kwargs(), label_convert=None, rare_class_sample=rcs, decoder=tree.decoder)
    ds = _dataset_class()(tree.json_path, tree.src, tree.tgt, **kw)
    assert len(ds) == 4 * 3 and (ds.source_data_width, ds.source_data_height) == (96, 48)
    random.seed(21)
    np.random.seed(22)
    plans = [ds.plan(idx) for idx in range(14)]
    after = (random.random(), np.random.random_sample())

    # the restatement of the reference's draws (cross_modality_dataset.py:266-269, 302-318, 443-445), same seeds
    random.seed(21)
    np.random.seed(22)
    (srh, srw), (sch, scw) = ds.source_resize_h_w, ds.source_crop_size_h_w
    (trh, trw), (tch, tcw) = ds.target_resize_h_w, ds.target_crop_size_h_w

    def draw(rh, rw, ch, cw):
        flip = random.random() < 0.5
        x = random.randint(0, rw - cw)
        y = random.randint(0, rh - ch)
        return flip, x, y

    n_tries = []
    for idx, plan in enumerate(plans):
        if rcs:
            c = np.random.choice(ds.rcs_classes, p=ds.rcs_classprob)
            f1 = np.random.choice(ds.samples_with_class[c])
            source_idx = ds.file_to_idx[f1]
            lab = tree.files[os.path.join(tree.src, ds.json['source_data']['label'][source_idx])]
            tries = [draw(srh, srw, sch, scw)]
            for _ in range(10):
                flip, x, y = tries[-1]
                if du.prep_label_ref(lab, (srh, srw), (y, x, sch, scw, flip))[1][c] > ds.rcs_min_pixels * ds.rcs_min_crop_ratio:
                    break
                tries.append(draw(srh, srw, sch, scw))
            assert (plan.rcs_class, plan.rcs_file) == (c, f1)
            n_tries.append(len(tries))
        else:
            source_idx = idx % 4
            tries = [draw(srh, srw, sch, scw)]
            assert plan.rcs_class is None and plan.rcs_file is None
        assert plan.source_idx == source_idx and plan.target_idx == idx % 3
        assert [t.astuple() for t in plan.source_tries] == tries and plan.source.astuple() == tries[-1]
        assert plan.target.astuple() == draw(trh, trw, tch, tcw)
    assert after == (random.random(), np.random.random_sample())        # and not one draw more
    if rcs:
        assert min(n_tries) == 1 and max(n_tries) > 1, n_tries          # both the accepted first crop and re-crops occurred


def test_rcs_class_probs_follow_the_reference_formula(tmp_path):
    import torch
    tree = _Tree(tmp_path, True)
    from madm_amd import data
    classes, prob = data.rcs_class_probs(tree.src, 0.01)
    stats = json.load(open(os.path.join(tree.src, "sample_class_stats.json")))
    total = {}
    for s in stats:
        for k, v in s.items():
            if k != "file":
                total[int(k)] = total.get(int(k), 0) + v
    order = sorted(total, key=lambda k: total[k])
    assert classes == order
    freq = torch.tensor([total[k] for k in order])
    want = torch.softmax((1 - freq / freq.sum()) / 0.01, dim=-1).numpy()
    assert prob.dtype == np.float32 and np.array_equal(prob, want)


# ---- 4. the reference's __getitem__, the restatement and the fixture on the product's own plan ---------------------------

@pytest.mark.skipif(not os.path.exists(du.REFERENCE_FILE), reason="the reference checkout is not on this machine")
def test_reference_pin(tmp_path):
    pytest.importorskip("PIL.Image")
    from madm_amd import data
    json_path, src, tgt = du.make_tree(str(tmp_path))
    Ref = du.load_reference_class()
    golden = np.load(du.GOLDEN)
    checked = 0
    for mode, kwargs, indices in (("train", du.train_kwargs(), du.TRAIN_INDICES), ("test", du.eval_kwargs(), du.EVAL_INDICES)):
        ds = data.CrossModalityDataset(json_path, src, tgt, **kwargs)
        ref = Ref(json_path, src, tgt, **kwargs)
        assert len(ds) == len(ref) and ds.deliver_label_process == ref.deliver_label_process
        assert (ds.target_data_width, ds.target_data_height) == (ref.target_data_width, ref.target_data_height)
        for idx in indices:
            random.seed(du.seed_of(idx))
            np.random.seed(du.seed_of(idx))
            plan = ds.plan(idx)
            mine = du.sample_from_plan(ds, plan)
            random.seed(du.seed_of(idx))
            np.random.seed(du.seed_of(idx))
            theirs = ref[idx]
            keys = [k for k in du.TENSOR_KEYS if k in theirs]
            assert sorted(keys) == sorted(mine)
            for k in keys:
                t = theirs[k].numpy()
                g = golden[du.golden_key(mode, idx, k)]
                assert t.dtype == mine[k].dtype == g.dtype and t.shape == mine[k].shape == g.shape, (mode, idx, k)
                assert np.array_equal(t, mine[k]), (mode, idx, k, "reference vs restatement")
                assert np.array_equal(t, g), (mode, idx, k, "reference vs fixture")
                checked += 1
            assert list(golden[du.golden_key(mode, idx, "meta")]) == [theirs["width"], theirs["height"]]
    assert checked == 6 * 3 + 3 * 2


def test_fixture_equals_restatement_on_the_products_plan(tmp_path):
    """The same pin without the reference checkout: fixture == restatement on the product's plan, and the non-tensor entries."""
    from madm_amd import data
    json_path, src, tgt = du.make_tree(str(tmp_path))
    golden = np.load(du.GOLDEN)
    flips = set()
    for mode, kwargs, indices in (("train", du.train_kwargs(), du.TRAIN_INDICES), ("test", du.eval_kwargs(), du.EVAL_INDICES)):
        ds = data.CrossModalityDataset(json_path, src, tgt, **kwargs)
        for idx in indices:
            random.seed(du.seed_of(idx))
            np.random.seed(du.seed_of(idx))
            plan = ds.plan(idx)
            if mode == "train":
                flips |= {plan.source.flip, plan.target.flip}
            for k, v in du.sample_from_plan(ds, plan).items():
                g = golden[du.golden_key(mode, idx, k)]
                assert g.dtype == v.dtype and np.array_equal(g, v), (mode, idx, k)
    assert flips == {False, True}           # the fixture's seeds cover both


# ---- 5. constructor and unsupported options --------------------------------------------------------------------------------

def test_constructor_signature_and_unsupported_options(tmp_path):
    from madm_amd import data
    names = list(inspect.signature(data.CrossModalityDataset.__init__).parameters)
    assert names == ["self", "json_path", "source_root_path", "target_root_path", "source_resize_h_w", "source_crop_size_h_w",
                     "target_resize_h_w", "target_crop_size_h_w", "test_resize_h_w", "train_or_test", "label_convert",
                     "remove_amp", "fda_fusion_val", "rare_class_sample", "remove_texture", "merge_more_target_data",
                     "pl_data_path", "kwargs"]
    json_path, src, tgt = du.make_tree(str(tmp_path))
    for option, value in (("remove_amp", [0.01, 0.1]), ("fda_fusion_val", [0.1, 0.2]), ("remove_texture", True),
                          ("merge_more_target_data", "more"), ("pl_data_path", "/pl")):
        with pytest.raises(NotImplementedError, match=option):
            data.CrossModalityDataset(json_path, src, tgt, **dict(du.train_kwargs(), **{option: value}))
    with pytest.raises(AssertionError):
        data.CrossModalityDataset(json_path.replace("Cityscapes_RGB_to_DELIVER_Depth", "other"), src, tgt, **du.train_kwargs())
    train = data.CrossModalityDataset(json_path, src, tgt, **du.train_kwargs())
    test = data.CrossModalityDataset(json_path, src, tgt, **du.eval_kwargs())
    assert len(train) == 3 * 2 and len(test) == 2
    assert not train.deliver_label_process and test.deliver_label_process      # 'to_DELIVER_Depth' + test (:187-188)


def test_loader_pool_and_samplers(tmp_path):
    import torch
    from madm_amd import data
    for name in ("data", "png_read", "_lib_data"):
        src_text = open(os.path.join(os.path.dirname(data.__file__), name + ".py")).read()
        assert "cpu_count" not in src_text
        for lib in ("PIL", "cv2", "imageio", "torchvision", "detectron2"):
            assert f"import {lib}" not in src_text and f"from {lib}" not in src_text
    json_path, src, tgt = du.make_tree(str(tmp_path))
    ds = data.CrossModalityDataset(json_path, src, tgt, **du.train_kwargs())
    loader = data.build_train_loader(ds, local_batch_size=2, num_workers=1000, seed=7)
    assert loader._pool._max_workers == data.MAX_WORKERS == 16
    loader.close()
    with pytest.raises(ValueError):
        data.build_train_loader(ds, total_batch_size=4, local_batch_size=2)
    with pytest.raises(ValueError):
        data.build_train_loader(ds, total_batch_size=3, world_size=2)
    # detectron2's TrainingSampler: one seeded randperm stream, reshuffled every pass, strided by rank
    g = torch.Generator()
    g.manual_seed(7)
    stream = sum((torch.randperm(len(ds), generator=g).tolist() for _ in range(5)), [])
    for rank in range(3):
        ld = data.build_train_loader(ds, total_batch_size=6, world_size=3, rank=rank, seed=7, num_workers=1)
        assert ld.batch_size == 2
        it = ld._sampler(0)
        assert [next(it) for _ in range(9)] == stream[rank::3][:9]
        it = ld._sampler(4)                                     # resumed behind 4 consumed entries
        assert [next(it) for _ in range(5)] == stream[rank::3][4:9]
        ld.close()
    # InferenceSampler: contiguous shards, the first ``total % world`` one longer
    test = data.CrossModalityDataset(json_path, src, tgt, **du.eval_kwargs())
    test.target_data_length = 11
    shards = []
    for rank in range(4):
        ld = data.build_test_loader(test, world_size=4, rank=rank, num_workers=1)
        shards.append(list(ld.indices))
        ld.close()
    assert [len(s) for s in shards] == [3, 3, 3, 2] and sum(shards, []) == list(range(11))


# ---- 6. the second library's code objects: the pins tests/test_host.py holds libmadm_hip.so to ----------------------------

def test_data_kernels_use_no_scratch_and_no_packed_fp32():
    """libmadm_data.so is built with the main library's flags (packed-FP32 ops off) and its kernels
    must not spill: read from the built library with the project's two scanners."""
    from madm_amd._lib_data import LIB_PATH
    rows = su.scan_kernels(LIB_PATH)
    names = " ".join(rows)
    assert len(rows) == 2 and "prep_image_kernel" in names and "prep_label_kernel" in names, list(rows)
