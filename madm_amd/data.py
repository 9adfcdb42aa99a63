"""Device-side dataset pipeline: PNG files to training and evaluation batches.

``CrossModalityDataset`` restates the reference's dataset of the same name (data/dataset/cross_modality_dataset.py:145-521)
for the native loop.  The reference is a CPU program -- PIL resize / crop / flip, numpy transposes and casts, a Python loop
of masked assignments over the labels -- inside detectron2's loaders.  Here a file is decoded on the host (png_read.py: zlib
+ one native loop, no imaging library), uploaded as uint8, and ONE launch of libmadm_data.so turns it into the tensor the
trainer or the evaluator consumes:

  data    mdata_prep_image_u8   PIL-exact BILINEAR resize, crop, flip, gray -> 3 channels, float      f32 [3, h, w], 0 .. 255
  label   mdata_prep_label_u8   PIL-exact NEAREST resize, crop, flip, DELIVER rule, label_convert,    i64 [1, h, w]
                                and the class histogram rare-class sampling reads

Both are bit-exact with the reference's pixels (tests/test_data_host.py pins the recipe to PIL and to the reference's
``__getitem__``; tests/test_data_gpu.py holds the kernels to the recipe).  The resize tables are built here in float64 and
cached on the device per (input size, output size).

Random draws come from ``random`` and ``np.random`` in the reference's order, always on the thread that consumes the
samples: source flip, x, y; with rare-class sampling first the class, then the file, then up to 10 re-crops; then target
flip, x, y.  Everything else of a sample runs on the dataset's own stream; a sample is handed over on the device (the
caller's current stream waits for the sample's event and the tensors are ``record_stream``-ed on it) -- no host sync per
sample.  Rare-class sampling reads the histogram after each try: the one host sync, on the loader stream only."""
import json
import logging
import os
import random
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import torch

from . import png_read
from ._lib_data import MAX_TAPS           # include/madm_data.h MDATA_MAX_TAPS: scale factors up to 8

logger = logging.getLogger("madm_amd.data")

MAX_WORKERS = 16            # decode threads are never sized from the machine's core count
PRECISION_BITS = 22         # Pillow Resample.c: 32 - 8 - 2

_JSON_NAMES = ('DELIVER_RGB2Depth', 'DELIVER_Depth2RGB', 'DSEC_RGB2REvents', 'cityscapes_dsec',
               'Cityscapes_RGB_to_DELIVER_Depth', 'Cityscapes_RGB_to_DSEC_Event', 'Cityscapes_RGB_to_DSEC_19_Event',
               'Cityscapes_RGB_to_VKITTI2_Depth', 'GTA5_RGB_to_Cityscapes_RGB', 'GTA5_RGB_to_DELIVER_Depth',
               'Cityscapes_RGB_to_FMB_Infrared')


# ---- the resize tables (host, float64) -------------------------------------------------------------------------------------

def bilinear_table(in_size, out_size):
    """PIL's BILINEAR coefficients of one axis (Pillow Resample.c, precompute_coeffs + normalize_coeffs_8bpc):
    (bounds int32 [out, 2] = (first input index, taps), coef int32 [out, ksize] = int(0.5 + w * 2^22), zero behind the taps)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"bilinear_table: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    if ksize > MAX_TAPS:
        raise ValueError(f"resize {in_size} -> {out_size}: scale factor {scale:.3f} above 8 is not supported "
                         f"(a window of {ksize} taps, the kernel holds {MAX_TAPS})")
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = (np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss
        w = np.maximum(0.0, 1.0 - np.abs(w))
        ww = 0.0
        for v in w:                     # the C loop's summation order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        bounds[xx] = (xmin, n)
        coef[xx, :n] = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)      # truncation; every w >= 0
    return bounds, coef


def nearest_table(in_size, out_size):
    """PIL's NEAREST source index of one axis (Pillow Geometry.c, the affine scale path): the ACCUMULATED double sum."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"nearest_table: sizes must be positive, got {in_size} -> {out_size}")
    a = in_size / out_size
    xo = a * 0.5
    tab = np.empty(out_size, dtype=np.int32)
    for x in range(out_size):
        tab[x] = int(xo)
        xo += a
    return tab


def deliver_lut():
    """The reference's DELIVER rule on a uint8 tensor (:406-409): v -> (v - 1) & 255 with 255 kept; label 0 wraps to 255."""
    lut = (np.arange(256, dtype=np.int64) - 1) & 255
    lut[255] = 255
    return lut.astype(np.uint8)


def convert_lut(label_convert):
    """``convert_label`` (:417-421) as one table: every pair compares against the ORIGINAL tensor, so it is a plain map."""
    lut = np.arange(256, dtype=np.int64)
    for old_id, new_id in label_convert:
        old_id, new_id = int(old_id), int(new_id)
        if not 0 <= new_id <= 255:
            raise ValueError(f"label_convert: new id {new_id} does not fit the 8-bit label table")
        if 0 <= old_id <= 255:
            lut[old_id] = new_id
    return lut.astype(np.uint8)


def rcs_class_probs(data_root, temperature):
    """``get_rcs_class_probs`` (:87-109): classes sorted by pixel count, softmax((1 - freq) / T) in torch float32."""
    with open(os.path.join(data_root, 'sample_class_stats.json')) as f:
        stats = json.load(f)
    total = {}
    for s in stats:
        for c, n in s.items():
            if c == 'file':
                continue
            total[int(c)] = total.get(int(c), 0) + n
    total = dict(sorted(total.items(), key=lambda kv: kv[1]))
    freq = torch.tensor(list(total.values()))
    freq = freq / torch.sum(freq)
    freq = torch.softmax((1 - freq) / temperature, dim=-1)
    return list(total.keys()), freq.numpy()


# ---- plans -----------------------------------------------------------------------------------------------------------------

class _File:
    """One file of a sample: decoded at most once, on a pool thread when the loader has a pool."""

    def __init__(self, path, decode, submit=None):
        self.path = path
        self._decode = decode
        self._future = submit(decode, path) if submit is not None else None
        self._value = None
        self.device = None          # the uploaded uint8 tensor, once a launch needed it

    def array(self):
        if self._value is None:
            self._value = self._future.result() if self._future is not None else self._decode(self.path)
            self._future = None
        return self._value


class Crop:
    """One drawn augmentation: ``flip``, ``x``, ``y`` in the reference's draw order."""
    __slots__ = ("flip", "x", "y")

    def __init__(self, flip, x, y):
        self.flip, self.x, self.y = bool(flip), int(x), int(y)

    def astuple(self):
        return self.flip, self.x, self.y

    def __repr__(self):
        return f"Crop(flip={self.flip}, x={self.x}, y={self.y})"


class Plan:
    """Everything drawn for one sample.  ``source_idx`` / ``target_idx``: the json entries; ``source`` / ``target``: the
    Crop used; ``source_tries``: every source Crop drawn (rare-class sampling re-crops; the last one is ``source``);
    ``rcs_class`` / ``rcs_file``: the rare-class draw, or None."""

    def __init__(self):
        self.mode = None
        self.source_idx = self.target_idx = None
        self.source = self.target = None
        self.source_tries = []
        self.rcs_class = self.rcs_file = None
        self.files = {}
        self.source_label = None    # rare-class sampling has produced it already


def _default_decoder(path):
    return png_read.read_png(path, with_colour_type=True)


class CrossModalityDataset:
    """The reference's dataset on the device.  Constructor arguments, keys of a sample, index arithmetic, draw order and
    the per-dataset quirks (swapped width / height in test mode, ``target_label`` only with ``test_resize_h_w``, the
    ``pred_save_name`` formats, the DSEC 640 x 480 pre-crop) are the reference's.  Further keywords: ``device``,
    ``decoder`` (``callable(path) -> np.ndarray`` for formats png_read.py does not read)."""

    rcs_class_temp = 0.01
    rcs_min_crop_ratio = 0.5
    rcs_min_pixels = 3000

    def __init__(self, json_path, source_root_path, target_root_path, source_resize_h_w=None, source_crop_size_h_w=None,
                 target_resize_h_w=None, target_crop_size_h_w=None, test_resize_h_w=None, train_or_test='train',
                 label_convert=None, remove_amp=None, fda_fusion_val=None, rare_class_sample=False, remove_texture=False,
                 merge_more_target_data=None, pl_data_path=None, **kwargs):
        self.device = kwargs.pop("device", "cuda")
        decoder = kwargs.pop("decoder", None)
        for name, value in (("remove_amp", remove_amp), ("fda_fusion_val", fda_fusion_val), ("remove_texture", remove_texture),
                            ("merge_more_target_data", merge_more_target_data), ("pl_data_path", pl_data_path)):
            if value:
                raise NotImplementedError(f"CrossModalityDataset: {name} is not built (no shipped config sets it)")

        self.source_resize_h_w = [0, 0] if source_resize_h_w is None else list(source_resize_h_w)
        self.source_crop_size_h_w = [0, 0] if source_crop_size_h_w is None else list(source_crop_size_h_w)
        self.target_resize_h_w = [0, 0] if target_resize_h_w is None else list(target_resize_h_w)
        self.target_crop_size_h_w = [0, 0] if target_crop_size_h_w is None else list(target_crop_size_h_w)
        self.test_resize_h_w = None if test_resize_h_w is None else list(test_resize_h_w)

        self.json_path = json_path
        if not any(name in json_path for name in _JSON_NAMES):
            raise AssertionError(f"json_path {json_path!r} names none of the known dataset pairs {_JSON_NAMES}")
        # labels of DELIVER need the extra rule (:183-188)
        self.deliver_label_process = False
        if 'DELIVER_RGB2Depth' in json_path or 'DELIVER_Depth2RGB' in json_path:
            self.deliver_label_process = True
        elif 'to_DELIVER_Depth' in json_path and train_or_test == 'test':
            self.deliver_label_process = True

        self.source_root_path = source_root_path
        self.target_root_path = target_root_path
        if train_or_test not in ('train', 'test'):
            raise AssertionError(f"train_or_test is 'train' or 'test', got {train_or_test!r}")
        self.train_or_test = train_or_test
        self.label_convert = label_convert
        self.rare_class_sample = rare_class_sample

        if decoder is None:
            self._decode = _default_decoder
        else:
            self._decode = lambda path: (np.asarray(decoder(path)), None)

        with open(json_path) as f:
            self.json = json.load(f)
        if train_or_test == 'train':
            first = os.path.join(source_root_path, self.json['source_data']['RGB'][0])
            self.source_data_width, self.source_data_height = self._size_of(first, decoder)
            self.source_data_length = len(self.json['source_data']['RGB'])
            for what, resize, crop in (("source", self.source_resize_h_w, self.source_crop_size_h_w),
                                       ("target", self.target_resize_h_w, self.target_crop_size_h_w)):
                if min(resize) < 1 or min(crop) < 1 or crop[0] > resize[0] or crop[1] > resize[1]:
                    raise ValueError(f"{what}: crop {crop} must be positive and fit the resize {resize}")
        else:
            self.source_data_length = 1
        first = target_root_path + self.json['target_data']['second_modality'][0]        # the reference's plain '+' (:220)
        self.target_data_width, self.target_data_height = self._size_of(first, decoder)
        self.target_data_length = len(self.json['target_data']['second_modality'])

        self._lut1 = deliver_lut() if self.deliver_label_process else None
        self._lut2 = convert_lut(label_convert) if label_convert is not None else None
        if rare_class_sample:
            self.init_rare_class_sample()

        # device state, created at the first sample (constructing the dataset needs no GPU)
        self._lock = threading.Lock()
        self._stream = None
        self._tables = {}
        self._host_tables = {}
        self._dev_lut1 = self._dev_lut2 = None

    @staticmethod
    def _size_of(path, decoder):
        if decoder is None:
            return png_read.png_size(path)
        a = np.asarray(decoder(path))
        return a.shape[1], a.shape[0]

    def __len__(self):
        return self.source_data_length * self.target_data_length

    def init_rare_class_sample(self):
        self.rcs_classes, self.rcs_classprob = rcs_class_probs(self.source_root_path, self.rcs_class_temp)
        logger.info("RCS Classes: %s", self.rcs_classes)
        logger.info("RCS ClassProb: %s", self.rcs_classprob)
        with open(os.path.join(self.source_root_path, 'samples_with_class.json')) as f:
            by_class = {int(k): v for k, v in json.load(f).items()}
        self.samples_with_class = {}
        for c in self.rcs_classes:
            files = [file.split('/')[-1] for file, pixels in by_class[c] if pixels > self.rcs_min_pixels]
            if not files:
                raise AssertionError(f"rare-class sampling: no file with more than {self.rcs_min_pixels} pixels of class {c}")
            self.samples_with_class[c] = files
        self.file_to_idx = {name.split('/')[-1]: i for i, name in enumerate(self.json['source_data']['label'])}

    # ---- drawing (the consuming thread) -------------------------------------------------------------------------------------

    @staticmethod
    def _draw(resize_h_w, crop_h_w):
        flip = random.random() < 0.5
        x = random.randint(0, resize_h_w[1] - crop_h_w[1])
        y = random.randint(0, resize_h_w[0] - crop_h_w[0])
        return Crop(flip, x, y)

    def _source_files(self, plan, source_idx, submit):
        sd = self.json['source_data']
        plan.source_idx = source_idx
        plan.files["source_rgb"] = _File(os.path.join(self.source_root_path, sd['RGB'][source_idx]),
                                          partial(self._load_image, self.source_resize_h_w), submit)
        plan.files["source_label"] = _File(os.path.join(self.source_root_path, sd['label'][source_idx]), self._load_label, submit)

    def plan(self, idx, submit=None):
        """Draws everything sample ``idx`` needs, in the reference's order, and names its files (``submit``: a pool's
        ``submit``, so that decoding starts at once).  With rare-class sampling the source label is produced here, because
        each re-crop depends on the class count of the one before."""
        plan = Plan()
        plan.mode = self.train_or_test
        plan.target_idx = idx % self.target_data_length
        td = self.json['target_data']
        target_path = os.path.join(self.target_root_path, td['second_modality'][plan.target_idx])
        if self.train_or_test == 'test':
            plan.files["target"] = _File(target_path, partial(self._load_image, self.test_resize_h_w), submit)
            if self.test_resize_h_w is not None:
                plan.files["target_label"] = _File(os.path.join(self.target_root_path, td['label'][plan.target_idx]),
                                                   self._load_label, submit)
            return plan
        if self.rare_class_sample:
            plan.rcs_class = c = np.random.choice(self.rcs_classes, p=self.rcs_classprob)
            plan.rcs_file = f1 = np.random.choice(self.samples_with_class[c])
            self._source_files(plan, self.file_to_idx[f1], submit)
            plan.files["target"] = _File(target_path, partial(self._load_image, self.target_resize_h_w), submit)
            crop = self._draw(self.source_resize_h_w, self.source_crop_size_h_w)
            plan.source_tries.append(crop)
            if self.rcs_min_crop_ratio > 0:
                for _ in range(10):
                    if self._rcs_count(plan, crop, int(c)) > self.rcs_min_pixels * self.rcs_min_crop_ratio:
                        break
                    crop = self._draw(self.source_resize_h_w, self.source_crop_size_h_w)
                    plan.source_tries.append(crop)
                    plan.source_label = None
            plan.source = crop
        else:
            self._source_files(plan, idx % self.source_data_length, submit)
            plan.files["target"] = _File(target_path, partial(self._load_image, self.target_resize_h_w), submit)
            plan.source = self._draw(self.source_resize_h_w, self.source_crop_size_h_w)
            plan.source_tries.append(plan.source)
        plan.target = self._draw(self.target_resize_h_w, self.target_crop_size_h_w)
        return plan

    def _rcs_count(self, plan, crop, c):
        """Pixels of class ``c`` in the source label under ``crop`` (before label_convert, as the reference counts, :309):
        one launch and the histogram's read-back on the loader stream."""
        with torch.cuda.stream(self._device_stream()):
            hist = torch.zeros(256, dtype=torch.int32, device=self.device)
            plan.source_label = self._label(plan.files["source_label"], self.source_resize_h_w, self.source_crop_size_h_w,
                                            crop, hist)
            return int(hist.cpu()[c]) if 0 <= c <= 255 else 0

    # ---- producing (the loader stream) --------------------------------------------------------------------------------------

    def _device_stream(self):
        with self._lock:
            if self._stream is None:
                self.device = torch.device(self.device)
                if self.device.type != "cuda":
                    raise RuntimeError("CrossModalityDataset produces device tensors: it needs a GPU (there is no CPU fallback)")
                if self.device.index is None:
                    self.device = torch.device("cuda", torch.cuda.current_device())
                self._stream = torch.cuda.Stream(self.device)
        return self._stream

    def host_table(self, kind, in_size, out_size):
        """The cached host table: kind 'bilinear' -> (bounds, coef) or None when the pass is skipped (equal sizes, as PIL
        skips it); kind 'nearest' -> the index table, or None for equal sizes (the identity)."""
        key = (kind, int(in_size), int(out_size))
        if key not in self._host_tables:
            if in_size == out_size:
                self._host_tables[key] = None
            else:
                self._host_tables[key] = bilinear_table(in_size, out_size) if kind == 'bilinear' else nearest_table(in_size, out_size)
        return self._host_tables[key]

    def _table(self, kind, in_size, out_size):
        key = (kind, int(in_size), int(out_size))
        if key not in self._tables:
            host = self.host_table(kind, in_size, out_size)
            if host is None:
                self._tables[key] = None
            elif kind == 'bilinear':
                self._tables[key] = tuple(torch.from_numpy(t).to(self.device) for t in host)
            else:
                self._tables[key] = torch.from_numpy(host).to(self.device)
        return self._tables[key]

    @staticmethod
    def _staged(arr):
        """(array, its host tensor) of a checked file."""
        arr = np.ascontiguousarray(arr)
        return arr, torch.from_numpy(arr)

    def _load_image(self, resize_h_w, path):
        """Decode + the host-side checks of a 'data' file that will be resized to ``resize_h_w`` (None: not at all) -> uint8
        [H, W] or [H, W, 3], staged for the upload."""
        arr, colour = self._decode(path)
        if arr.dtype != np.uint8:
            raise ValueError(f"{path}: {arr.dtype} samples: only 8-bit data images are prepared on the device")
        resized = resize_h_w is not None and (int(resize_h_w[0]), int(resize_h_w[1])) != self._window(arr)
        if arr.ndim == 3 and arr.shape[2] == 4:
            # the reference keeps [:3] (:377-378); PIL resizes RGBA premultiplied, the identity only for an opaque image
            if resized and not bool((arr[:, :, 3] == 255).all()):
                raise NotImplementedError(f"{path}: an RGBA data image with transparency (PIL's premultiplied resize)")
            arr = arr[:, :, :3]
        if arr.ndim == 3 and arr.shape[2] == 1:
            arr = arr[:, :, 0]
        if arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] != 3):
            raise ValueError(f"{path}: a data image has 1, 3 or 4 channels, got shape {arr.shape}")
        if colour == 3 and resized:
            raise NotImplementedError(f"{path}: a palette data image (PIL resizes palette indices with NEAREST)")
        return self._staged(arr)

    def _load_label(self, path):
        arr, _colour = self._decode(path)
        if arr.dtype != np.uint8:
            raise ValueError(f"{path}: {arr.dtype} samples: only 8-bit labels are prepared on the device")
        if arr.ndim == 3 and not self.deliver_label_process:
            raise ValueError(f"{path}: a label must be single-channel (shape {arr.shape}); only the DELIVER labels are read "
                             "from channel 0 of a multi-channel file")
        if arr.ndim not in (2, 3):
            raise ValueError(f"{path}: a label is [H, W] or [H, W, C], got shape {arr.shape}")
        return self._staged(arr)

    def _upload(self, file):
        # pinned here, on the consuming thread: pinning on the decode threads halved the loaders' rates (tools/bench_data.py)
        if file.device is None:
            file.device = file.array()[1].pin_memory().to(self.device, non_blocking=True)
        return file.device

    def _window(self, arr):
        """The source window (rows, columns) of a decoded file: DSEC's 640 x 480 frames lose rows 440 .. 479 (:360-361)."""
        h, w = arr.shape[:2]
        if self.train_or_test == 'train' and 'DSEC_RGB' in self.json_path and (w, h) == (640, 480):
            return 440, 640
        return h, w

    def _geometry(self, arr, resize_h_w, crop_h_w, crop):
        """(in_h, in_w, rh, rw, y0, x0, ch, cw, flip) of one launch; ``crop`` None = the whole (resized) image."""
        in_h, in_w = self._window(arr)
        if crop is not None:
            rh, rw = int(resize_h_w[0]), int(resize_h_w[1])
            return in_h, in_w, rh, rw, crop.y, crop.x, int(crop_h_w[0]), int(crop_h_w[1]), int(crop.flip)
        rh, rw = (in_h, in_w) if resize_h_w is None else (int(resize_h_w[0]), int(resize_h_w[1]))
        return in_h, in_w, rh, rw, 0, 0, rh, rw, 0

    def _image(self, file, resize_h_w, crop_h_w, crop):
        from . import _lib_data
        arr, _host = file.array()
        in_h, in_w, rh, rw, y0, x0, ch, cw, flip = self._geometry(arr, resize_h_w, crop_h_w, crop)
        C = 1 if arr.ndim == 2 else 3
        src = self._upload(file)
        hb = self._table('bilinear', in_w, rw)
        vb = self._table('bilinear', in_h, rh)
        out = torch.empty((3, ch, cw), dtype=torch.float32, device=self.device)
        _lib_data.check(_lib_data.lib.mdata_prep_image_u8(
            src.data_ptr(), C, src.shape[1] * C, in_h, in_w,
            hb[0].data_ptr() if hb else None, hb[1].data_ptr() if hb else None, hb[1].shape[1] if hb else 0,
            vb[0].data_ptr() if vb else None, vb[1].data_ptr() if vb else None, vb[1].shape[1] if vb else 0,
            rh, rw, y0, x0, ch, cw, flip, out.data_ptr(), cw, ch * cw,
            torch.cuda.current_stream(self.device).cuda_stream), "mdata_prep_image_u8")
        return out

    def _label(self, file, resize_h_w, crop_h_w, crop, hist=None):
        from . import _lib_data
        arr, _host = file.array()
        px = 1 if arr.ndim == 2 else arr.shape[2]
        in_h, in_w, rh, rw, y0, x0, ch, cw, flip = self._geometry(arr, resize_h_w, crop_h_w, crop)
        src = self._upload(file)
        if self._lut1 is not None and self._dev_lut1 is None:
            self._dev_lut1 = torch.from_numpy(self._lut1).to(self.device)
        if self._lut2 is not None and self._dev_lut2 is None:
            self._dev_lut2 = torch.from_numpy(self._lut2).to(self.device)
        yt = self._table('nearest', in_h, rh)
        xt = self._table('nearest', in_w, rw)
        out = torch.empty((1, ch, cw), dtype=torch.int64, device=self.device)
        _lib_data.check(_lib_data.lib.mdata_prep_label_u8(
            src.data_ptr(), px, src.shape[1] * px, in_h, in_w,
            yt.data_ptr() if yt is not None else None, xt.data_ptr() if xt is not None else None,
            rh, rw, y0, x0, ch, cw, flip,
            self._dev_lut1.data_ptr() if self._dev_lut1 is not None else None,
            self._dev_lut2.data_ptr() if self._dev_lut2 is not None else None,
            hist.data_ptr() if hist is not None else None, out.data_ptr(), cw,
            torch.cuda.current_stream(self.device).cuda_stream), "mdata_prep_label_u8")
        return out

    def launch(self, plan):
        """Uploads the plan's files and launches its kernels on the dataset's stream; returns what ``hand_over`` takes.  The
        loaders call it ahead of the consumer, so that a sample is usually finished when it is handed over."""
        stream = self._device_stream()
        with torch.cuda.stream(stream):
            if plan.mode == 'train':
                rgb = self._image(plan.files["source_rgb"], self.source_resize_h_w, self.source_crop_size_h_w, plan.source)
                label = plan.source_label
                if label is None:
                    label = self._label(plan.files["source_label"], self.source_resize_h_w, self.source_crop_size_h_w,
                                        plan.source)
                target = self._image(plan.files["target"], self.target_resize_h_w, self.target_crop_size_h_w, plan.target)
                out = {'source_rgb': rgb, 'source_label': label, 'target_second_modality': target,
                       'width': self.target_crop_size_h_w[1], 'height': self.target_crop_size_h_w[0]}
                tensors = (rgb, label, target)
            else:
                label_rel = self.json['target_data']['label'][plan.target_idx]
                target = self._image(plan.files["target"], self.test_resize_h_w, None, None)
                out = {'target_second_modality': target, 'file_name': os.path.join(self.target_root_path, label_rel),
                       'width': target.shape[-2], 'height': target.shape[-1]}         # swapped, as in the reference (:498-499)
                tensors = (target,)
                if self.test_resize_h_w is not None:
                    out['target_label'] = self._label(plan.files["target_label"], self.test_resize_h_w, None, None)
                    tensors += (out['target_label'],)
                elif self.label_convert is not None:
                    raise KeyError('target_label')          # the reference converts a label it never loaded (:504-505)
                out['pred_save_name'] = self._pred_save_name(label_rel)
            done = torch.cuda.Event()
            done.record(stream)
        plan.files.clear()
        return out, tensors, done

    def hand_over(self, launched):
        """The sample of ``launch``, handed to the caller's current stream on the device: that stream waits for the sample's
        event and the tensors are registered with it (``record_stream``).  No host sync.  A consumer that reads a tensor on yet
        another stream registers that use itself, as with any tensor made elsewhere: the runners do for the image they copy,
        ``SemSegEvaluator.process`` does for the label it reads on a slot's stream."""
        out, tensors, done = launched
        consumer = torch.cuda.current_stream(self.device)
        if consumer != self._stream:
            consumer.wait_event(done)
            for t in tensors:
                t.record_stream(consumer)
        return out

    def produce(self, plan):
        return self.hand_over(self.launch(plan))

    def _pred_save_name(self, label_rel):
        words = label_rel.split('/')
        p = self.json_path
        if 'Cityscapes_RGB_to_DELIVER_Depth' in p or 'GTA5_RGB_to_DELIVER_Depth' in p:
            return '{}_{}_{}_{}'.format(words[-4], words[-3], words[-2], words[-1])
        if 'Cityscapes_RGB_to_DSEC_Event' in p or 'Cityscapes_RGB_to_DSEC_19_Event' in p:
            return '{}_{}'.format(words[-3], words[-1])
        if 'Cityscapes_RGB_to_VKITTI2_Depth' in p or 'GTA5_RGB_to_Cityscapes_RGB' in p or 'Cityscapes_RGB_to_FMB_Infrared' in p:
            return words[-1]
        raise NotImplementedError('pred_save_name in {}'.format(p))

    def __getitem__(self, idx):
        return self.produce(self.plan(idx))


# ---- loaders ---------------------------------------------------------------------------------------------------------------

def _pool_size(num_workers):
    return max(1, min(int(num_workers), MAX_WORKERS))


class TrainLoader:
    """Infinite iterator of ``list[dict]`` (detectron2's ``build_detection_train_loader`` with ``TrainingSampler`` and the
    trivial collator): indices are a seeded ``torch.randperm`` stream over ``len(dataset)``, reshuffled every pass and strided
    by rank.  Files are decoded on ``num_workers`` threads; draws and launches stay on the consuming thread.

    ``prefetch`` batches are planned -- drawn -- ahead of the one returned, so their files decode while the trainer runs;
    half of them are also uploaded and launched ahead on the dataset's stream.
    With ``prefetch=0`` nothing is drawn ahead: the ``random`` / ``np.random`` states ``MadmTrainer.state_dict()`` saves,
    together with this loader's ``state_dict()`` (the sampler's position), resume the exact sample stream.  With
    ``prefetch > 0`` a checkpoint's generator states are that many batches ahead of the batch the trainer last consumed."""

    def __init__(self, dataset, local_batch_size, num_workers=4, seed=0, prefetch=2, rank=0, world_size=1):
        if local_batch_size < 1 or prefetch < 0 or not 0 <= rank < world_size:
            raise ValueError(f"TrainLoader: bad local_batch_size={local_batch_size} prefetch={prefetch} rank={rank}/{world_size}")
        self.dataset, self.batch_size, self.prefetch = dataset, int(local_batch_size), int(prefetch)
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self._pool = ThreadPoolExecutor(max_workers=_pool_size(num_workers), thread_name_prefix="madm-data")
        self._planned, self._launched = deque(), deque()
        self._drawn = 0             # indices taken from the sampler by this rank
        self._indices = self._sampler(0)

    def _sampler(self, skip):
        """This rank's share of the infinite index stream, ``skip`` of its entries already consumed."""
        size = len(self.dataset)
        g = torch.Generator()
        g.manual_seed(self.seed)
        pos = 0                     # position in the global stream
        first = self.rank + skip * self.world_size
        while True:
            perm = torch.randperm(size, generator=g).tolist()
            if pos + size > first:
                for i in range(max(first - pos, 0), size):
                    if (pos + i - self.rank) % self.world_size == 0:
                        yield perm[i]
            pos += size

    def _plan_batch(self):
        batch = []
        for _ in range(self.batch_size):
            idx = next(self._indices)
            self._drawn += 1
            batch.append(self.dataset.plan(idx, submit=self._pool.submit))
        return batch

    def __iter__(self):
        return self

    def __next__(self):
        while len(self._planned) + len(self._launched) < self.prefetch + 1:
            self._planned.append(self._plan_batch())
        while self._planned and len(self._launched) < self.prefetch // 2 + 1:      # decoded ahead by all, launched by half
            self._launched.append([self.dataset.launch(p) for p in self._planned.popleft()])
        return [self.dataset.hand_over(x) for x in self._launched.popleft()]

    def state_dict(self):
        """The sampler's position: samples handed out so far (planned-ahead batches are not counted: they are drawn again)."""
        return {"seed": self.seed, "rank": self.rank, "world_size": self.world_size,
                "consumed": self._drawn - self.batch_size * (len(self._planned) + len(self._launched))}

    def load_state_dict(self, sd):
        if (sd["seed"], sd["rank"], sd["world_size"]) != (self.seed, self.rank, self.world_size):
            raise ValueError(f"TrainLoader: the saved sampler {sd} is not this loader's (seed {self.seed}, rank {self.rank} of "
                             f"{self.world_size})")
        self._planned.clear()
        self._launched.clear()
        self._drawn = int(sd["consumed"])
        self._indices = self._sampler(self._drawn)

    def close(self):
        self._planned.clear()
        self._launched.clear()
        self._pool.shutdown(wait=True, cancel_futures=True)


class TestLoader:
    """Batch size 1 over this rank's contiguous shard (detectron2's ``InferenceSampler``); re-iterable.  ``prefetch`` samples
    are planned ahead so that their files decode while the consumer works; half of them are also launched ahead."""
    __test__ = False        # not a test class, whatever its name says to a collector

    def __init__(self, dataset, num_workers=4, prefetch=4, rank=0, world_size=1):
        if prefetch < 0 or not 0 <= rank < world_size:
            raise ValueError(f"TestLoader: bad prefetch={prefetch} rank={rank}/{world_size}")
        self.dataset, self.prefetch = dataset, int(prefetch)
        total = len(dataset)
        shard, left = divmod(total, world_size)
        sizes = [shard + int(r < left) for r in range(world_size)]
        begin = sum(sizes[:rank])
        self.indices = range(begin, min(begin + sizes[rank], total))
        self._pool = ThreadPoolExecutor(max_workers=_pool_size(num_workers), thread_name_prefix="madm-data")

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        planned, launched = deque(), deque()
        it = iter(self.indices)
        while True:
            while len(planned) + len(launched) < self.prefetch + 1:
                idx = next(it, None)
                if idx is None:
                    break
                planned.append(self.dataset.plan(idx, submit=self._pool.submit))
            while planned and len(launched) < self.prefetch // 2 + 1:               # decoded ahead by all, launched by half
                launched.append(self.dataset.launch(planned.popleft()))
            if not launched:
                return
            yield [self.dataset.hand_over(launched.popleft())]

    def close(self):
        self._pool.shutdown(wait=True, cancel_futures=True)


def build_train_loader(dataset, total_batch_size=None, local_batch_size=None, num_workers=4, seed=0, prefetch=2, rank=0,
                       world_size=1):
    """Exactly one of ``total_batch_size`` (divided by ``world_size``) and ``local_batch_size``."""
    if (total_batch_size is None) == (local_batch_size is None):
        raise ValueError("build_train_loader: give exactly one of total_batch_size and local_batch_size")
    if local_batch_size is None:
        if total_batch_size <= 0 or total_batch_size % world_size:
            raise ValueError(f"build_train_loader: total_batch_size {total_batch_size} is not divisible by {world_size} ranks")
        local_batch_size = total_batch_size // world_size
    return TrainLoader(dataset, local_batch_size, num_workers=num_workers, seed=seed, prefetch=prefetch, rank=rank,
                       world_size=world_size)


def build_test_loader(dataset, num_workers=4, prefetch=4, rank=0, world_size=1):
    return TestLoader(dataset, num_workers=num_workers, prefetch=prefetch, rank=rank, world_size=world_size)
