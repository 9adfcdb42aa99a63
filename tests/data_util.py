"""Test plumbing of the dataset pipeline (tests/test_data_host.py, tests/test_data_gpu.py), pure numpy:

* the restatement of PIL's two 8-bit resizes from the recipe of Pillow's Resample.c / Geometry.c, written with plain Python
  loops for the tables, independent of madm_amd/data.py's;
* the restatement of one 'data' / 'label' launch on top of them (window, resize, crop, flip, repeat, tables, histogram);
* a PNG writer that applies the five scanline filters forward;
* a maker of a tiny dataset tree + json whose name contains ``Cityscapes_RGB_to_DELIVER_Depth``."""
import json
import math
import os
import struct
import zlib

import numpy as np

PRECISION_BITS = 22

# (input H x W, output H x W, source window rows or None): the resize cases of the host and the GPU tests
RESIZE_CASES = [
    ((37, 53), (24, 40), None),       # non-integer downscale
    ((24, 40), (37, 53), None),       # upscale
    ((40, 80), (20, 40), None),       # exact 2x
    ((33, 33), (33, 20), None),       # one pass skipped
    ((480, 640), (64, 128), 440),     # source window: rows 0 .. 439 (scale 6.875 / 5)
]


# ---- the recipe ------------------------------------------------------------------------------------------------------------

def bilinear_coeffs(in_size, out_size):
    """(bounds [(xmin, n)], coef [[int]], ksize) of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs                   # Pillow multiplies by the reciprocal of the filter scale
    bounds, coef = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        ws, ww = [], 0.0
        for x in range(xmax - xmin):
            w = max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss))
            ws.append(w)
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        k = [int(0.5 + w * (1 << PRECISION_BITS)) for w in ws]
        bounds.append((xmin, xmax - xmin))
        coef.append(k + [0] * (ksize - len(k)))
    return bounds, coef, ksize


def nearest_index(in_size, out_size):
    a = in_size / out_size
    xo = a * 0.5
    tab = []
    for _ in range(out_size):
        tab.append(int(xo))
        xo += a                     # the accumulated sum, not x * a
    return tab


def _pass(img, out_size, axis):
    """One bilinear pass of a uint8 [H, W, C] array along ``axis`` (0 = vertical, 1 = horizontal)."""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img                  # PIL skips a pass whose sizes are equal
    bounds, coef, _k = bilinear_coeffs(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for i, ((lo, n), k) in enumerate(zip(bounds, coef)):
        acc = np.tensordot(np.asarray(k[:n], dtype=np.int64), src[lo:lo + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(img, out_h, out_w):
    """PIL ``resize((out_w, out_h), BILINEAR)`` of a uint8 [H, W] or [H, W, C] array: horizontal pass, then vertical."""
    a = img[:, :, None] if img.ndim == 2 else img
    a = _pass(_pass(a, out_w, 1), out_h, 0)
    return np.ascontiguousarray(a[:, :, 0] if img.ndim == 2 else a)


def resize_nearest(img, out_h, out_w):
    ys = np.asarray(nearest_index(img.shape[0], out_h))
    xs = np.asarray(nearest_index(img.shape[1], out_w))
    return np.ascontiguousarray(img[ys][:, xs])


def deliver_lut():
    return np.asarray([255 if v in (0, 255) else v - 1 for v in range(256)], dtype=np.uint8)


def convert_lut(pairs):
    lut = list(range(256))
    for old, new in pairs:
        if 0 <= old <= 255:
            lut[old] = new
    return np.asarray(lut, dtype=np.uint8)


def prep_image_ref(arr, resize_h_w, crop=None, window_rows=None):
    """f32 [3, ch, cw]: the 'data' path.  ``crop`` = (y, x, ch, cw, flip) or None (whole image)."""
    a = arr if window_rows is None else arr[:window_rows]
    if a.ndim == 3 and a.shape[2] == 4:
        a = a[:, :, :3]
    if resize_h_w is not None:
        a = resize_bilinear(a, resize_h_w[0], resize_h_w[1])
    if crop is not None:
        y, x, ch, cw, flip = crop
        a = a[y:y + ch, x:x + cw]
        if flip:
            a = a[:, ::-1]
    a = a[None] if a.ndim == 2 else np.transpose(a, (2, 0, 1))
    if a.shape[0] == 1:
        a = np.repeat(a, 3, axis=0)
    return np.ascontiguousarray(a, dtype=np.float32)


def prep_label_ref(arr, resize_h_w, crop=None, window_rows=None, lut1=None, lut2=None):
    """(i64 [1, ch, cw], histogram int64 [256] after lut1 and before lut2): the 'label' path; channel 0 of an HWC array."""
    a = arr if window_rows is None else arr[:window_rows]
    if a.ndim == 3:
        a = a[:, :, 0]
    if resize_h_w is not None:
        a = resize_nearest(a, resize_h_w[0], resize_h_w[1])
    if crop is not None:
        y, x, ch, cw, flip = crop
        a = a[y:y + ch, x:x + cw]
        if flip:
            a = a[:, ::-1]
    if lut1 is not None:
        a = lut1[a]
    hist = np.bincount(a.reshape(-1), minlength=256)
    if lut2 is not None:
        a = lut2[a]
    return np.ascontiguousarray(a[None], dtype=np.int64), hist


# ---- PNG writing -----------------------------------------------------------------------------------------------------------

def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def filter_rows(rows, bpp, filters):
    """Forward PNG filtering of uint8 [H, row_bytes] raw rows; ``filters``: one type (0 .. 4) or one per row.  The
    predictors use the RAW bytes, so every row is independent."""
    H, n = rows.shape
    filters = [filters] * H if isinstance(filters, int) else list(filters)
    r = rows.astype(np.int32)
    left = np.zeros_like(r)
    left[:, bpp:] = r[:, :-bpp] if n > bpp else 0
    up = np.zeros_like(r)
    up[1:] = r[:-1]
    upleft = np.zeros_like(r)
    upleft[1:, bpp:] = r[:-1, :-bpp] if n > bpp else 0
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    pred = {0: np.zeros_like(r), 1: left, 2: up, 3: (left + up) >> 1, 4: paeth}
    out = np.empty((H, n + 1), dtype=np.uint8)
    for y, f in enumerate(filters):
        out[y, 0] = f
        out[y, 1:] = (r[y] - pred[f][y]) & 255 if f in pred else rows[y]
    return out


def png_bytes(arr, filters=0, colour_type=None, interlace=0, bit_depth=None, palette=None):
    """A PNG file of a uint8 [H, W] / [H, W, 3] / [H, W, 4] or uint16 [H, W] array.  ``colour_type`` 3 writes [H, W] as
    palette indices (with a PLTE chunk); the header fields can be overridden to write files the reader must refuse."""
    arr = np.asarray(arr)
    H, W = arr.shape[:2]
    if arr.dtype == np.uint16:
        raw, bpp, depth, ctype = arr.astype(">u2").view(np.uint8).reshape(H, W * 2), 2, 16, 0
    else:
        c = 1 if arr.ndim == 2 else arr.shape[2]
        raw, bpp, depth, ctype = arr.reshape(H, W * c), c, 8, {1: 0, 3: 2, 4: 6}[c]
    if colour_type is not None:
        ctype = colour_type
    if bit_depth is not None:
        depth = bit_depth
    body = filter_rows(np.ascontiguousarray(raw), bpp, filters).tobytes()
    chunks = [_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))]
    if ctype == 3:
        pal = np.asarray(palette if palette is not None else [[i, 255 - i, (7 * i) & 255] for i in range(256)], dtype=np.uint8)
        chunks.append(_chunk(b"PLTE", pal.tobytes()))
    z = zlib.compress(body, 6)      # two IDAT chunks: the stream may be split anywhere
    chunks += [_chunk(b"IDAT", z[:len(z) // 2]), _chunk(b"IDAT", z[len(z) // 2:]), _chunk(b"IEND", b"")]
    return b"\x89PNG\r\n\x1a\n" + b"".join(chunks)


def write_png(path, arr, **kw):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(png_bytes(arr, **kw))


# ---- the tiny dataset tree ------------------------------------------------------------------------------------------------

TREE = dict(source_hw=(48, 96), target_hw=(64, 64), source_resize=[24, 48], source_crop=[16, 20], target_resize=[40, 40],
            target_crop=[16, 20], test_resize=[32, 32], n_source=3, n_target=2, num_classes=6,
            label_convert=[[0, 255], [1, 0], [2, 1], [3, 2], [7, 3], [8, 255]])


def make_tree(root, seed=0, n_target=None):
    """Writes a Cityscapes -> DELIVER shaped tree under ``root``: 3 RGB source images + gray labels (ids 0 .. 8), 2 target
    'depth' images (gray, RGB alternating) + RGBA labels whose channel 0 holds the class (DELIVER's format: ids 0 .. 6 and
    255), every file with another filter mix.  Returns (json_path, source_root, target_root) -- ``target_root`` ends in a
    separator, as the reference's constructor joins it with a plain ``+``."""
    rng = np.random.RandomState(seed)
    src_root, tgt_root = os.path.join(root, "cityscapes"), os.path.join(root, "deliver") + os.sep
    js = {"source_data": {"RGB": [], "label": []}, "target_data": {"second_modality": [], "label": []}}
    sh, sw = TREE["source_hw"]
    for i in range(TREE["n_source"]):
        img = rng.randint(0, 256, size=(sh, sw, 3)).astype(np.uint8)
        img[:, : sw // 2] = (np.linspace(0, 255, sh * (sw // 2)).reshape(sh, sw // 2, 1) + 40 * i).astype(np.uint8)  # smooth half
        lab = rng.randint(0, 9, size=(sh // 4, sw // 4)).astype(np.uint8).repeat(4, 0).repeat(4, 1)
        rgb_rel, lab_rel = f"leftImg8bit/train/city/img_{i}.png", f"gtFine/train/city/img_{i}_labelIds.png"
        write_png(os.path.join(src_root, rgb_rel), img, filters=[(y + i) % 5 for y in range(sh)])
        write_png(os.path.join(src_root, lab_rel), lab, filters=i % 5)
        js["source_data"]["RGB"].append(rgb_rel)
        js["source_data"]["label"].append(lab_rel)
    th, tw = TREE["target_hw"]
    for i in range(TREE["n_target"] if n_target is None else n_target):   # more targets only append: the first files stay as they are
        depth = rng.randint(0, 256, size=(th, tw) if i % 2 == 0 else (th, tw, 3)).astype(np.uint8)
        cls = rng.randint(0, 7, size=(th // 4, tw // 4)).astype(np.uint8).repeat(4, 0).repeat(4, 1)
        cls[rng.rand(th, tw) < 0.05] = 255
        lab = np.stack([cls, rng.randint(0, 256, size=(th, tw)).astype(np.uint8), np.zeros((th, tw), np.uint8),
                        np.full((th, tw), 255, np.uint8)], axis=2)
        d_rel, l_rel = f"depth/cloud/test/MAP_{i}/{i:06d}_depth_front.png", f"semantic/cloud/test/MAP_{i}/{i:06d}_semantic_front.png"
        write_png(os.path.join(tgt_root, d_rel), depth, filters=(4 - i) % 5)
        write_png(os.path.join(tgt_root, l_rel), lab, filters=[(2 * y + i) % 5 for y in range(th)])
        js["target_data"]["second_modality"].append(d_rel)
        js["target_data"]["label"].append(l_rel)
    json_path = os.path.join(root, "Cityscapes_RGB_to_DELIVER_Depth.json")
    with open(json_path, "w") as f:
        json.dump(js, f)
    return json_path, src_root, tgt_root


def train_kwargs():
    return dict(source_resize_h_w=TREE["source_resize"], source_crop_size_h_w=TREE["source_crop"],
                target_resize_h_w=TREE["target_resize"], target_crop_size_h_w=TREE["target_crop"], train_or_test='train',
                label_convert=TREE["label_convert"])


def eval_kwargs():
    return dict(test_resize_h_w=TREE["test_resize"], train_or_test='test')


def sample_from_plan(ds, plan):
    """The restatement applied on the product's own plan: what ``ds.produce(plan)`` must hold, as numpy arrays."""
    from madm_amd import png_read
    js = ds.json
    lut1 = deliver_lut() if ds.deliver_label_process else None
    lut2 = convert_lut(ds.label_convert) if ds.label_convert is not None else None
    tgt = png_read.read_png(os.path.join(ds.target_root_path, js['target_data']['second_modality'][plan.target_idx]))
    if plan.mode == 'train':
        rgb = png_read.read_png(os.path.join(ds.source_root_path, js['source_data']['RGB'][plan.source_idx]))
        lab = png_read.read_png(os.path.join(ds.source_root_path, js['source_data']['label'][plan.source_idx]))
        sc = (plan.source.y, plan.source.x, ds.source_crop_size_h_w[0], ds.source_crop_size_h_w[1], plan.source.flip)
        tc = (plan.target.y, plan.target.x, ds.target_crop_size_h_w[0], ds.target_crop_size_h_w[1], plan.target.flip)
        return {"source_rgb": prep_image_ref(rgb, ds.source_resize_h_w, sc),
                "source_label": prep_label_ref(lab, ds.source_resize_h_w, sc, lut1=lut1, lut2=lut2)[0],
                "target_second_modality": prep_image_ref(tgt, ds.target_resize_h_w, tc)}
    out = {"target_second_modality": prep_image_ref(tgt, ds.test_resize_h_w)}
    if ds.test_resize_h_w is not None:
        lab = png_read.read_png(os.path.join(ds.target_root_path, js['target_data']['label'][plan.target_idx]))
        out["target_label"] = prep_label_ref(lab, ds.test_resize_h_w, lut1=lut1, lut2=lut2)[0]
    return out


# ---- the reference's dataset, loaded by path -------------------------------------------------------------------------------

REFERENCE_FILE = "/root/reference/data/dataset/cross_modality_dataset.py"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_samples.npz")
TRAIN_INDICES, EVAL_INDICES = (0, 1, 2, 3, 4, 5), (0, 1, 2)


def seed_of(idx):
    return 1000 + idx


def load_reference_class():
    """The reference's ``CrossModalityDataset`` class, its module loaded by path under a stub ``torchvision.transforms``
    (``Compose``, ``ToTensor`` and a ``RandomHorizontalFlip`` that mirrors a PIL image: all the module touches)."""
    import importlib.util
    import sys
    import types

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

    class ToTensor:
        pass

    class RandomHorizontalFlip:
        def __init__(self, p=0.5):
            assert p == 1

        def __call__(self, img):
            from PIL import Image
            return img.transpose(Image.FLIP_LEFT_RIGHT)

    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.Compose, tr.ToTensor, tr.RandomHorizontalFlip = Compose, ToTensor, RandomHorizontalFlip
    tv.transforms = tr
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms")}
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    try:
        spec = importlib.util.spec_from_file_location("_reference_cross_modality_dataset", REFERENCE_FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.CrossModalityDataset


TENSOR_KEYS = ("source_rgb", "source_label", "target_second_modality", "target_label")


def golden_key(mode, idx, key):
    return f"{mode}_{idx}_{key}"
