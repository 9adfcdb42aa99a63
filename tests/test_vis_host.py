"""CPU tests of the periodic training picture (madm_amd/vis.py): the sheet layout against the reference's index
arithmetic (modeling/meta_arch/cmdise.py:250,261), the zlib-only PNG encoder, the writer (ordering, atomic files, sidecar,
error propagation; in line and on its thread) and the constructor checks of ``MTMADISE``."""
import ctypes
import io
import json
import math
import os
import struct
import threading
import zlib

import numpy as np
import pytest
import torch


def test_layout_matches_reference_index_arithmetic():
    from madm_amd import vis
    cols_max = 5
    for n in range(1, 14):
        for B in range(1, 4):
            rows, cols, cells = vis.layout(n, B, cols_max)
            # cmdise.py:250
            assert (rows, cols) == (B * math.ceil(n / cols_max), min(cols_max, n))
            seen = set()
            for i in range(n):
                for j in range(B):
                    vis_x, vis_y = i % cols_max, j * math.ceil(n / cols_max) + i // cols_max     # cmdise.py:261
                    assert cells[i][j] == (vis_y, vis_x)
                    assert 0 <= vis_y < rows and 0 <= vis_x < cols
                    seen.add((vis_y, vis_x))
            assert len(seen) == n * B
    with pytest.raises(ValueError):
        vis.layout(0, 1, 5)


def decode_png(data):
    """A PNG reader for what ``encode_png`` may emit (RGB8, no interlace, filter 0): (array [H, W, 3], IHDR fields)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any(), "every row uses filter 0"
    return rows[:, 1:].reshape(H, W, 3).copy()


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (48, 250), (64, 3)])
def test_encode_png_round_trips(shape):
    from madm_amd import vis
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    img = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    data = vis.encode_png(img)
    assert np.array_equal(decode_png(data), img)
    assert np.array_equal(decode_png(vis.encode_png(torch.from_numpy(img))), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        im = Image.open(io.BytesIO(data))
        assert im.size == (shape[1], shape[0]) and im.mode == "RGB"
        assert np.array_equal(np.asarray(im), img)
    for bad in (img.astype(np.int32), img[:, :, :2], img[0]):
        with pytest.raises(ValueError):
            vis.encode_png(bad)


def test_product_path_needs_no_imaging_library():
    import madm_amd.vis as v
    src = open(v.__file__).read()
    for name in ("PIL", "matplotlib", "cv2", "imageio"):
        assert f"import {name}" not in src and f"from {name}" not in src


def _sheet(seed, H=6, W=10):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8))


def _meta(n=3, B=1, H=3, W=2, cols_max=5):
    from madm_amd import vis
    tiles = [dict(data_type=k, info=f"tile{i}", data=None) for i, k in zip(range(n), ("image", "logits", "label") * 6)]
    return vis.VisWriter.describe(tiles, B, H, W, cols_max)


@pytest.mark.parametrize("async_write", [True, False], ids=["thread", "inline"])
def test_writer_order_atomic_files_and_sidecar(tmp_path, async_write):
    from madm_amd import vis
    w = vis.VisWriter(tmp_path, rank=3, async_write=async_write)
    d = tmp_path / "vis_results"
    observed = []                   # what exists under a FINAL name at the moment each file is encoded / replaced
    real_replace = os.replace

    def spy_replace(src, dst):
        # nothing under the final name yet, and the temporary file is complete before it takes the name
        assert not os.path.exists(dst)
        observed.append((os.path.basename(dst), os.path.getsize(src)))
        real_replace(src, dst)

    a, b = _sheet(1), _sheet(2)
    os.replace = spy_replace
    try:
        w.submit_canvas(250, a, _meta())
        if async_write:
            assert w._thread is not None
        w.submit_canvas(500, b, _meta())       # waits for the first one: the order is kept
        first_done = sorted(p.name for p in d.iterdir())
        w.wait()
    finally:
        os.replace = real_replace
    assert [n for n, _ in observed] == ["000250_rank3.json", "000250_rank3.png", "000500_rank3.json", "000500_rank3.png"]
    assert {"000250_rank3.json", "000250_rank3.png"} <= set(first_done)
    assert sorted(p.name for p in d.iterdir()) == ["000250_rank3.json", "000250_rank3.png", "000500_rank3.json",
                                                   "000500_rank3.png"]                 # and no temporary file is left
    for it, sheet in ((250, a), (500, b)):
        data = open(w.path(it), "rb").read()
        assert len(data) == dict(observed)[os.path.basename(w.path(it))]
        assert np.array_equal(decode_png(data), sheet.numpy())
    side = json.load(open(w.path(500, "json")))
    assert side["iteration"] == 500 and side["rank"] == 3
    assert (side["rows"], side["cols"], side["cols_max"], side["batch"], side["tile_size"]) == (1, 3, 5, 1, [3, 2])
    assert [(t["info"], t["kind"]) for t in side["tiles"]] == [("tile0", "image"), ("tile1", "logits"), ("tile2", "label")]
    assert [t["rects"] for t in side["tiles"]] == [[[0, 0, 2, 3]], [[2, 0, 2, 3]], [[4, 0, 2, 3]]]
    assert w._thread is None
    w.close()
    with pytest.raises(RuntimeError):
        w.submit_canvas(750, a, _meta())


def test_sidecar_rectangles_of_a_ragged_sheet():
    m = _meta(n=7, B=2, H=4, W=6, cols_max=5)
    assert (m["rows"], m["cols"]) == (4, 5)
    # tile 6 of image 1: column 1, row 1 * 2 + 1
    assert m["tiles"][6]["rects"] == [[6, 4, 6, 4], [6, 12, 6, 4]]
    assert m["tiles"][4]["rects"] == [[24, 0, 6, 4], [24, 8, 6, 4]]


@pytest.mark.parametrize("async_write", [True, False], ids=["thread", "inline"])
def test_writer_failure_is_reraised_by_the_next_call(tmp_path, async_write, monkeypatch):
    from madm_amd import vis

    class Boom(RuntimeError):
        pass

    calls = []

    def failing(host):
        calls.append(1)
        raise Boom("disk full")

    for nxt in ("submit", "wait", "close"):
        w = vis.VisWriter(tmp_path / nxt, async_write=async_write)
        monkeypatch.setattr(w, "_encode", failing)
        if async_write:
            w.submit_canvas(1, _sheet(1), _meta())          # the training thread is not the one that fails ...
            with pytest.raises(Boom):                       # ... the next call reports it
                {"submit": lambda: w.submit_canvas(2, _sheet(2), _meta()), "wait": w.wait, "close": w.close}[nxt]()
        else:
            with pytest.raises(Boom):
                w.submit_canvas(1, _sheet(1), _meta())
        w.wait()                                            # reported once
        d = tmp_path / nxt / "vis_results"
        assert not [p for p in d.iterdir() if p.suffix == ".png" or p.name.endswith(".tmp")] if d.exists() else True
        monkeypatch.setattr(w, "_encode", vis.encode_png)
        if nxt != "close":
            w.submit_canvas(3, _sheet(3), _meta())          # and the writer is usable again
            w.wait()
            assert os.path.exists(w.path(3))
    assert calls


def test_writer_waits_at_interpreter_exit(tmp_path):
    """A process that ends right after a submit still leaves the whole file behind."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, torch; sys.path.insert(0, %r); from madm_amd import vis\n"
            "w = vis.VisWriter(%r)\n"
            "w.submit_canvas(7, torch.full((64, 64, 3), 9, dtype=torch.uint8), dict(tiles=[]))\n" % (root, str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
    data = open(tmp_path / "vis_results" / "000007_rank0.png", "rb").read()
    assert (decode_png(data) == 9).all()


def test_compose_argument_checks_without_gpu():
    from madm_amd import vis, _lib
    lib = _lib.lib
    with pytest.raises(ValueError):
        vis.compose([], 5, [0] * 3)
    with pytest.raises(ValueError):
        vis.compose([dict(data_type="image", info="x", data=torch.zeros(1, 3, 4, 4))], 5, [0] * 3)     # CPU tensor
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    tiles = (_lib.VisTile * 17)()
    for t in tiles:
        t.kind, t.src, t.C, t.h, t.w = _lib.VIS_IMAGE, p, 3, 8, 8
    assert lib.madm_vis_compose(tiles, 1, 1, 8, 8, 5, None, p, None) == -1 and b"null" in lib.madm_last_error()
    assert lib.madm_vis_compose(tiles, 0, 1, 8, 8, 5, p, p, None) == -1 and b"tiles" in lib.madm_last_error()
    assert lib.madm_vis_compose(tiles, 17, 1, 8, 8, 5, p, p, None) == -1 and b"tiles" in lib.madm_last_error()
    assert lib.madm_vis_compose(tiles, 1, 1, 8, 8, 0, p, p, None) == -1 and b"geometry" in lib.madm_last_error()
    tiles[1].h = 4                      # only logits are resized
    assert lib.madm_vis_compose(tiles, 2, 1, 8, 8, 5, p, p, None) == -1 and b"only logits" in lib.madm_last_error()
    tiles[1].h, tiles[1].kind = 8, 7
    assert lib.madm_vis_compose(tiles, 2, 1, 8, 8, 5, p, p, None) == -1 and b"unknown kind" in lib.madm_last_error()
    tiles[1].kind, tiles[1].C = _lib.VIS_LABEL, 3
    assert lib.madm_vis_compose(tiles, 2, 1, 8, 8, 5, p, p, None) == -1 and b"channel" in lib.madm_last_error()
    tiles[1].kind, tiles[1].C, tiles[1].src = _lib.VIS_LOGITS, 0, p
    assert lib.madm_vis_compose(tiles, 2, 1, 8, 8, 5, p, p, None) == -1 and b"logits shape" in lib.madm_last_error()
    assert lib.madm_abi_version() == 6


class _Stub(torch.nn.Module):
    """Just enough of a backbone / head for ``MTMADISE.__init__`` on the CPU."""

    def __init__(self):
        super().__init__()
        self.feature_projections = torch.nn.Linear(2, 2)
        self.clip_project_others = torch.nn.Linear(2, 2)
        self.ldm_extractor = self
        self.unet = torch.nn.Linear(2, 2)

    @property
    def feature_extractor(self):
        return self


def _model(**kw):
    from madm_amd.mtmadise import MTMADISE
    return MTMADISE(_Stub(), torch.nn.Linear(2, 2), None, target_modality="Depth", train_palette=[1, 2, 3] * 11, **kw)


def test_constructor_checks_and_off_means_no_writer(tmp_path):
    before = threading.active_count()
    for off in (dict(), dict(vis_period=None), dict(vis_period=0), dict(vis_period=None, output_dir=str(tmp_path))):
        m = _model(**off)
        assert m.vis_writer is None and m.last_vis is None and not m.vis_period
    with pytest.raises(ValueError, match="output_dir"):
        _model(vis_period=250)
    with pytest.raises(ValueError):
        _model(vis_period=-5, output_dir=str(tmp_path))
    with pytest.raises(ValueError):
        _model(vis_period=250, output_dir=str(tmp_path), vis_max_cols=0)
    with pytest.raises(ValueError, match="tiles"):       # 8 + 2 (mic) + 2 ('st') + 3 (reg_uncertain) + 2 (extra pass) = 17
        _model(vis_period=250, output_dir=str(tmp_path), mic=True, vae_decoder_loss='st', reg_uncertain=True,
               rev_noise_sup=True)
    m = _model(vis_period=250, output_dir=str(tmp_path), vis_async=False, vis_denorm=(1, 0), vis_max_cols=4)
    assert m.vis_period == 250 and m.vis_writer is not None and not m.vis_writer.async_write
    assert m.vis_denorm == (1.0, 0.0) and m.vis_max_cols == 4
    assert m.vis_writer.path(250).endswith(os.path.join("vis_results", "000250_rank0.png"))
    m = _model(vis_period=250, output_dir=str(tmp_path))
    assert m.vis_denorm == (0.5, 0.5) and m.vis_max_cols == 5
    assert _model(vis_period=250, output_dir=str(tmp_path), vis_async=True).vis_writer.async_write
    assert m.vis_writer._thread is None and m.vis_writer.canvas is None        # nothing allocated or started before a dump
    assert threading.active_count() == before
    assert not (tmp_path / "vis_results").exists()
