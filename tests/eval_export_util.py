"""Shared by the evaluator-export tests: the numpy restatement of the pack buffer's layout (include/madm_hip.h,
madm_eval_export_pack), a PNG reader for what the exporter may emit, and the PIL fixture."""
import os
import struct
import zlib

import numpy as np

DELIVER_PALETTE = [70, 130, 180, 70, 70, 70, 190, 153, 153, 220, 20, 60, 153, 153, 153, 128, 64, 128, 244, 35, 232,
                   107, 142, 35, 0, 0, 142, 102, 102, 156, 250, 170, 30]
DIRS = ("image", "pred", "pred_color", "gt")


def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_export_pil.npz"))


def planes_ref(image, pred, gt, palette, num_classes, ignore_label):
    """What the reference's four statements (d2_evaluator.py:169-183) put into the files: np.uint8(image) as [H, W, 3],
    pred as uint16, palette[pred], palette[gt'] with the palette zero-padded to 256 entries."""
    image, pred, gt = np.asarray(image), np.asarray(pred), np.asarray(gt)
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal.reshape(-1)[:len(palette)] = np.asarray(palette, dtype=np.uint8)
    img = image if image.dtype == np.uint8 else np.trunc(image).astype(np.uint8)      # values in [0, 255]: truncation
    gtp = np.where(gt == ignore_label, num_classes, gt)
    return [np.ascontiguousarray(np.transpose(img, (1, 2, 0))), pred.astype(np.uint16),
            pal[pred.astype(np.uint8)], pal[gtp.astype(np.uint8)]]


def pack_ref(image, pred, gt, palette, num_classes, ignore_label):
    """The pack buffer: per plane H rows of [filter byte 0 | samples], 16-bit samples big-endian; image, pred,
    pred_color, gt_color in this order; H * (4 + 11 W) bytes."""
    H, W = np.asarray(pred).shape
    parts = []
    for a in planes_ref(image, pred, gt, palette, num_classes, ignore_label):
        body = a.astype(">u2").view(np.uint8).reshape(H, 2 * W) if a.dtype == np.uint16 else a.reshape(H, 3 * W)
        parts.append(np.concatenate([np.zeros((H, 1), dtype=np.uint8), body], axis=1).reshape(-1))
    out = np.concatenate(parts)
    assert out.size == H * (4 + 11 * W)
    return out


def decode_png(data):
    """(array, (bit depth, colour type)) of an RGB8 ([H, W, 3] u8) or 16-bit grayscale ([H, W] u16) PNG with CRC-checked
    chunks, no interlace and filter 0 on every row."""
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
    assert (comp, filt, lace) == (0, 0, 0) and (depth, colour) in ((8, 2), (16, 0))
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    bpp = 3 if colour == 2 else 2
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + bpp * W)
    assert not rows[:, 0].any(), "every row uses filter 0"
    body = np.ascontiguousarray(rows[:, 1:])
    if colour == 2:
        return body.reshape(H, W, 3), (depth, colour)
    return body.view(">u2").astype(np.uint16).reshape(H, W), (depth, colour)


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())
