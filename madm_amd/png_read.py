"""PNG reading without an imaging library (the dataset pipeline's decoder, madm_amd/data.py).

Chunk parsing is Python (every CRC checked), inflate is ``zlib`` and the one byte loop -- undoing the scanline filters -- is
``mdata_png_unfilter`` of libmadm_data.so (host C++; ctypes releases the GIL around it, as zlib does around inflate, so decode
threads run in parallel).  Python checks every length before the call; the native function checks every filter byte.

Supported: non-interlaced, bit depth 8, colour types 0 (gray), 2 (RGB), 3 (palette: the INDICES are returned, as
``np.array`` of a PIL ``P`` image gives them) and 6 (RGBA, four channels); bit depth 16 with colour type 0 is decoded to
``uint16`` so that the caller can refuse it by name.  Everything else raises ``ValueError`` naming the file and the field."""
import struct
import zlib

import numpy as np

_MAGIC = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_MAX_PIXELS = 1 << 28       # refuse absurd headers before allocating for them


def _chunks(data, name):
    """(tag, payload) of every chunk, CRC checked, up to and including IEND."""
    pos, n = len(_MAGIC), len(data)
    while True:
        if pos + 8 > n:
            raise ValueError(f"{name}: truncated PNG: no IEND chunk (file ends at byte {n})")
        length, = struct.unpack_from(">I", data, pos)
        tag = bytes(data[pos + 4:pos + 8])
        end = pos + 8 + length
        if end + 4 > n:
            raise ValueError(f"{name}: truncated PNG: chunk {tag!r} at byte {pos} claims {length} bytes, the file has {n}")
        crc, = struct.unpack_from(">I", data, end)
        if zlib.crc32(data[pos + 4:end]) & 0xFFFFFFFF != crc:
            raise ValueError(f"{name}: bad CRC in chunk {tag!r} at byte {pos}")
        yield tag, data[pos + 8:end]
        if tag == b"IEND":
            return
        pos = end + 4


def png_header(data, name="<bytes>"):
    """(width, height, bit_depth, colour_type, interlace) from the IHDR chunk of PNG bytes (only the head is needed)."""
    if len(data) < 33 or bytes(data[:8]) != _MAGIC:
        raise ValueError(f"{name}: not a PNG file (bad signature)")
    length, = struct.unpack_from(">I", data, 8)
    if bytes(data[12:16]) != b"IHDR" or length != 13:
        raise ValueError(f"{name}: the first chunk is not a 13-byte IHDR")
    crc, = struct.unpack_from(">I", data, 29)
    if zlib.crc32(data[12:29]) & 0xFFFFFFFF != crc:
        raise ValueError(f"{name}: bad CRC in chunk b'IHDR' at byte 8")
    w, h, depth, colour, comp, filt, interlace = struct.unpack_from(">IIBBBBB", data, 16)
    if w < 1 or h < 1 or w * h > _MAX_PIXELS:
        raise ValueError(f"{name}: unsupported size: width {w}, height {h}")
    if comp != 0 or filt != 0:
        raise ValueError(f"{name}: unsupported compression method {comp} / filter method {filt}")
    return w, h, depth, colour, interlace


def png_size(path):
    """(width, height) of a PNG file, reading its first 33 bytes."""
    with open(path, "rb") as f:
        head = f.read(33)
    w, h, _d, _c, _i = png_header(head, str(path))
    return w, h


def decode_png(data, name="<bytes>", with_colour_type=False):
    """PNG bytes -> ``np.ndarray``: uint8 [H, W] (colour types 0 and 3), [H, W, 3] (type 2), [H, W, 4] (type 6), or uint16
    [H, W] (16-bit gray).  ``with_colour_type``: returns (array, colour type) -- palette indices and gray levels look alike."""
    from . import _lib_data
    data = memoryview(data).cast("B") if not isinstance(data, (bytes, bytearray)) else data
    w, h, depth, colour, interlace = png_header(data, name)
    if interlace != 0:
        raise ValueError(f"{name}: unsupported interlace method {interlace} (only non-interlaced files)")
    if colour not in _CHANNELS:
        raise ValueError(f"{name}: unsupported colour type {colour}")
    if not (depth == 8 and colour in (0, 2, 3, 6)) and not (depth == 16 and colour == 0):
        raise ValueError(f"{name}: unsupported bit depth {depth} with colour type {colour} "
                         "(8-bit gray, RGB, palette, RGBA and 16-bit gray are read)")
    idat = [bytes(p) for tag, p in _chunks(data, name) if tag == b"IDAT"]
    if not idat:
        raise ValueError(f"{name}: no IDAT chunk")
    bpp = _CHANNELS[colour] * depth // 8
    row_bytes = w * bpp
    want = h * (1 + row_bytes)
    z = zlib.decompressobj()
    try:
        raw = z.decompress(b"".join(idat), want + 1)
    except zlib.error as e:
        raise ValueError(f"{name}: corrupt IDAT stream: {e}") from None
    if len(raw) != want:
        raise ValueError(f"{name}: IDAT holds {'more than ' if len(raw) > want else ''}{len(raw)} bytes of scanlines, "
                         f"{w} x {h} at {bpp} bytes per pixel needs {want}")
    out = np.empty(h * row_bytes, dtype=np.uint8)
    src = np.frombuffer(raw, dtype=np.uint8)
    rc = _lib_data.lib.mdata_png_unfilter(src.ctypes.data, src.size, out.ctypes.data, out.size, h, row_bytes, bpp)
    if rc == _lib_data.MDATA_ERR_FORMAT:
        raise ValueError(f"{name}: {_lib_data.last_error()}")
    _lib_data.check(rc, "mdata_png_unfilter")
    if depth == 16:
        arr = out.view(">u2").astype(np.uint16).reshape(h, w)
    else:
        c = _CHANNELS[colour]
        arr = out.reshape(h, w) if c == 1 else out.reshape(h, w, c)
    return (arr, colour) if with_colour_type else arr


def read_png(path, with_colour_type=False):
    with open(path, "rb") as f:
        data = f.read()
    return decode_png(data, str(path), with_colour_type)
