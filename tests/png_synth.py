"""A small PNG writer for the decoder tests: any supported bit depth and colour type, a chosen filter
type per row, the IDAT stream split into several chunks with ancillary chunks in between, and the
damage the parser has to decline (interlace flag, sub-byte depths, a filter byte 5)."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# every format the device route takes: (bit depth, colour type) -> bytes per pixel 1, 3, 1, 2, 4, 2, 6, 4, 8
FORMATS = ((8, 0), (8, 2), (8, 3), (8, 4), (8, 6), (16, 0), (16, 2), (16, 4), (16, 6))


def bpp_of(depth, ctype):
    return CHANNELS[ctype] * depth // 8


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def filter_rows(rows, bpp, filters):
    """rows: [H, W * bpp] uint8 reconstructed bytes -> the raw stream (bytes): per row its filter byte
    and the filtered bytes.  A filter byte above 4 stores the row unfiltered."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    h, stride = rows.shape
    cur = rows.astype(np.int32)
    a = np.zeros_like(cur)
    a[:, bpp:] = cur[:, :-bpp] if stride > bpp else 0
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, bpp:] = cur[:-1, :-bpp] if stride > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    preds = (np.zeros_like(cur), a, b, (a + b) >> 1, paeth)
    raw = np.empty((h, 1 + stride), np.uint8)
    for y, f in enumerate(filters):
        raw[y, 0] = f
        raw[y, 1:] = (cur[y] - (preds[f][y] if f <= 4 else 0)) & 255
    return raw.tobytes()


def samples(rng, h, w, depth, ctype, palette_len=256, smooth=True):
    """[H, W * bpp] uint8 sample bytes.  `smooth` makes neighbours close (so that Paeth and Average
    meet all their branches and carries), every fourth row is noise."""
    bpp = bpp_of(depth, ctype)
    if ctype == 3:
        return rng.integers(0, palette_len, (h, w)).astype(np.uint8)
    data = rng.integers(0, 256, (h, w * bpp)).astype(np.int32)
    if smooth:
        walk = np.cumsum(rng.integers(-3, 4, (h, w * bpp)), axis=1) + rng.integers(0, 256, (h, 1))
        data = np.where((np.arange(h) % 4 == 3)[:, None], data, walk)
    return (data & 255).astype(np.uint8)


def write_png(rows, w, depth, ctype, filters, palette=None, idat_chunks=1, ancillary=False,
              interlace=0, level=6):
    """The file around the given sample bytes ([H, W * bpp] uint8; for a sub-byte depth whatever the
    caller packed).  palette: [k, 3] uint8 for colour type 3."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    h = rows.shape[0]
    bpp = max(1, CHANNELS.get(ctype, 1) * depth // 8)
    stream = zlib.compress(filter_rows(rows, bpp, filters), level)
    out = [SIG, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))]
    if ancillary:
        out.append(chunk(b"gAMA", struct.pack(">I", 45455)))
        out.append(chunk(b"tEXt", b"Comment\x00made by the test"))
    if palette is not None:
        out.append(chunk(b"PLTE", np.ascontiguousarray(palette, dtype=np.uint8).tobytes()))
    cuts = [len(stream) * i // idat_chunks for i in range(idat_chunks + 1)]
    for i in range(idat_chunks):
        out.append(chunk(b"IDAT", stream[cuts[i]:cuts[i + 1]]))
    if ancillary:
        out.append(chunk(b"tIME", struct.pack(">HBBBBB", 2024, 1, 2, 3, 4, 5)))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def idat_of(data):
    """The joined IDAT bodies of a PNG file."""
    pos, parts = 8, []
    while pos + 8 <= len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        if data[pos + 4:pos + 8] == b"IDAT":
            parts.append(data[pos + 8:pos + 8 + length])
        pos += 12 + length
    return b"".join(parts)


def filters_for(mode, h, rng):
    """mode 0..4: that filter type on every row; "random": a seeded random type per row."""
    if mode == "random":
        return [int(v) for v in rng.integers(0, 5, h)]
    return [int(mode)] * h
