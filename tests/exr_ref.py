"""A small OpenEXR 2.x scanline writer for the tests, restated in numpy from the published file layout (not the product's
reader, and not pinned against libOpenEXR, which is not available here).

File: magic 76 2f 31 01, int32 version (2 | flags), the header (attributes `name\\0 type\\0 int32 size value`, ended by a
zero byte), one uint64 file offset per chunk in increasing-y order, then the chunks, each int32 y, int32 size, data.  A chunk
holds 1 scanline (NONE, RLE, ZIPS) or 16 (ZIP); a scanline holds each channel's `width` samples, channels sorted by name.
RLE and ZIP(S) first interleave the chunk's bytes (even bytes, then odd) and delta-code them (d[i] = t[i] - t[i-1] + 128
mod 256); a chunk that does not shrink is stored raw."""
import struct
import zlib

import numpy as np

UINT, HALF, FLOAT = 0, 1, 2
NONE, RLE, ZIPS, ZIP = 0, 1, 2, 3
INC, DEC = 0, 1
LINES = {NONE: 1, RLE: 1, ZIPS: 1, ZIP: 16}
_DTYPE = {UINT: "<u4", HALF: "<f2", FLOAT: "<f4"}


def predict(raw):
    """interleave + delta predictor of RLE / ZIP(S) (the encoder side)"""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    t = np.concatenate([a[0::2], a[1::2]])
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + np.uint8(128)                  # uint8 arithmetic wraps mod 256
    return d.tobytes()


def unpredict(coded):
    """the decoder side: t = prefix sum of (d - 128) mod 256 with t[0] = d[0]; out[2k] = t[k], out[2k+1] = t[(n+1)/2 + k]"""
    d = np.frombuffer(bytes(coded), dtype=np.uint8).astype(np.int64)
    e = d - 128
    e[:1] = d[:1]
    t = (np.cumsum(e) & 0xFF).astype(np.uint8)
    h = (len(t) + 1) // 2
    out = np.empty_like(t)
    out[0::2], out[1::2] = t[:h], t[h:]
    return out.tobytes()


def rle_compress(b):
    """OpenEXR RLE: a run of 3..128 equal bytes -> (count - 1, byte); up to 127 other bytes -> (-count as int8, bytes)"""
    b = bytes(b)
    out, i, n = bytearray(), 0, len(b)
    while i < n:
        r = 1
        while i + r < n and r < 128 and b[i + r] == b[i]:
            r += 1
        if r >= 3:
            out += bytes([r - 1, b[i]])
            i += r
            continue
        j = i
        while j < n and j - i < 127 and not (j + 2 < n and b[j] == b[j + 1] == b[j + 2]):
            j += 1
        out += bytes([(256 - (j - i)) & 0xFF]) + b[i:j]
        i = j
    return bytes(out)


def rle_decompress(b):
    out, i = bytearray(), 0
    while i < len(b):
        c = b[i] - 256 if b[i] > 127 else b[i]
        if c < 0:
            out += b[i + 1:i + 1 - c]
            i += 1 - c
        else:
            out += bytes([b[i + 1]]) * (c + 1)
            i += 2
    return bytes(out)


def _attr(name, atype, value):
    return name + b"\0" + atype + b"\0" + struct.pack("<i", len(value)) + value


def chlist(channels, sampling=None):
    """channels: [(name bytes, pixel type)]; sampling: {name: (xs, ys)}"""
    body = b""
    for name, t in channels:
        xs, ys = (sampling or {}).get(name, (1, 1))
        body += name + b"\0" + struct.pack("<iB3xii", t, 0, xs, ys)
    return body + b"\0"


def write_exr(path, channels, compression=ZIP, line_order=INC, origin=(0, 0), chunk_hook=None, sampling=None, version_flags=0,
              list_order=None):
    """channels: {name: (array [h, w], pixel type)}.  Returns {"row_bytes", "chunks": the scanline bytes of each chunk in
    increasing-y order, "coded": whether each chunk was stored compressed}.  chunk_hook(c, stored) may replace a chunk's stored
    bytes (the size field follows the replacement); list_order writes the channel list in another order than sorted."""
    names = sorted(channels)
    h, w = next(iter(channels.values()))[0].shape
    x0, y0 = origin
    types = [(n.encode(), channels[n][1]) for n in (list_order or names)]
    header = (_attr(b"channels", b"chlist", chlist(types, sampling))
              + _attr(b"compression", b"compression", bytes([compression]))
              + _attr(b"dataWindow", b"box2i", struct.pack("<iiii", x0, y0, x0 + w - 1, y0 + h - 1))
              + _attr(b"displayWindow", b"box2i", struct.pack("<iiii", x0, y0, x0 + w - 1, y0 + h - 1))
              + _attr(b"lineOrder", b"lineOrder", bytes([line_order]))
              + _attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
              + _attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
              + _attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")
    lines = LINES.get(compression, 16)
    planes = {n: np.ascontiguousarray(channels[n][0]).astype(_DTYPE[channels[n][1]]) for n in names}
    rows = [b"".join(planes[n][y].tobytes() for n in names) for y in range(h)]
    chunks, stored, coded = [], [], []
    for c in range(-(-h // lines)):
        raw = b"".join(rows[c * lines:(c + 1) * lines])
        if compression == RLE:
            z = rle_compress(predict(raw))
        elif compression in (ZIP, ZIPS):
            z = zlib.compress(predict(raw))
        else:
            z = raw
        use = z if len(z) < len(raw) else raw
        chunks.append(raw)
        coded.append(use is z and compression != NONE)
        stored.append(chunk_hook(c, use) if chunk_hook else use)
    n = len(chunks)
    head = struct.pack("<4sI", b"\x76\x2f\x31\x01", 2 | version_flags) + header
    table_at = len(head)
    pos = table_at + 8 * n
    offsets = [0] * n
    body = b""
    for c in (range(n) if line_order == INC else reversed(range(n))):
        offsets[c] = pos + len(body)
        body += struct.pack("<ii", y0 + c * lines, len(stored[c])) + stored[c]
    with open(path, "wb") as f:
        f.write(head + struct.pack("<%dQ" % n, *offsets) + body)
    return {"row_bytes": len(rows[0]), "chunks": chunks, "coded": coded, "table_at": table_at, "offsets": offsets}


def half_values(x):
    """what a HALF channel holds for float data x: numpy's round to nearest even, back to float32"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)
