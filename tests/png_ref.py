"""An independent NumPy restatement of the PNG writer's rules (csrc/png.h): the five filters and the adaptive choice, the segment
cuts and the chunk layout, with zlib.crc32 and zlib.adler32 as judges.  It writes no files of its own: it says what the filtered
stream must be and takes a file apart.  Also the case list that the host and the device tests share."""
import io
import struct
import zlib

import numpy as np

SEGMENT = 65520
FILTERS = ("none", "sub", "up", "average", "paeth")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


def as_hwc(a):
    a = np.asarray(a)
    return a[:, :, None] if a.ndim == 2 else a


def candidates(a):
    """uint8 [5, H, W * C]: the image filtered with each of the five types (row 0 sees zeros above, bytes left of a row are zero)"""
    a = as_hwc(a)
    h, w, c = a.shape
    x = a.reshape(h, w * c).astype(np.int32)
    left = np.zeros_like(x)
    left[:, c:] = x[:, :-c] if w > 1 else 0
    up = np.zeros_like(x)
    up[1:] = x[:-1]
    upleft = np.zeros_like(x)
    upleft[1:, c:] = x[:-1, :-c] if w > 1 else 0
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    preds = (np.zeros_like(x), left, up, (left + up) // 2, paeth)
    return np.stack([((x - q) & 255).astype(np.uint8) for q in preds])


def row_types(a, filter="adaptive"):
    """the filter type of every row"""
    cand = candidates(a)
    if filter != "adaptive":
        return np.full(cand.shape[1], FILTERS.index(filter))
    cost = np.abs(cand.view(np.int8).astype(np.int64)).sum(axis=2)          # [5, H]
    return np.argmin(cost, axis=0)                                          # the first minimum: the lowest type on a tie


def filtered_stream(a, filter="adaptive"):
    cand = candidates(a)
    types = row_types(a, filter)
    rows = cand[types, np.arange(cand.shape[1])]
    return np.concatenate([types.astype(np.uint8)[:, None], rows], axis=1).tobytes()


def chunks(data):
    """[(tag, payload)] of a file; the signature, every length and every CRC are checked on the way"""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        tag, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(payload) == n
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(tag + payload), tag
        out.append((tag, payload))
        at += 12 + n
    assert at == len(data)
    return out


def bound(stream):
    segs = -(-stream // SEGMENT)
    return 8 + 25 + 12 + 6 + stream + segs * (5 + 12)


def check_file(data, a, filter="adaptive"):
    """everything the issue asks of one file: PIL's pixels, the chunks, IHDR, the IDAT count, the zlib stream, the bound.  Returns
    the IDAT payloads."""
    from PIL import Image
    a = as_hwc(a)
    h, w, c = a.shape
    parts = chunks(data)
    tags = [t for t, _ in parts]
    stream = filtered_stream(a, filter)
    n_idat = -(-len(stream) // SEGMENT)
    assert tags == [b"IHDR"] + [b"IDAT"] * n_idat + [b"IEND"]
    assert parts[0][1] == struct.pack(">IIBBBBB", w, h, 8, COLOUR_TYPE[c], 0, 0, 0)
    assert parts[-1][1] == b""
    idat = [p for t, p in parts if t == b"IDAT"]
    z = b"".join(idat)
    assert z[:2] == b"\x78\x01"
    assert zlib.decompress(z) == stream
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(stream)
    assert len(data) <= bound(len(stream))
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[c] and im.size == (w, h)
    assert np.array_equal(np.asarray(im).reshape(h, w, c), a)
    return idat


def segment_kinds(idat):
    """'stored' or 'coded' per IDAT, from the block type bits of its first block (every segment starts on a byte)"""
    kinds = []
    for k, p in enumerate(idat):
        first = p[2] if k == 0 else p[0]
        kinds.append("stored" if (first >> 1) & 3 == 0 else "coded")
    return kinds


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _ramp(h, w, c, dx, dy, step=1):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(dx * x + dy * y) * step + 7 * k for k in range(c)], axis=-1).astype(np.uint8)


def noise(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def paeth_tie_cases():
    """2 x 2 grey images whose last byte meets one Paeth tie each: (a, b, c) = (left, up, upleft) of that byte"""
    out = {}
    for name, (a, b, c) in {"pa=pb": (10, 10, 4), "pb=pc": (14, 2, 10), "pa=pc": (4, 13, 10)}.items():
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        assert {"pa=pb": pa == pb < pc, "pb=pc": pb == pc < pa, "pa=pc": pa == pc < pb}[name]      # the tie decides
        out[name] = np.array([[c, b], [a, 99]], dtype=np.uint8)
    return out


def filter_cases():
    """{name: image}: what the issue lists for the filtered stream"""
    cases = {}
    for c in (1, 3, 4):
        cases["zero_c%d" % c] = np.zeros((4, 6, c), np.uint8)
        cases["hramp_c%d" % c] = _ramp(5, 40, c, 1, 0, 3)
        cases["vramp_c%d" % c] = _ramp(9, 7, c, 0, 1, 5)
        cases["diag_c%d" % c] = _ramp(8, 11, c, 1, 1, 2)
        cases["noise_c%d" % c] = noise(7, 13, c, seed=c)
        cases["wrap_c%d" % c] = _ramp(3, 300, c, 1, 0, 1)              # passes 255 -> 0
        for w in (1, 2, c + 1):
            cases["w%d_c%d" % (w, c)] = noise(5, w, c, seed=10 * w + c)
    rows = np.repeat(np.array([[3], [200], [200], [17], [90]], np.uint8), 21, axis=1)
    cases["constant_rows"] = rows[:, :, None]
    # a smooth surface with curvature: Average and Paeth rows
    y, x = np.mgrid[0:12, 0:31]
    cases["surface"] = np.stack([(x * x // 7 + y * y // 3 + x * y // 5 + k) for k in range(3)], axis=-1).astype(np.uint8)
    cases["avg"] = np.stack([(3 * x + 3 * y + ((x + y) & 1)) for k in range(1)], axis=-1).astype(np.uint8)
    for name, img in paeth_tie_cases().items():
        cases["tie_" + name] = img[:, :, None]
    return cases


def file_cases():
    """{name: (image, filter)}: the shapes the issue lists for whole files.  Streams of exactly 65520, 65519, 65521 and 131040 bytes,
    a row across a cut, a row longer than a segment, all-stored noise, coded-then-stored, the Adler case."""
    cases = {}
    for c in (1, 3, 4):
        cases["one_c%d" % c] = (noise(1, 1, c, seed=c), "adaptive")
    cases["stream_65520"] = (_ramp(80, 818, 1, 1, 2), "adaptive")              # 80 * 819
    cases["stream_65519"] = (_ramp(1, 65518, 1, 1, 0), "adaptive")
    cases["stream_65521"] = (_ramp(1, 21840, 3, 1, 0), "adaptive")             # 1 + 65520
    cases["stream_131040"] = (_ramp(160, 818, 1, 2, 1), "adaptive")            # two full segments
    cases["straddle"] = (_ramp(70, 333, 3, 1, 1), "adaptive")                  # rows of 1000 bytes: row 65 lies across the cut
    smooth = _ramp(3, 21841, 3, 1, 1)
    cases["long_row"] = (smooth, "adaptive")                                   # a row of 65524 bytes
    cases["noise_stored"] = (noise(150, 300, 3, seed=5), "adaptive")           # 135150 bytes, three stored segments
    mixed = _ramp(100, 400, 3, 1, 1)                                           # rows of 1201 bytes: 120100 bytes, the cut is in row 54
    mixed[54:] = noise(46, 400, 3, seed=6)                                     # noise from there on
    cases["coded_then_stored"] = (mixed, "adaptive")
    cases["adler_255"] = (np.full((10, 7000, 1), 255, np.uint8), "none")       # 70 000 bytes of 255 (and ten type bytes)
    for f in FILTERS:
        cases["fixed_" + f] = (noise(9, 14, 3, seed=8) // 16 + _ramp(9, 14, 3, 1, 1, 4), f)
    return cases
