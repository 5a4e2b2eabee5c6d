"""OpenEXR training files: the counterpart of hdr_io.read_rgbe / read_hdr for the HDR collections the reference reads with
cv2.imread(path, cv2.IMREAD_UNCHANGED) (dataset.py:181-186).

    hdr = read_exr("scene.exr")                  # float32 RGB [H, W, 3] on the device, the file's values (no clipping)

Scope, restated from OpenEXR 2.x's published file layout (no OpenEXR library is used):
  * magic 76 2f 31 01, version 2, single-part scanline images (the long-names flag 0x400 is allowed; tiled 0x200, deep 0x800
    and multi-part 0x1000 files are refused);
  * compression NO_COMPRESSION (0), RLE (1), ZIPS (2) and ZIP (3); PIZ (4) only where the caller asks for it (piz=, below);
    PXR24, B44, B44A, DWAA and DWAB are refused by name;
  * channels R, G and B, each HALF or FLOAT; other channels (A, Z, ...) of any type are skipped but occupy their bytes; every
    channel has x / y sampling 1;
  * any dataWindow (the image is the data window, as in OpenCV's decoder), line order INCREASING_Y or DECREASING_Y.

Layout: after the header comes a table of one uint64 file offset per chunk, indexed by increasing y whatever the line order.
A chunk is int32 y (its first scanline), int32 size, then the data of 1 scanline (NONE, RLE, ZIPS) or 16 (ZIP; the last chunk
may hold fewer).  A scanline holds, channel by channel in name-sorted order, `width` samples (HALF 2 bytes, FLOAT / UINT 4,
little-endian).  RLE and ZIP(S) both interleave the chunk's bytes (even bytes first, then odd) and delta-code them
(d[i] = t[i] - t[i-1] + 128) before compressing; a chunk whose stored size equals its decoded size is stored raw.

Split of the work: the host reads and checks the bytes and inflates (zlib, which drops the GIL) or run-length decodes
(libshdr's shdr_exr_rle_decode, via ctypes, which drops it too) every chunk; the device undoes the predictor and the
interleave (shdr_exr_unpredict_u8) and converts / resizes straight from the planar scanlines (shdr_exr_load_resize_f32,
csrc/exr.hip).  Every refusal is a ValueError naming the file and the reason.

With inflate="device" (read_exr; exr_inflate= of dataset.PatchHDRDataset and hdr_real.HdrRealFolder; opt-in) the host keeps only the
container checks (read_stored) and the device inflates too: the stored bytes of all chunks of all files go up in one copy, one
launch of K.inflate (csrc/inflate.hip, a zlib decoder with one wave per chunk; csrc/inflate.h is the decoder, shared with the host
routine K.inflate_host that the tests judge against zlib) decodes them into place, one launch undoes the predictor, and one small
copy of the chunks' status codes back is the only wait (upload_batch).  The pixels are the same bits.

PIZ (piz= of read_header / read_payload / read_stored / read_item / read_exr, exr_piz= of the dataset readers; "refuse" is the
default and keeps the refusal by name): 32 scanlines per chunk, all channels inside the PIZ data; a chunk is a bitmap of the 16-bit
values present, one Huffman-coded stream (code words of up to 58 bits, a run code) of the wavelet coefficients of every channel's
word planes, and decodes -- Huffman, inverse wavelet, reverse LUT -- to the planar scanlines themselves, with no predictor to undo
(csrc/piz.h: the rules, shared by both sides).  piz="host": libshdr's shdr_piz_decode_host decodes every chunk in the loading
threads (ctypes: no GIL).  piz="device": the file comes back as a Stored and upload_batch hands its chunks to K.piz_decode
(csrc/piz.hip) beside the K.inflate launch of the ZIP files, into one buffer.  The PIZ reader is UNPINNED: the format is restated
from memory of OpenEXR 2.x, and no OpenEXR-written file has been read (the tests' files come from tests/piz_ref.py, an
independent restatement of the same rules).

Writing (encode_exr / write_exr) mirrors that split.  The device converts float32 to HALF or FLOAT, lays the samples out as planar
scanlines (B, G, R) and applies the interleave and the delta predictor, all chunks of a batch of images in one launch
(K.exr_pack, csrc/exr_write.hip).  With encoder="host" the predicted bytes come back and zlib.compress deflates every chunk in a
bounded thread pool (full deflate, the better ratio); with encoder="device" a Huffman-only zlib encoder codes them on the device
(K.deflate_huffman, csrc/deflate.hip), with encoder="device_lz" one that also finds LZ77 matches (K.deflate_lz, csrc/deflate_lz.hip:
smaller files than "device", larger than "host"); a last kernel writes the chunk headers and the offset tables, and everything that follows
the file headers comes back in one copy.  Either way a chunk that does not get strictly smaller is stored raw.  Files are
single-part scanline, channels B, G, R of one type, data window (0, 0) - (W - 1, H - 1), INCREASING_Y, NONE / ZIPS / ZIP.
"""
import collections
import concurrent.futures
import ctypes
import struct
import zlib

import numpy as np
import torch

try:
    from . import _lib
    from . import _ops as K
except ImportError:
    import _lib
    import _ops as K

MAGIC = b"\x76\x2f\x31\x01"
UINT, HALF, FLOAT = 0, 1, 2
SAMPLE_BYTES = {UINT: 4, HALF: 2, FLOAT: 4}
NO_COMPRESSION, RLE_COMPRESSION, ZIPS_COMPRESSION, ZIP_COMPRESSION, PIZ_COMPRESSION = 0, 1, 2, 3, 4
COMPRESSION_NAMES = ("NO_COMPRESSION", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB")
LINES_PER_CHUNK = {NO_COMPRESSION: 1, RLE_COMPRESSION: 1, ZIPS_COMPRESSION: 1, ZIP_COMPRESSION: 16}
LINES_PER_CHUNK_PIZ = {**LINES_PER_CHUNK, PIZ_COMPRESSION: 32}           # what a reader asked for PIZ (piz=) accepts
PIZ_WORDS = {UINT: 2, HALF: 1, FLOAT: 2}                                    # 16-bit words of a sample in a PIZ chunk
INCREASING_Y, DECREASING_Y = 0, 1
FLAG_TILED, FLAG_LONG_NAMES, FLAG_DEEP, FLAG_MULTIPART = 0x200, 0x400, 0x800, 0x1000
MAX_SIDE = 1 << 20                 # a larger data window is refused as absurd
MAX_PIXELS = 1 << 28

Channel = collections.namedtuple("Channel", "name type offset")      # offset: byte offset of the channel's run in a scanline
Header = collections.namedtuple("Header", "data_window width height channels compression line_order lines row_bytes n_chunks "
                                          "table_offset")
Payload = collections.namedtuple("Payload", "header data offsets coded")
Stored = collections.namedtuple("Stored", "header path data src_offsets offsets mode")
"""data: uint8 [offsets[-1]], the chunks in increasing-y order; offsets: int64 [n_chunks + 1], chunk c at
data[offsets[c]:offsets[c + 1]] (min(lines, rows left) * row_bytes bytes); coded: uint8 [n_chunks], 1 where the predictor and
the interleave are still to be undone (0 for raw chunks and NO_COMPRESSION)"""
"""Stored (read_stored): a ZIP / ZIPS (or, with piz="device", PIZ) file whose chunks are still as the file holds them.  data: uint8, the chunks' stored bytes back to
back in increasing-y order, chunk headers stripped; src_offsets: int64 [n_chunks + 1], chunk c is data[src_offsets[c]:src_offsets[c + 1]];
offsets: the decoded offsets, identical to Payload.offsets; mode: uint8 [n_chunks], 1 a zlib stream (of a PIZ file: a PIZ chunk), 0
stored raw (K.inflate's and K.piz_decode's mode bytes; header.compression says which); path: the file, for error messages"""


def is_exr(path):
    with open(path, "rb") as f:
        return f.read(4) == MAGIC


def _fail(path, reason):
    return ValueError("%s: %s" % (path, reason))


def _cstr(data, pos, max_len, path, what):
    end = data.find(b"\0", pos, pos + max_len + 1)
    if end < 0:
        raise _fail(path, "truncated header" if data.find(b"\0", pos) < 0 else "%s longer than %d bytes" % (what, max_len))
    return data[pos:end], end + 1


def _unpack(fmt, data, pos, path):
    n = struct.calcsize(fmt)
    if pos + n > len(data):
        raise _fail(path, "truncated header")
    return struct.unpack_from(fmt, data, pos)


def _parse_chlist(value, path, max_name):
    chans, pos = [], 0
    while True:
        if pos >= len(value):
            raise _fail(path, "truncated channel list")
        if value[pos] == 0:
            break
        name, pos = _cstr(value, pos, max_name, path, "channel name")
        if pos + 16 > len(value):
            raise _fail(path, "truncated channel list")
        ptype, _, xs, ys = struct.unpack_from("<iB3xii", value, pos)
        pos += 16
        if ptype not in SAMPLE_BYTES:
            raise _fail(path, "channel %r has unknown pixel type %d" % (name.decode("latin-1"), ptype))
        if xs != 1 or ys != 1:
            raise _fail(path, "channel %r has sampling %d x %d (only 1 is supported)" % (name.decode("latin-1"), xs, ys))
        chans.append((name, ptype))
    return chans


def _parse_header(data, path, piz=False):
    if len(data) < 8:
        raise _fail(path, "truncated header")
    if data[:4] != MAGIC:
        raise _fail(path, "not an OpenEXR file")
    version, = struct.unpack_from("<I", data, 4)
    if version & 0xFF != 2:
        raise _fail(path, "OpenEXR version %d (only 2 is supported)" % (version & 0xFF))
    for flag, what in ((FLAG_TILED, "tiled"), (FLAG_DEEP, "deep"), (FLAG_MULTIPART, "multi-part")):
        if version & flag:
            raise _fail(path, "%s OpenEXR files are not supported (single-part scanline only)" % what)
    if version & ~0xFF & ~FLAG_LONG_NAMES:
        raise _fail(path, "unknown version flags 0x%x" % (version & ~0xFF))
    max_name = 255 if version & FLAG_LONG_NAMES else 31
    attrs, pos = {}, 8
    while True:
        if pos >= len(data):
            raise _fail(path, "truncated header")
        if data[pos] == 0:
            pos += 1
            break
        name, pos = _cstr(data, pos, max_name, path, "attribute name")
        atype, pos = _cstr(data, pos, max_name, path, "attribute type")
        size, = _unpack("<i", data, pos, path)
        pos += 4
        if size < 0 or pos + size > len(data):
            raise _fail(path, "truncated header")
        attrs[name] = (atype, data[pos:pos + size])
        pos += size

    def attr(name, atype, size=None):
        if name not in attrs:
            raise _fail(path, "missing header attribute %r" % name.decode())
        t, v = attrs[name]
        if t != atype or (size is not None and len(v) != size):
            raise _fail(path, "header attribute %r has type %r, size %d" % (name.decode(), t.decode("latin-1"), len(v)))
        return v

    if b"type" in attrs and attrs[b"type"][1].rstrip(b"\0") != b"scanlineimage":
        raise _fail(path, "part type %r is not supported (scanline images only)" % attrs[b"type"][1].decode("latin-1"))
    comp = attr(b"compression", b"compression", 1)[0]
    lines_per_chunk = LINES_PER_CHUNK_PIZ if piz else LINES_PER_CHUNK
    if comp not in lines_per_chunk:
        name = COMPRESSION_NAMES[comp] if comp < len(COMPRESSION_NAMES) else "unknown (%d)" % comp
        raise _fail(path, "%s compression is not supported (NO_COMPRESSION, RLE, ZIPS and ZIP are)" % name)
    order = attr(b"lineOrder", b"lineOrder", 1)[0]
    if order not in (INCREASING_Y, DECREASING_Y):
        raise _fail(path, "line order %d is not supported (INCREASING_Y or DECREASING_Y)" % order)
    xmin, ymin, xmax, ymax = struct.unpack("<iiii", attr(b"dataWindow", b"box2i", 16))
    width, height = xmax - xmin + 1, ymax - ymin + 1
    if width <= 0 or height <= 0 or width > MAX_SIDE or height > MAX_SIDE or width * height > MAX_PIXELS:
        raise _fail(path, "data window (%d, %d) - (%d, %d) is empty or absurd" % (xmin, ymin, xmax, ymax))
    chans = sorted(_parse_chlist(attr(b"channels", b"chlist"), path, max_name))     # the layout's order, whatever the list's
    names = [n for n, _ in chans]
    if len(set(names)) != len(names):
        raise _fail(path, "duplicate channel names")
    for need in (b"R", b"G", b"B"):
        if need not in names:
            raise _fail(path, "no %s channel (RGB images only; luminance / chroma files are not supported)" % need.decode())
    channels, off = [], 0
    for n, t in chans:
        if n in (b"R", b"G", b"B") and t == UINT:
            raise _fail(path, "channel %s is UINT (colour channels must be HALF or FLOAT)" % n.decode())
        channels.append(Channel(n.decode("latin-1"), t, off))
        off += SAMPLE_BYTES[t] * width
    lines = lines_per_chunk[comp]
    n_chunks = -(-height // lines)
    if pos + 8 * n_chunks > len(data):
        raise _fail(path, "truncated offset table")
    return Header((xmin, ymin, xmax, ymax), width, height, tuple(channels), comp, order, lines, off, n_chunks, pos)


def read_header(path, piz=False):
    """the data window, the channel list (name, type, byte offset in a scanline; layout order), compression, line order, lines
    per chunk, scanline bytes and chunk count of an OpenEXR file; ValueError (naming the file) on anything out of scope.  piz: a
    PIZ file is in scope (32 lines per chunk)"""
    with open(path, "rb") as f:
        data = f.read()
    return _parse_header(data, path, piz)


def _rle_decode(src, size, dst, capacity):
    lib = _lib.load()
    n = lib.shdr_exr_rle_decode(ctypes.c_void_p(src), size, ctypes.c_void_p(dst), capacity)
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return n


def rle_decode(data, capacity):
    """OpenEXR RLE bytes -> the decoded bytes (at most `capacity`; libshdr host routine); ValueError on an overrun"""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(max(int(capacity), 1), dtype=np.uint8)
    n = _rle_decode(src.ctypes.data, src.size, out.ctypes.data, int(capacity))
    return out[:n].tobytes()


def check_piz_option(what, piz, allowed=("refuse", "host", "device")):
    if piz not in allowed:
        raise ValueError("%s: piz must be %s, got %r" % (what, " or ".join(repr(a) for a in allowed), piz))
    return piz


def read_payload(path, piz="refuse"):
    """the file's chunks decoded on the host (inflated / run-length decoded, predictor and interleave NOT undone): a Payload.
    piz="host": a PIZ file is in scope; its chunks are decoded by libshdr's host routine (K.piz_decode_host, ctypes: no GIL) into
    the planar scanlines, with nothing left to undo (coded 0)"""
    check_piz_option("read_payload", piz, ("refuse", "host"))
    with open(path, "rb") as f:
        data = f.read()
    return _payload(data, _parse_header(data, path, piz != "refuse"), path)


def piz_words(hdr):
    """the 16-bit words per sample of the header's channels, in layout order (K.piz_decode's chan_words)"""
    return [PIZ_WORDS[ch.type] for ch in hdr.channels]


def _payload(data, hdr, path):
    n, lines, row_bytes = hdr.n_chunks, hdr.lines, hdr.row_bytes
    table = np.frombuffer(data, dtype="<u8", count=n, offset=hdr.table_offset).astype(np.uint64)
    table_end = hdr.table_offset + 8 * n
    rows = np.minimum(lines, hdr.height - np.arange(n, dtype=np.int64) * lines)
    offsets = np.concatenate([[0], np.cumsum(rows * row_bytes)]).astype(np.int64)
    out = np.empty(int(offsets[-1]), dtype=np.uint8)
    coded = np.zeros(n, dtype=np.uint8)
    src = np.frombuffer(data, dtype=np.uint8)
    ymin = hdr.data_window[1]
    for c in range(n):
        o = int(table[c])
        if o < table_end or o > len(data) - 8:
            raise _fail(path, "chunk %d: offset %d lies outside the file's chunk data" % (c, o))
        y, size = struct.unpack_from("<ii", data, o)
        if y != ymin + c * lines:
            raise _fail(path, "chunk %d: y is %d, its table slot implies %d" % (c, y, ymin + c * lines))
        if size < 0 or size > len(data) - o - 8:
            raise _fail(path, "chunk %d: size %d runs past the end of the file" % (c, size))
        lo, hi = int(offsets[c]), int(offsets[c + 1])
        want = hi - lo
        raw = src[o + 8:o + 8 + size]
        if size == want:                                                 # stored raw (compression would not shrink it)
            out[lo:hi] = raw
            continue
        if size > want or hdr.compression == NO_COMPRESSION:
            raise _fail(path, "chunk %d: %d bytes stored, its %d scanlines hold %d" % (c, size, int(rows[c]), want))
        if hdr.compression == PIZ_COMPRESSION:
            _, st = K.piz_decode_host(raw, hdr.width, int(rows[c]), piz_words(hdr), out=out[lo:hi])
            if st:
                raise _fail(path, "chunk %d: PIZ error: %s" % (c, K.piz_reason(st)))
            continue                                                     # planar scanlines already: no predictor to undo
        if hdr.compression == RLE_COMPRESSION:
            try:
                got = _rle_decode(raw.ctypes.data, size, out[lo:hi].ctypes.data, want)
            except ValueError as exc:
                raise _fail(path, "chunk %d: %s" % (c, exc)) from None
        else:
            d = zlib.decompressobj()
            try:
                buf = d.decompress(data[o + 8:o + 8 + size], want + 1)
            except zlib.error as exc:
                raise _fail(path, "chunk %d: zlib error: %s" % (c, exc)) from None
            if len(buf) == want and not d.eof:
                raise _fail(path, "chunk %d: zlib error: incomplete or overlong stream" % c)
            got = len(buf)
            if got == want:
                out[lo:hi] = np.frombuffer(buf, dtype=np.uint8)
        if got != want:
            raise _fail(path, "chunk %d: decodes to %s bytes, its %d scanlines hold %d" % (
                c, got if got <= want else "more than %d" % want, int(rows[c]), want))
        coded[c] = 1
    return Payload(hdr, out, offsets, coded)


def check_inflate_option(what, inflate):
    if inflate not in ("host", "device"):
        raise ValueError("%s: inflate must be 'host' or 'device', got %r" % (what, inflate))
    return inflate


def read_stored(path, piz="refuse"):
    """the host half of the device route: every container check of read_payload, with its messages, and nothing inflated.  ZIP and
    ZIPS files come back as a Stored (the chunks' bytes as the file holds them); RLE and NO_COMPRESSION files as read_payload's
    Payload.  upload_batch takes both.  piz: a PIZ file is refused, decoded on the host into a Payload ("host"), or comes back as a
    Stored ("device") whose mode bytes mean 1 a PIZ chunk, 0 stored raw: K.piz_decode's."""
    return read_item(path, "device", piz)


def read_item(path, inflate="host", piz="refuse"):
    """read_payload or read_stored, file by file: a ZIP / ZIPS file is left stored with inflate="device", a PIZ file with
    piz="device"; everything else is decoded on the host (a PIZ file only if piz="host")"""
    check_inflate_option("read_item", inflate)
    check_piz_option("read_item", piz)
    with open(path, "rb") as f:
        data = f.read()
    hdr = _parse_header(data, path, piz != "refuse")
    if hdr.compression == PIZ_COMPRESSION:
        if piz != "device":
            return _payload(data, hdr, path)
    elif hdr.compression not in (ZIP_COMPRESSION, ZIPS_COMPRESSION) or inflate != "device":
        return _payload(data, hdr, path)
    n, lines, row_bytes = hdr.n_chunks, hdr.lines, hdr.row_bytes
    table = np.frombuffer(data, dtype="<u8", count=n, offset=hdr.table_offset).astype(np.uint64)
    table_end = hdr.table_offset + 8 * n
    rows = np.minimum(lines, hdr.height - np.arange(n, dtype=np.int64) * lines)
    offsets = np.concatenate([[0], np.cumsum(rows * row_bytes)]).astype(np.int64)
    src = np.frombuffer(data, dtype=np.uint8)
    mode = np.ones(n, dtype=np.uint8)
    parts, src_offsets = [], np.zeros(n + 1, dtype=np.int64)
    ymin = hdr.data_window[1]
    for c in range(n):
        o = int(table[c])
        if o < table_end or o > len(data) - 8:
            raise _fail(path, "chunk %d: offset %d lies outside the file's chunk data" % (c, o))
        y, size = struct.unpack_from("<ii", data, o)
        if y != ymin + c * lines:
            raise _fail(path, "chunk %d: y is %d, its table slot implies %d" % (c, y, ymin + c * lines))
        if size < 0 or size > len(data) - o - 8:
            raise _fail(path, "chunk %d: size %d runs past the end of the file" % (c, size))
        want = int(offsets[c + 1] - offsets[c])
        if size == want:                                                 # stored raw (compression would not shrink it)
            mode[c] = 0
        elif size > want:
            raise _fail(path, "chunk %d: %d bytes stored, its %d scanlines hold %d" % (c, size, int(rows[c]), want))
        parts.append(src[o + 8:o + 8 + size])
        src_offsets[c + 1] = src_offsets[c] + size
    return Stored(hdr, path, np.concatenate(parts), src_offsets, offsets, mode)


def upload_batch(items, device):
    """any mix of read_stored's Stored items and Payloads -> [(planes, offsets)] as upload() gives them, one pair per item, with all
    the work of all the files batched: one staging buffer and one copy carry the stored bytes to the device, one K.inflate launch
    decodes every ZIP / ZIPS chunk of every file into its place (chunks that are decoded already, or stored raw, are copied by that
    launch), one K.piz_decode call does the same for every chunk of the PIZ files, into the same buffer (the PIZ files' chunks lie
    behind the others in both buffers, so each call sees one contiguous part of the two offset tables), one K.exr_unpredict launch
    undoes the predictor, and one small copy of the chunks' status and byte counts back is the only host wait.
    ValueError("<path>: chunk <c>: inflate error: <reason>") (or "PIZ error") for the first chunk, in file order, that a kernel refuses."""
    items = list(items)
    if not items:
        return []
    is_piz = [isinstance(it, Stored) and it.header.compression == PIZ_COMPRESSION for it in items]
    order = [i for i in range(len(items)) if not is_piz[i]] + [i for i in range(len(items)) if is_piz[i]]
    n_chunks = [items[i].header.n_chunks for i in order]
    first = np.concatenate([[0], np.cumsum(n_chunks)]).astype(np.int64)          # of the items in `order`
    n = int(first[-1])
    n_z = int(first[len(items) - sum(is_piz)])                                   # chunks in front of the PIZ files'
    # one int64 table: source offsets, slot offsets, then every file's own chunk offsets (what load_resize reads)
    tables = np.empty(2 * (n + 1) + n + len(items), dtype=np.int64)
    src_off, dst_off, own = tables[:n + 1], tables[n + 1:2 * (n + 1)], tables[2 * (n + 1):]
    flags = np.empty(2 * n, dtype=np.uint8)
    mode, coded = flags[:n], flags[n:]
    geom, words = np.zeros((n - n_z, 4), dtype=np.int32), []
    parts, s_at, d_at, own_at = [], 0, 0, []
    for k, i in enumerate(order):
        it = items[i]
        a, b = int(first[k]), int(first[k + 1])
        if isinstance(it, Stored):
            parts.append(it.data)
            src_off[a:b + 1] = s_at + it.src_offsets
            mode[a:b] = it.mode
            coded[a:b] = 0 if is_piz[i] else it.mode                      # a PIZ chunk decodes to the scanlines themselves
            s_at += int(it.src_offsets[-1])
            if is_piz[i]:
                hdr = it.header
                geom[a - n_z:b - n_z, 0] = hdr.width
                geom[a - n_z:b - n_z, 1] = np.minimum(hdr.lines, hdr.height - np.arange(b - a) * hdr.lines)
                geom[a - n_z:b - n_z, 2] = len(words)
                geom[a - n_z:b - n_z, 3] = len(hdr.channels)
                words += piz_words(hdr)
        else:                                                            # decoded on the host: copied as it is
            parts.append(it.data)
            src_off[a:b + 1] = s_at + it.offsets
            mode[a:b] = 0
            coded[a:b] = it.coded
            s_at += int(it.offsets[-1])
        dst_off[a:b + 1] = d_at + it.offsets
        d_at += int(it.offsets[-1])
        own_at.append(a + k)
        own[a + k:b + k + 1] = it.offsets
    staging = torch.empty(max(s_at, 1), dtype=torch.uint8).pin_memory()         # alive until the wait below
    if s_at:
        np.concatenate(parts, out=staging.numpy()[:s_at])
    src = staging.to(device, non_blocking=True)[:s_at]
    tables_dev = torch.from_numpy(tables).to(device)
    flags_dev = torch.from_numpy(flags).to(device)
    src_off_dev, dst_off_dev, own_dev = tables_dev[:n + 1], tables_dev[n + 1:2 * (n + 1)], tables_dev[2 * (n + 1):]
    dst = torch.empty(d_at, device=device, dtype=torch.uint8)
    status, written = [], []
    if n_z:
        _, w, st = K.inflate(src, src_off[:n_z + 1], dst_off[:n_z + 1], mode=flags_dev[:n_z], src_offsets_dev=src_off_dev[:n_z + 1],
                             dst_offsets_dev=dst_off_dev[:n_z + 1], dst=dst)
        status.append(st)
        written.append(w)
    if n > n_z:
        _, w, st = K.piz_decode(src, src_off[n_z:], dst_off[n_z:], geom, words, mode=flags_dev[n_z:n], src_offsets_dev=src_off_dev[n_z:],
                                dst_offsets_dev=dst_off_dev[n_z:], dst=dst)
        status.append(st)
        written.append(w)
    planes = K.exr_unpredict(dst, dst_off_dev, flags_dev[n:]) if coded.any() else dst
    result = torch.stack([torch.cat(status).to(torch.int64), torch.cat(written)]).cpu().numpy()       # the host waits here, once
    bad = np.flatnonzero((result[0] != 0) | (result[1] != np.diff(dst_off)))
    if bad.size:
        k = np.searchsorted(first, bad, side="right") - 1                        # the items (in `order`) of the bad chunks
        j = int(np.argmin(np.asarray(order)[k]))                                 # the first of them in file order (bad is sorted)
        c, k = int(bad[j]), int(k[j])
        st = int(result[0, c])
        reason = (K.piz_reason if c >= n_z else K.inflate_reason)(st)
        raise _fail(getattr(items[order[k]], "path", "item %d" % order[k]), "chunk %d: %s error: %s" % (
            c - int(first[k]), "PIZ" if c >= n_z else "inflate",
            reason if st else "%d bytes written, its slot holds %d" % (result[1, c], dst_off[c + 1] - dst_off[c])))
    out = [None] * len(items)
    for k, i in enumerate(order):
        lo = int(dst_off[first[k]])
        out[i] = (planes[lo:lo + int(items[i].offsets[-1])], own_dev[own_at[k]:own_at[k] + n_chunks[k] + 1])
    return out


def channel_table(header, order="RGB"):
    """(byte offsets, types) of the channels named by `order` ("RGB", or "BGR" for the training arena)"""
    by_name = {ch.name: ch for ch in header.channels}
    return [by_name[c].offset for c in order], [by_name[c].type for c in order]


def upload(payload, device):
    """the payload on the device with the predictor undone: (planar scanline bytes, chunk offsets) as uint8 / int64 tensors"""
    data = torch.from_numpy(payload.data).to(device)
    offsets = torch.from_numpy(payload.offsets).to(device)
    if not payload.coded.any():
        return data, offsets
    coded = torch.from_numpy(payload.coded).to(device)
    return K.exr_unpredict(data, offsets, coded), offsets


def load_resize(payload, planes, offsets, out, order="RGB", clip=False):
    """the payload's image (of upload()) converted to float32 in channel order `order` and resized into out [H, W, 3]"""
    hdr = payload.header
    chan_off, chan_type = channel_table(hdr, order)
    return K.exr_load_resize(planes, offsets, hdr.lines, hdr.row_bytes, chan_off, chan_type, hdr.height, hdr.width, out, clip)


def read_exr(path, device=None, inflate="host", piz="refuse"):
    """OpenEXR file -> float32 RGB [H, W, 3] on the device (the data window; the file's values, HALF converted exactly, no
    clipping): the EXR counterpart of hdr_io.read_hdr.  inflate: who inflates ZIP / ZIPS chunks -- "host" (zlib) or "device"
    (K.inflate, csrc/inflate.hip: the stored bytes are uploaded); piz: a PIZ file is refused ("refuse"), decoded by libshdr's host
    routine ("host") or by K.piz_decode ("device", csrc/piz.hip); the pixels are the same"""
    check_inflate_option("read_exr", inflate)
    check_piz_option("read_exr", piz)
    device = device or torch.device("cuda", torch.cuda.current_device())
    payload = read_item(path, inflate, piz)
    if inflate == "device" or isinstance(payload, Stored):
        (planes, offsets), = upload_batch([payload], device)
    else:
        planes, offsets = upload(payload, device)
    out = torch.empty((payload.header.height, payload.header.width, 3), device=device, dtype=torch.float32)
    return load_resize(payload, planes, offsets, out, "RGB", clip=False)


# ---- writing ----------------------------------------------------------------------------------------------------------------
PIXEL_TYPES = {"half": HALF, "float": FLOAT}
WRITE_COMPRESSIONS = {"none": NO_COMPRESSION, "zips": ZIPS_COMPRESSION, "zip": ZIP_COMPRESSION}
MAX_DEFLATE_THREADS = 16           # zlib drops the GIL; the bound of dataset.MAX_LOAD_THREADS


def _attr(name, atype, value):
    return name + b"\0" + atype + b"\0" + struct.pack("<i", len(value)) + value


def file_header(height, width, pixel_type, compression):
    """magic, version 2 and the eight attributes OpenEXR requires, in name order, for a B, G, R image of one pixel type"""
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", pixel_type, 0, 1, 1) for n in (b"B", b"G", b"R")) + b"\0"
    box = struct.pack("<iiii", 0, 0, width - 1, height - 1)
    return (MAGIC + struct.pack("<I", 2)
            + _attr(b"channels", b"chlist", chlist)
            + _attr(b"compression", b"compression", bytes([compression]))
            + _attr(b"dataWindow", b"box2i", box)
            + _attr(b"displayWindow", b"box2i", box)
            + _attr(b"lineOrder", b"lineOrder", bytes([INCREASING_Y]))
            + _attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
            + _attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
            + _attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def _write_options(what, pixel_type, compression, encoder, piz="refuse"):
    if pixel_type not in PIXEL_TYPES:
        raise ValueError("%s: pixel type %r is not supported ('half' or 'float')" % (what, pixel_type))
    check_piz_option(what, piz)
    if compression == "piz" and piz != "refuse":                        # asked for by name: piz="host" or "device"
        comp = PIZ_COMPRESSION
    elif compression not in WRITE_COMPRESSIONS:
        raise ValueError("%s: %s compression is not supported ('none', 'zips' and 'zip' are%s)" % (
            what, compression.upper() if isinstance(compression, str) else repr(compression),
            "; 'piz' with piz='host' or 'device'" if compression == "piz" else ""))
    elif piz != "refuse":
        raise ValueError("%s: piz=%r goes with compression='piz' only, got %r" % (what, piz, compression))
    else:
        comp = WRITE_COMPRESSIONS[compression]
    if encoder not in ("host", "device", "device_lz"):
        raise ValueError("%s: encoder must be 'host', 'device' or 'device_lz', got %r" % (what, encoder))
    return PIXEL_TYPES[pixel_type], comp


def _on_device(images, what):
    def one(x):
        if isinstance(x, np.ndarray):
            if x.dtype != np.float32:
                raise ValueError("%s: expected float32 images, got %s" % (what, x.dtype))
            return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", torch.cuda.current_device()))
        return x
    return [one(x) for x in images] if isinstance(images, (list, tuple)) else one(images)


def _assemble(header, lines, stored):
    """one file: header, offset table, then per chunk int32 y, int32 size and the stored bytes"""
    n = len(stored)
    pos = len(header) + 8 * n
    table, parts = [], []
    for c, data in enumerate(stored):
        table.append(pos)
        parts.append(struct.pack("<ii", c * lines, len(data)))
        parts.append(data)
        pos += 8 + len(data)
    return header + struct.pack("<%dQ" % n, *table) + b"".join(parts)


def _piz_geometry(packed, ptype):
    """(geom int32 [n_chunks, 4], chan_words) of the packed batch's chunks for K.piz_encode: B, G, R of one pixel type"""
    words = PIZ_WORDS[ptype]
    first = packed.table[0]
    geom = np.zeros((packed.chunk_off.size - 1, 4), dtype=np.int32)
    for i, (h, w) in enumerate(packed.shapes):
        a, b = int(first[i]), int(first[i + 1])
        geom[a:b, 0] = w
        geom[a:b, 1] = np.minimum(packed.lines, int(h) - np.arange(b - a) * packed.lines)
    geom[:, 3] = 3
    return geom, [words] * 3


def encode_exr(images, pixel_type="half", compression="zip", encoder="host", saturate=True, reverse_channels=False, piz="refuse"):
    """float32 images -> a list of OpenEXR files as `bytes`, one per image.  images: one [H, W, 3], one [N, H, W, 3] or a list of
    [H, W, 3] of different sizes, device tensors (float32 host arrays are uploaded).  pixel_type "half" (numpy's astype(float16);
    saturate: finite values beyond +-65504 become +-65504 instead of inf) or "float"; compression "none", "zips", "zip" or -- only
    together with piz="host" / "device" -- "piz"; reverse_channels: channel 0 is blue (HdrReconstructor.reconstruct_device's order).
    encoder: who deflates ZIP / ZIPS chunks -- "host": zlib.compress per chunk in a thread pool; "device": the Huffman-only encoder
    of csrc/deflate.hip (larger files, no host deflate, one copy of the finished bytes); "device_lz": the same route with the LZ77
    encoder of csrc/deflate_lz.hip (matches from a chainless hash table and runs: files between the two).  piz: who codes PIZ chunks
    (32 scanlines each) -- "refuse" (the default: compression="piz" is a ValueError, as it always was), "host": libshdr's host
    encoder per chunk in the thread pool, "device": K.piz_encode (csrc/piz_enc.hip) and one copy of the finished bytes; both write the
    same files, and `encoder` plays no part in them.  THE PIZ WRITER IS UNPINNED AGAINST THE OPENEXR LIBRARY, like the PIZ reader: no
    OpenEXR-built reader has opened these files (tests/piz_ref.py writes the same bytes, and this package's readers read them back).
    The whole batch is packed, predicted and (device) coded in one call each."""
    ptype, comp = _write_options("encode_exr", pixel_type, compression, encoder, piz)
    lines = LINES_PER_CHUNK_PIZ[comp]
    packed = K.exr_pack(_on_device(images, "encode_exr"), ptype, lines, reverse_channels, saturate,
                        predict=comp not in (NO_COMPRESSION, PIZ_COMPRESSION))
    headers = [file_header(int(h), int(w), ptype, comp) for h, w in packed.shapes]
    first, chunk_off = packed.table[0], packed.chunk_off
    n_chunks = chunk_off.size - 1
    on_device = piz == "device" if comp == PIZ_COMPRESSION else comp != NO_COMPRESSION and encoder != "host"
    if on_device:
        if comp == PIZ_COMPRESSION:
            geom, words = _piz_geometry(packed, ptype)
            out, out_offsets, _ = K.piz_encode(packed.planar, chunk_off, geom, words, pad=8, front=8 * n_chunks,
                                               chunk_off_dev=packed.chunk_off_dev)
        else:
            deflate = K.deflate_lz if encoder == "device_lz" else K.deflate_huffman
            out, out_offsets, _ = deflate(packed.predicted, chunk_off, raw=packed.planar, pad=8, front=8 * n_chunks,
                                          offsets_dev=packed.chunk_off_dev)
        K.exr_finish_chunks(out, out_offsets, packed, [len(h) for h in headers])
        off = out_offsets.cpu().numpy()
        blob = memoryview(out[:8 * n_chunks + int(off[-1])].cpu().numpy())          # sliced without copies, joined once per file
        return [b"".join((headers[i], blob[8 * int(first[i]):8 * int(first[i + 1])],
                          blob[8 * n_chunks + int(off[first[i]]):8 * n_chunks + int(off[first[i + 1]])])) for i in range(len(headers))]
    bounds = [(int(chunk_off[c]), int(chunk_off[c + 1])) for c in range(n_chunks)]
    if comp == NO_COMPRESSION:
        planar = packed.planar.cpu().numpy()
        stored = [planar[a:b] for a, b in bounds]
    else:
        planar = None
        if comp == PIZ_COMPRESSION:
            planar = packed.planar.cpu().numpy()
            geom, words = _piz_geometry(packed, ptype)
            jobs = [(planar[a:b], int(g[0]), int(g[1])) for (a, b), g in zip(bounds, geom)]
            with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_DEFLATE_THREADS, n_chunks)) as pool:
                stored = list(pool.map(lambda j: K.piz_encode_host(j[0], j[1], j[2], words), jobs))
        else:
            predicted = packed.predicted.cpu().numpy()
            with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_DEFLATE_THREADS, n_chunks)) as pool:
                stored = list(pool.map(zlib.compress, [predicted[a:b] for a, b in bounds]))
        for c, (a, b) in enumerate(bounds):
            if len(stored[c]) >= b - a:                                   # does not shrink: the scanline bytes as they are
                if planar is None:
                    planar = packed.planar.cpu().numpy()
                stored[c] = planar[a:b]
    return [_assemble(headers[i], lines, stored[int(first[i]):int(first[i + 1])]) for i in range(len(headers))]


def write_exr(path, image, pixel_type="half", compression="zip", encoder="host", saturate=True, reverse_channels=False, piz="refuse"):
    """one float32 image [H, W, 3] -> an OpenEXR file (encode_exr)"""
    if getattr(image, "ndim", 0) != 3:
        raise ValueError("write_exr: expected one image [H, W, 3], got shape %s" % (tuple(getattr(image, "shape", ())),))
    data = encode_exr([image], pixel_type, compression, encoder, saturate, reverse_channels, piz)[0]
    with open(path, "wb") as f:
        f.write(data)
