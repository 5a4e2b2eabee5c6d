"""Baseline-JPEG files decoded on the device, bit for bit what PIL (libjpeg-turbo: islow IDCT, fancy upsampling) returns.

    rgb = jpeg.decode(["a.jpg", "b.jpg", data])        # one batch call -> uint8 RGB [H, W, 3] device tensors
    img = jpeg.read_ldr_device("scene.jpg")            # hdr_io.read_ldr on the device; PIL for what is out of scope

Split of the work, as for OpenEXR (exr.py): the host checks the container -- parse() walks the markers (SOF, DQT, DHT, DRI, SOS,
the EXIF Orientation), removes the FF 00 byte stuffing and cuts the scan at its RSTn markers with vectorised NumPy, and builds
per Huffman table what the kernel reads (a 9-bit look-ahead table, maxcode / valoff for longer codes, as libjpeg's jdhuff.c).
It touches no bit and no coefficient.  The device (csrc/jpeg.hip) decodes the Huffman stream with the self-synchronising
scheme of Weissenberger & Schmidt, undoes the DC prediction, dequantises, runs the islow IDCT, upsamples and converts to RGB.
With unstuff="device" (opt-in) the host walks the markers only up to SOS (parse_header) and the device also finds the end of the
scan, removes the stuffing and fills the segment arena (plan_device, csrc/jpeg_scan.hip): the same arena, the same exceptions.

In scope: SOF0 / SOF1 (8-bit, Huffman), one component (grey) or three (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1
(4:4:4, 4:2:2, 4:2:0), one interleaved scan, any restart interval, any legal DHT.  Everything else raises Unsupported with the
reason (progressive, arithmetic, 12-bit, lossless, four components, Adobe transform=0 RGB, other samplings, several scans, not
a JPEG at all); a damaged file raises CorruptJpeg, from the host checks before anything is launched or from the device's error
word after it.

The other direction (at the end of this file): encode() / write_jpeg() write baseline files on the device, byte for byte what PIL
writes for the same quality, subsampling and restart interval (csrc/jpeg_enc.hip; the rules are csrc/jpeg_enc.h).

    files = jpeg.encode([u8_a, u8_b], quality=90, subsampling="420")     # uint8 RGB device tensors of any sizes -> list of bytes
"""
import collections
import ctypes
import os
import struct

import numpy as np

try:
    from . import _lib
except ImportError:
    import _lib

SUBSEQ_BITS = 512              # bits per subsequence (one thread): the shortest device time of 256 / 512 / 1024 / 2048 on all three
                               # inputs of tools/jpeg_bench.py
WG = 256                       # subsequences per workgroup
HUFF_BYTES = 1416              # SHDR_JPEG_HUFF_BYTES
TABLE_BYTES = 512 + 4 * HUFF_BYTES

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)            # zigzag index -> natural (row-major) position

LAYOUTS = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}
DEVICE_ERRORS = {1: "a bit pattern that is no code word", 2: "the entropy-coded data ends before the image is complete",
                 3: "a run of zeros leaves its block"}


class Unsupported(ValueError):
    """a file this decoder does not handle (hdr_io.read_ldr does)"""


class CorruptJpeg(ValueError):
    """a damaged JPEG file"""


Component = collections.namedtuple("Component", "id h v tq td ta")
Header = collections.namedtuple("Header", "width height components layout qtables htables restart_interval scan_start scan_end "
                                          "rst_offsets orientation")
"""components: Component(id, h, v, tq, td, ta) in scan order; layout: "grey", "444", "422" or "420"; qtables: {id: uint16 [64],
natural order}; htables: {(class, id): (counts uint8 [16], symbols uint8 [n])}, class 0 = DC, 1 = AC; restart_interval in MCUs
(0: none); the entropy-coded data is data[scan_start:scan_end]; rst_offsets: file offsets of the FF of every RSTn marker in
it; orientation: the EXIF Orientation (1 if absent)"""


def _name(item):
    return "<%d bytes>" % len(item) if isinstance(item, (bytes, bytearray, memoryview)) else str(item)


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, "rb") as f:
        return f.read()


def _exif_orientation(seg):
    """the Orientation tag (0x0112) of IFD0 of an APP1 Exif payload, or None"""
    if len(seg) < 14 or seg[:6] != b"Exif\0\0":
        return None
    tiff = seg[6:]
    if tiff[:2] == b"II":
        e = "<"
    elif tiff[:2] == b"MM":
        e = ">"
    else:
        return None
    magic, ifd = struct.unpack_from(e + "HI", tiff, 2)
    if magic != 42 or ifd + 2 > len(tiff):
        return None
    n, = struct.unpack_from(e + "H", tiff, ifd)
    for i in range(n):
        o = ifd + 2 + 12 * i
        if o + 12 > len(tiff):
            return None
        tag, typ, count = struct.unpack_from(e + "HHI", tiff, o)
        if tag == 0x0112:
            if typ != 3 or count != 1:
                return None
            return struct.unpack_from(e + "H", tiff, o + 8)[0]
    return None


def _check_huffman(counts, nsym, what):
    if nsym > 256:
        raise CorruptJpeg("%s has %d symbols (at most 256)" % (what, nsym))
    code = 0
    for l in range(1, 17):
        code += int(counts[l - 1])
        if code > (1 << l):
            raise CorruptJpeg("%s over-subscribes the code space at length %d" % (what, l))
        code <<= 1


SOF_NAMES = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
             0xC7: "differential lossless", 0xC9: "arithmetic-coded", 0xCA: "arithmetic-coded progressive",
             0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded differential", 0xCE: "arithmetic-coded differential",
             0xCF: "arithmetic-coded differential"}


ScanHeader = collections.namedtuple("ScanHeader", "width height components layout qtables htables restart_interval scan_start orientation")
"""what parse_header returns: the fields of Header that do not depend on the bytes of the scan"""


def parse_header(data):
    """bytes of a JPEG file -> ScanHeader: the marker walk up to and including the SOS header.  No byte of the scan is touched;
    Unsupported / CorruptJpeg with the reason"""
    data = bytes(data)
    n = len(data)
    if n < 2 or data[0] != 0xFF:
        raise Unsupported("not a JPEG file")
    if data[1] != 0xD8:
        raise CorruptJpeg("no SOI marker")
    qtables, htables = {}, {}
    frame = None
    restart = 0
    orientation = None
    adobe = None
    pos = 2
    while True:
        while pos < n and data[pos] != 0xFF:                      # (garbage between segments is skipped, as libjpeg does)
            pos += 1
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise CorruptJpeg("no SOS marker before the end of the file")
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise CorruptJpeg("EOI before any scan")
        if pos + 2 > n:
            raise CorruptJpeg("truncated marker segment")
        length, = struct.unpack_from(">H", data, pos)
        if length < 2 or pos + length > n:
            raise CorruptJpeg("the length of segment FF%02X at byte %d runs past the end of the file" % (m, pos - 2))
        seg = data[pos + 2:pos + length]
        pos += length
        if m in SOF_NAMES:
            raise Unsupported("%s JPEG (SOF%d)" % (SOF_NAMES[m], m - 0xC0))
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise CorruptJpeg("two frame headers")
            if len(seg) < 6:
                raise CorruptJpeg("truncated frame header")
            prec, h, w, nc = struct.unpack_from(">BHHB", seg, 0)
            if prec != 8:
                raise Unsupported("%d-bit samples (8 only)" % prec)
            if len(seg) < 6 + 3 * nc:
                raise CorruptJpeg("truncated frame header")
            if w == 0 or h == 0:
                raise Unsupported("no size in the frame header (DNL)" if w else "zero width")
            if nc not in (1, 3):
                raise Unsupported("%d components (1 or 3)" % nc)
            frame = (w, h, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)])
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or p + 1 + size > len(seg):
                    raise CorruptJpeg("bad quantisation table segment")
                zz = np.frombuffer(seg, dtype=">u2" if pq else np.uint8, count=64, offset=p + 1).astype(np.uint16)
                table = np.zeros(64, dtype=np.uint16)
                table[ZIGZAG] = zz
                qtables[tq] = table
                p += 1 + size
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 3 or p + 17 > len(seg):
                    raise CorruptJpeg("bad Huffman table segment")
                counts = np.frombuffer(seg, dtype=np.uint8, count=16, offset=p + 1)
                nsym = int(counts.sum())
                _check_huffman(counts, nsym, "Huffman table %s%d" % ("AC" if tc else "DC", th))
                if p + 17 + nsym > len(seg):
                    raise CorruptJpeg("bad Huffman table segment")
                htables[(tc, th)] = (counts.copy(), np.frombuffer(seg, dtype=np.uint8, count=nsym, offset=p + 17).copy())
                p += 17 + nsym
        elif m == 0xDD:
            if len(seg) != 2:
                raise CorruptJpeg("bad DRI segment")
            restart, = struct.unpack(">H", seg)
        elif m == 0xE1 and orientation is None:
            orientation = _exif_orientation(seg)
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            break
    if frame is None:
        raise CorruptJpeg("SOS before the frame header")
    width, height, fcomps = frame
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise CorruptJpeg("bad scan header")
    ns = seg[0]
    if ns != len(fcomps):
        raise Unsupported("several scans (the first holds %d of %d components)" % (ns, len(fcomps)))
    if (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]) != (0, 63, 0):
        raise Unsupported("a scan that is not the whole spectrum at full precision")
    comps = []
    for i in range(ns):
        cid, tables = seg[1 + 2 * i], seg[2 + 2 * i]
        match = [c for c in fcomps if c[0] == cid]
        if len(match) != 1:
            raise CorruptJpeg("the scan names component %d, the frame has not" % cid)
        _, h, v, tq = match[0]
        comps.append(Component(cid, h, v, tq, tables >> 4, tables & 15))
    if [c.id for c in comps] != [c[0] for c in fcomps]:
        raise Unsupported("a scan whose components are not in the frame's order")
    for c in comps:
        if c.tq not in qtables:
            raise CorruptJpeg("component %d references quantisation table %d, which the file does not define" % (c.id, c.tq))
        for cls, t in ((0, c.td), (1, c.ta)):
            if (cls, t) not in htables:
                raise CorruptJpeg("component %d references Huffman table %s%d, which the file does not define" % (
                    c.id, "AC" if cls else "DC", t))
    if len(comps) == 1:
        layout = "grey"
    else:
        if adobe == 0:
            raise Unsupported("Adobe transform=0 (RGB stored without a colour transform)")
        ids = [c.id for c in comps]
        if adobe is None and ids == [ord("R"), ord("G"), ord("B")]:
            raise Unsupported("components named R, G, B (stored without a colour transform)")
        key = (comps[0].h, comps[0].v)
        if key not in LAYOUTS or any((c.h, c.v) != (1, 1) for c in comps[1:]):
            raise Unsupported("sampling factors %s (4:4:4, 4:2:2 and 4:2:0 only)" % "/".join("%dx%d" % (c.h, c.v) for c in comps))
        layout = LAYOUTS[key]
    return ScanHeader(width, height, tuple(comps), layout, qtables, htables, restart, pos, orientation if orientation is not None else 1)


def parse(data):
    """bytes of a JPEG file -> Header; Unsupported / CorruptJpeg with the reason"""
    data = bytes(data)
    hd = parse_header(data)
    # the entropy-coded data ends at the first marker that is neither stuffing (FF 00), a fill byte (FF FF) nor RSTn
    scan_start = hd.scan_start
    buf = np.frombuffer(data, dtype=np.uint8, offset=scan_start)
    nxt = buf[1:]
    is_ff = buf[:-1] == 0xFF
    rst = is_ff & (nxt >= 0xD0) & (nxt <= 0xD7)
    other = np.flatnonzero(is_ff & (nxt != 0) & (nxt != 0xFF) & ~rst)
    if other.size == 0:
        raise CorruptJpeg("no EOI marker: the file is cut inside its entropy-coded data")
    end = int(other[0])
    if buf[end + 1] != 0xD9:
        if buf[end + 1] in (0xDA, 0xC4, 0xDB, 0xDD):
            raise Unsupported("several scans")
        raise Unsupported("marker FF%02X after the scan" % buf[end + 1])
    if np.any(is_ff[:end] & (nxt[:end] == 0xFF)):
        raise Unsupported("fill bytes inside the entropy-coded data")
    rst_offsets = np.flatnonzero(rst[:end]).astype(np.int64) + scan_start
    return Header(hd.width, hd.height, hd.components, hd.layout, hd.qtables, hd.htables, hd.restart_interval, scan_start, scan_start + end,
                  rst_offsets, hd.orientation)


def geometry(header):
    """(mcus_x, mcus_y, blocks per MCU, [(h, v, bw, bh, cw, ch) per component]): the padded block grid and libjpeg's
    downsampled size of every component"""
    if header.layout == "grey":                                   # a single-component scan is not interleaved: MCU = one block
        mx, my = -(-header.width // 8), -(-header.height // 8)
        return mx, my, 1, [(1, 1, mx, my, header.width, header.height)]
    hmax, vmax = header.components[0].h, header.components[0].v
    mx, my = -(-header.width // (8 * hmax)), -(-header.height // (8 * vmax))
    comps = [(c.h, c.v, mx * c.h, my * c.v, -(-header.width * c.h // hmax), -(-header.height * c.v // vmax)) for c in header.components]
    return mx, my, sum(c[0] * c[1] for c in comps), comps


def unstuff(data, header):
    """the scan's restart segments with the FF 00 stuffing removed: (bytes uint8 [n], int64 [n_segments + 1] offsets into them).
    Vectorised: no Python loop over bytes."""
    buf = np.frombuffer(data, dtype=np.uint8, count=header.scan_end - header.scan_start, offset=header.scan_start)
    keep = np.ones(buf.size, dtype=bool)
    prev_ff = np.zeros(buf.size, dtype=bool)
    prev_ff[1:] = buf[:-1] == 0xFF
    keep[prev_ff & (buf == 0)] = False                            # the stuffed zero
    marks = header.rst_offsets - header.scan_start
    keep[marks] = False
    keep[marks + 1] = False
    starts = np.zeros(buf.size, dtype=np.int64)
    starts[marks] = 1
    seg_of = np.cumsum(starts)[keep]                              # segment of every kept byte
    lengths = np.bincount(seg_of, minlength=marks.size + 1).astype(np.int64)
    return buf[keep], np.concatenate([[0], np.cumsum(lengths)])


def device_huffman(counts, symbols):
    """one Huffman table as csrc/jpeg.hip reads it (HUFF_BYTES bytes): uint16 look[512], int32 maxcode[17], int32 valoff[17],
    uint8 symbols[256]"""
    look = np.zeros(512, dtype=np.uint16)
    maxcode = np.full(17, -1, dtype=np.int32)
    valoff = np.zeros(17, dtype=np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        cnt = int(counts[l - 1])
        if cnt:
            valoff[l] = k - code
            if l <= 9:
                for i in range(cnt):
                    lo = (code + i) << (9 - l)
                    look[lo:lo + (1 << (9 - l))] = (l << 8) | int(symbols[k + i])
            code += cnt
            k += cnt
            maxcode[l] = code - 1
        code <<= 1
    val = np.zeros(256, dtype=np.uint8)
    val[:len(symbols)] = symbols
    out = np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), val])
    assert out.size == HUFF_BYTES
    return out


def device_tables(header):
    """(TABLE_BYTES uint8: four quantisation tables then four Huffman tables, {tq: slot}, {(class, id): slot}) of one image"""
    blob = np.zeros(TABLE_BYTES, dtype=np.uint8)
    qslot, hslot = {}, {}
    for c in header.components:
        if c.tq not in qslot:
            qslot[c.tq] = len(qslot)
            blob[128 * qslot[c.tq]:128 * qslot[c.tq] + 128] = header.qtables[c.tq].astype("<u2").view(np.uint8)
        for key in ((0, c.td), (1, c.ta)):
            if key not in hslot:
                if len(hslot) == 4:
                    raise Unsupported("more than four Huffman tables in one scan")
                hslot[key] = len(hslot)
                o = 512 + HUFF_BYTES * hslot[key]
                blob[o:o + HUFF_BYTES] = device_huffman(*header.htables[key])
    return blob, qslot, hslot


_COMPONENT = [(n, np.int32) for n in ("h", "v", "tq", "dc_slot", "ac_slot", "bw", "bh", "blk_off", "plane_off", "cw", "ch")]
IMAGE_DTYPE = np.dtype([("blk_off", np.int64), ("plane_off", np.int64), ("out_off", np.int64), ("table_off", np.int64)] +
                       [(n, np.int32) for n in ("width", "height", "ncomp", "mcus_x", "mcus_y", "blocks_per_mcu", "restart_interval",
                                                "first_wg", "n_wg", "reserved", "reserved2")] +
                       [("comp", np.dtype(_COMPONENT), (3,))])
"""mirror of shdr_jpeg_image (include/shdr.h)"""
assert IMAGE_DTYPE.itemsize == 32 + 44 + 3 * 44


class Batch(ctypes.Structure):
    """mirror of shdr_jpeg_batch"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("data", "tables", "images", "images_dev", "segs", "segs_dev", "sub_seg", "sub_seg_dev",
                                                "passes", "stage_ms")] + \
               [(n, ctypes.c_int64) for n in ("data_bytes", "table_bytes", "n_sub", "n_blocks", "plane_bytes", "out_bytes")] + \
               [(n, ctypes.c_int32) for n in ("n_images", "n_segs", "subseq_bits", "reserved")]


Plan = collections.namedtuple("Plan", "headers data tables images segs sub_seg n_blocks plane_bytes out_bytes subseq_bits")


class _Layout:
    """the O(segments) part of a plan, shared by plan() and plan_device(): from the lengths of an image's unstuffed restart segments
    its rows of `segs`, its subsequence slots and its record of `images`, and the running offsets of the batch"""

    def __init__(self, n_items, subseq_bits):
        self.subseq_bits = int(subseq_bits)
        self.images = np.zeros(n_items, dtype=IMAGE_DTYPE)
        self.headers, self.tabs, self.seg_rows, self.sub_rows = [], [], [], []
        self.dword = self.blk = self.plane = self.out = self.n_sub = self.n_segs = 0

    @staticmethod
    def segments(hd):
        """the restart segments the header implies"""
        mx, my, _, _ = geometry(hd)
        ri = hd.restart_interval
        return -(-mx * my // ri) if ri else 1

    def check(self, item, hd, n_segments, n_bytes):
        """the two checks that follow the unstuffing, with the host route's words"""
        mx, my, _, _ = geometry(hd)
        ri = hd.restart_interval
        want = self.segments(hd)
        if n_segments != want:
            raise CorruptJpeg("%s: %d restart segments, its %d MCUs at restart interval %d make %d" % (
                _name(item), n_segments, mx * my, ri, want))
        if n_bytes >= 1 << 27:
            raise Unsupported("%s: more than 128 MiB of entropy-coded data" % _name(item))

    def add(self, hd, tables, lengths):
        """image len(self.headers) of the batch; tables: device_tables(hd); lengths: int64 per restart segment.  Returns the arena dword
        of every segment (int64) and the dwords the image takes"""
        i = len(self.headers)
        blob, qslot, hslot = tables
        mx, my, bpm, comps = geometry(hd)
        ri = hd.restart_interval
        # every segment starts on a dword of the arena; pad bytes read as 1-bits like libjpeg's, though no decoder sees them
        dwords = (lengths + 3) // 4
        seg_dword = self.dword + np.concatenate([[0], np.cumsum(dwords)[:-1]])
        total = int(dwords.sum())
        self.dword += total
        subs = np.maximum(1, -(-lengths * 8 // self.subseq_bits))
        first_sub = self.n_sub + np.concatenate([[0], np.cumsum(subs)[:-1]])
        per = (ri if ri else mx * my) * bpm
        first_block = np.arange(lengths.size, dtype=np.int64) * per
        rows = np.zeros((lengths.size, 6), dtype=np.int32)
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = seg_dword, lengths * 8, first_sub, first_block
        rows[:, 4], rows[:, 5] = np.minimum(per, mx * my * bpm - first_block), i
        self.seg_rows.append(rows)
        total_subs = int(subs.sum())
        n_wg = -(-total_subs // WG)
        slot = np.full(n_wg * WG, -1, dtype=np.int32)
        slot[:total_subs] = self.n_segs + np.repeat(np.arange(lengths.size), subs)
        self.sub_rows.append(slot)
        self.n_segs += lengths.size
        im = self.images[i]
        im["blk_off"], im["plane_off"], im["out_off"], im["table_off"] = self.blk, self.plane, self.out, TABLE_BYTES * i
        im["width"], im["height"], im["ncomp"], im["mcus_x"], im["mcus_y"] = hd.width, hd.height, len(comps), mx, my
        im["blocks_per_mcu"], im["restart_interval"], im["first_wg"], im["n_wg"] = bpm, ri, self.n_sub // WG, n_wg
        cb = 0
        for c, (h, v, bw, bh, cw, ch) in enumerate(comps):
            k = hd.components[c]
            im["comp"][c] = (h, v, qslot[k.tq], hslot[(0, k.td)], hslot[(1, k.ta)], bw, bh, cb, cb * 64, cw, ch)
            cb += bw * bh
        self.blk += cb
        self.plane += cb * 64
        self.out += hd.width * hd.height * 3
        self.n_sub += n_wg * WG
        self.headers.append(hd)
        self.tabs.append(blob)
        return seg_dword, total

    def plan(self, data):
        return Plan(self.headers, data, np.concatenate(self.tabs), self.images, np.ascontiguousarray(np.concatenate(self.seg_rows)),
                    np.concatenate(self.sub_rows), self.blk, self.plane, self.out, self.subseq_bits)


def plan(items, subseq_bits=SUBSEQ_BITS):
    """parse every item and lay the batch out: the host half of decode().  items: paths or bytes."""
    lay = _Layout(len(items), subseq_bits)
    chunks = []
    for i, item in enumerate(items):
        try:
            raw = _read(item)
            hd = parse(raw)
            tables = device_tables(hd)
        except (Unsupported, CorruptJpeg) as exc:
            raise type(exc)("%s: %s" % (_name(item), exc)) from None
        stream, offs = unstuff(raw, hd)
        lay.check(item, hd, offs.size - 1, stream.size)
        lengths = np.diff(offs)
        dword = lay.dword
        seg_dword, total = lay.add(hd, tables, lengths)
        arena = np.full(total * 4, 0xFF, dtype=np.uint8)
        seg_of = np.repeat(np.arange(lengths.size), lengths)
        arena[(seg_dword[seg_of] - dword) * 4 + np.arange(stream.size) - offs[:-1][seg_of]] = stream
        chunks.append(arena)
    return lay.plan(np.concatenate(chunks))


SCAN_TILE = 4096               # SHDR_JPEG_SCAN_TILE: raw bytes per workgroup of csrc/jpeg_scan.hip
SCAN_PREFIX_TILES = 256        # tiles per workgroup of its cross-tile prefix sum (kScanChunk): a region of more than 1 MiB spans two
SCAN_IMAGE_DTYPE = np.dtype([("offset", np.int64), ("length", np.int64), ("first_tile", np.int64), ("seg_cap", np.int32),
                             ("first_bound", np.int32), ("first_seg", np.int32), ("reserved", np.int32)])
"""mirror of shdr_jpeg_scan_image (include/shdr.h)"""
assert SCAN_IMAGE_DTYPE.itemsize == 40
SCAN_REPORT_DTYPE = np.dtype([("end", np.int64), ("kept", np.int64), ("n_rst", np.int32), ("fill", np.int32), ("end_marker", np.int32),
                              ("reserved", np.int32)])
"""mirror of shdr_jpeg_scan_report"""
assert SCAN_REPORT_DTYPE.itemsize == 32


def scan_images(lengths, seg_caps):
    """SCAN_IMAGE_DTYPE [n] of regions of these lengths laid one after the other, each on a multiple of 16, and the bytes they take"""
    lengths, seg_caps = np.asarray(lengths, dtype=np.int64), np.asarray(seg_caps, dtype=np.int64)
    im = np.zeros(lengths.size, dtype=SCAN_IMAGE_DTYPE)
    padded = (lengths + 15) // 16 * 16
    im["offset"] = np.cumsum(padded) - padded
    im["length"] = lengths
    tiles = -(-lengths // SCAN_TILE)
    im["first_tile"] = np.cumsum(tiles) - tiles
    im["seg_cap"] = seg_caps
    im["first_bound"] = np.cumsum(seg_caps - 1) - (seg_caps - 1)
    im["first_seg"] = np.cumsum(seg_caps) - seg_caps
    return im, int(padded.sum())


def _scan_checks(report):
    """the end of parse(), on the scan call's report of one region: its exceptions and words"""
    if report["end"] < 0:
        raise CorruptJpeg("no EOI marker: the file is cut inside its entropy-coded data")
    m = int(report["end_marker"])
    if m != 0xD9:
        if m in (0xDA, 0xC4, 0xDB, 0xDD):
            raise Unsupported("several scans")
        raise Unsupported("marker FF%02X after the scan" % m)
    if report["fill"]:
        raise Unsupported("fill bytes inside the entropy-coded data")


def _indexed(exc, index):
    exc.index = index                                             # which item of the batch: hdr_real sorts files out of scope with it
    return exc


def plan_device(items, device=None, subseq_bits=SUBSEQ_BITS, timing=None, events=None):
    """plan() with the per-byte work on the device (csrc/jpeg_scan.hip): the host reads the files and walks the markers up to SOS
    (parse_header), the scan regions go up in one copy from a pinned buffer, the scan call finds every region's end, counts its kept
    bytes and restart markers and returns the kept bytes before every marker; the host reads that small report back, makes parse()'s
    and plan()'s checks on it (the same exceptions, naming the same item, with an attribute `index`), lays the segments out as
    plan() does, and the compaction call writes the arena.  The Plan's `data` is that arena, a uint8 device tensor; everything else
    is plan()'s.  Headers have rst_offsets None (nobody located the markers on the host).  timing: a dict that receives the wall
    time in ms of read_parse, stage (into the pinned buffer), scan_launch (upload + launches), scan_wait (the report's readback),
    layout, compact_launch (the table uploads and the launch); events: a dict that receives the device-event time in ms of the scan
    call and of the compaction call (measurement: each call then waits for its last kernel)."""
    import time
    import torch
    try:
        from . import _ops as K
    except ImportError:
        import _ops as K
    t0 = time.perf_counter()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    raws, heads, tables = [], [], []
    deferred = None                                               # the first item the header walk refuses: items after it do not matter
    for i, item in enumerate(items):
        try:
            raw = _read(item)
            hd = parse_header(raw)
        except (Unsupported, CorruptJpeg) as exc:
            deferred = (i, type(exc)("%s: %s" % (_name(item), exc)), False)
            break
        raws.append(raw)
        heads.append(hd)
        try:
            tables.append(device_tables(hd))
        except (Unsupported, CorruptJpeg) as exc:                 # (the host route looks at the scan before it looks at the tables)
            deferred = (i, type(exc)("%s: %s" % (_name(item), exc)), True)
            break
    if not raws:
        raise _indexed(deferred[1], deferred[0]) from None
    t1 = time.perf_counter()
    caps = [_Layout.segments(hd) for hd in heads]
    desc, total = scan_images([len(r) - hd.scan_start for r, hd in zip(raws, heads)], caps)
    if total >= 1 << 33:
        raise Unsupported("more than 8 GiB of files in one batch")
    staging = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    for r, hd, d in zip(raws, heads, desc):
        host[d["offset"]:d["offset"] + d["length"]] = np.frombuffer(r, dtype=np.uint8, count=int(d["length"]), offset=hd.scan_start)
    t2 = time.perf_counter()
    with torch.cuda.device(dev):
        src = staging.to(dev, non_blocking=True)
        scan_ms, compact_ms = ([], []) if events is not None else (None, None)
        result, ws, desc_dev = K.jpeg_scan(src, desc, stage_ms=scan_ms)
        t3 = time.perf_counter()
        back = result.cpu().numpy()                               # the one readback: a few words per image, one per restart marker
    t4 = time.perf_counter()
    n = len(raws)
    report = back[:n * SCAN_REPORT_DTYPE.itemsize].view(SCAN_REPORT_DTYPE)
    bounds = back[n * SCAN_REPORT_DTYPE.itemsize:].view(np.int64)
    lay = _Layout(n, subseq_bits)
    for i, (item, hd, rep, d) in enumerate(zip(items, heads, report, desc)):
        try:
            _scan_checks(rep)
        except (Unsupported, CorruptJpeg) as exc:
            raise _indexed(type(exc)("%s: %s" % (_name(item), exc)), i) from None
        if deferred is not None and deferred[0] == i:
            raise _indexed(deferred[1], i) from None
        try:
            lay.check(item, hd, int(rep["n_rst"]) + 1, int(rep["kept"]))
        except (Unsupported, CorruptJpeg) as exc:
            raise _indexed(exc, i) from None
        b = bounds[d["first_bound"]:d["first_bound"] + d["seg_cap"] - 1]
        lengths = np.diff(np.concatenate([[0], b, [rep["kept"]]])).astype(np.int64)
        lay.add(Header(hd.width, hd.height, hd.components, hd.layout, hd.qtables, hd.htables, hd.restart_interval, hd.scan_start,
                       hd.scan_start + int(rep["end"]), None, hd.orientation), tables[i], lengths)
    if deferred is not None:
        raise _indexed(deferred[1], deferred[0]) from None
    p = lay.plan(None)
    t5 = time.perf_counter()
    with torch.cuda.device(dev):
        segs_dev = torch.from_numpy(p.segs.reshape(-1)).to(dev)
        arena = K.jpeg_compact(src, desc, desc_dev, result, ws, segs_dev, p.segs.shape[1], lay.dword * 4, stage_ms=compact_ms)
    t6 = time.perf_counter()
    if timing is not None:
        timing.update(read_parse=(t1 - t0) * 1e3, stage=(t2 - t1) * 1e3, scan_launch=(t3 - t2) * 1e3, scan_wait=(t4 - t3) * 1e3,
                      layout=(t5 - t4) * 1e3, compact_launch=(t6 - t5) * 1e3)
    if events is not None:
        events.update(scan=scan_ms[0], compact=compact_ms[0], raw_bytes=total, arena_bytes=lay.dword * 4)
    return p._replace(data=arena)


STAGE_NAMES = ("clear", "sync_passes", "scan_write", "dc", "idct", "finish")       # SHDR_JPEG_STAGES of shdr_jpeg_batch.stage_ms


def check_unstuff_option(what, unstuff):
    if unstuff not in ("host", "device"):
        raise ValueError("%s: unstuff must be 'host' or 'device', got %r" % (what, unstuff))
    return unstuff


class Decoded:
    """what one batch call left on the device (decode() / decode_coefficients() wrap it).  host_ms: wall time of the host half
    (read + parse + unstuff + lay out, then the uploads); stages=True also fills stage_ms, the device-event time of every stage
    of the library call (STAGE_NAMES), at the price of waiting for the call's last kernel.
    unstuff: who finds the end of the scan, removes the stuffing and fills the segment arena -- "host" (plan: NumPy) or "device"
    (plan_device: csrc/jpeg_scan.hip; the same arena, the same exceptions).  host_ms then names the parts of that route: read_parse,
    stage, scan_launch, scan_wait (the host waits for the scan's report), layout, compact_launch, and upload (the other tables);
    stages=True also fills scan_ms: the device-event times "scan" and "compact" of the two calls, and the bytes they moved."""

    def __init__(self, items, device=None, pixels=True, subseq_bits=SUBSEQ_BITS, out=None, stages=False, unstuff="host"):
        import time
        import torch
        lib = _lib.load()
        check_unstuff_option("jpeg.decode", unstuff)
        self.items = list(items)
        if not self.items:
            raise ValueError("jpeg.decode: no items")
        device_of = lambda: torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        up = lambda a: torch.from_numpy(a).to(dev)
        t0 = time.perf_counter()
        if unstuff == "device":
            self.device = dev = device_of()
            self.host_ms = {}
            self.scan_ms = {} if stages else None
            self.plan = p = plan_device(self.items, dev, subseq_bits, timing=self.host_ms, events=self.scan_ms)
            t1 = time.perf_counter()
            self._keep = (p.data, up(p.tables), up(p.images.view(np.uint8)), up(p.segs.reshape(-1)), up(p.sub_seg))
            self.host_ms["upload"] = (time.perf_counter() - t1) * 1e3
        else:
            self.plan = p = plan(self.items, subseq_bits)
            t1 = time.perf_counter()
            self.device = dev = device_of()
            self._keep = (up(p.data), up(p.tables), up(p.images.view(np.uint8)), up(p.segs.reshape(-1)), up(p.sub_seg))
            self.host_ms = {"plan": (t1 - t0) * 1e3, "upload": (time.perf_counter() - t1) * 1e3}
        data, tables, images, segs, sub_seg = self._keep
        n_sub = p.sub_seg.size
        ws_bytes = lib.shdr_jpeg_workspace_bytes(n_sub, p.n_blocks, p.plane_bytes)
        if ws_bytes < 0:
            raise RuntimeError(lib.shdr_last_error().decode())
        self.workspace = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        self.coef = torch.empty((p.n_blocks, 64), device=dev, dtype=torch.int16)
        self.errors = torch.empty(len(self.items), device=dev, dtype=torch.int32)
        if out is not None and (out.dtype != torch.uint8 or out.numel() != p.out_bytes or not out.is_contiguous() or out.device != dev):
            raise ValueError("jpeg.decode: `out` must be a contiguous uint8 device tensor of %d elements" % p.out_bytes)
        self.out = (out if out is not None else torch.empty(p.out_bytes, device=dev, dtype=torch.uint8)) if pixels else None
        self._passes = ctypes.c_int32(0)
        stage_ms = (ctypes.c_float * len(STAGE_NAMES))()
        b = Batch(data.data_ptr(), tables.data_ptr(), p.images.ctypes.data, images.data_ptr(), p.segs.ctypes.data, segs.data_ptr(),
                  p.sub_seg.ctypes.data, sub_seg.data_ptr(), ctypes.addressof(self._passes),
                  ctypes.addressof(stage_ms) if stages else None, data.numel(), p.tables.size, n_sub,
                  p.n_blocks, p.plane_bytes, p.out_bytes, len(self.items), p.segs.shape[0], p.subseq_bits, 0)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            if pixels:
                rc = lib.shdr_jpeg_decode_u8(ctypes.byref(b), self.coef.data_ptr(), self.out.data_ptr(), self.errors.data_ptr(),
                                             self.workspace.data_ptr(), stream)
            else:
                rc = lib.shdr_jpeg_entropy_decode(ctypes.byref(b), self.coef.data_ptr(), self.errors.data_ptr(),
                                                  self.workspace.data_ptr(), stream)
        _lib.check(rc, "shdr_jpeg_decode_u8" if pixels else "shdr_jpeg_entropy_decode")
        self.passes = self._passes.value
        self.stage_ms = dict(zip(STAGE_NAMES, stage_ms)) if stages else None

    def check(self):
        """CorruptJpeg naming the first item whose entropy-coded data the device found damaged"""
        err = self.errors.cpu().numpy()
        for i in np.flatnonzero(err):
            raise CorruptJpeg("%s: %s" % (_name(self.items[i]), DEVICE_ERRORS.get(int(err[i]), "error %d" % err[i])))

    def image(self, i):
        im = self.plan.images[i]
        h, w, o = int(im["height"]), int(im["width"]), int(im["out_off"])
        return self.out[o:o + h * w * 3].view(h, w, 3)

    def coefficients(self, i):
        """per component int16 [bh, bw, 64] (views of the arena)"""
        im = self.plan.images[i]
        res = []
        for c in range(int(im["ncomp"])):
            k = im["comp"][c]
            o = int(im["blk_off"]) + int(k["blk_off"])
            res.append(self.coef[o:o + int(k["bw"]) * int(k["bh"])].view(int(k["bh"]), int(k["bw"]), 64))
        return res

    def sync_rounds(self):
        """per subsequence the round in which its end state last changed (shdr_jpeg_sync_rounds); -1 for unused slots"""
        import torch
        p = self.plan
        rounds = np.zeros(p.sub_seg.size, dtype=np.int32)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().shdr_jpeg_sync_rounds(self.workspace.data_ptr(), p.sub_seg.size, p.n_blocks, p.plane_bytes,
                                                     rounds.ctypes.data, stream), "shdr_jpeg_sync_rounds")
        rounds[p.sub_seg < 0] = -1
        return rounds


def apply_orientation(img, orientation):
    """the EXIF Orientation applied to [H, W, 3] (a tensor, host or device), as PIL.ImageOps.exif_transpose does; pure data movement"""
    o = int(orientation)
    if o == 2:
        img = img.flip(1)
    elif o == 3:
        img = img.flip(0, 1)
    elif o == 4:
        img = img.flip(0)
    elif o == 5:
        img = img.transpose(0, 1)
    elif o == 6:
        img = img.transpose(0, 1).flip(1)
    elif o == 7:
        img = img.transpose(0, 1).flip(0, 1)
    elif o == 8:
        img = img.transpose(0, 1).flip(0)
    return img.contiguous()


def decode(items, device=None, subseq_bits=SUBSEQ_BITS, orient=True, unstuff="host"):
    """paths or bytes -> one uint8 RGB [H, W, 3] device tensor per item, from ONE batch call; byte for byte PIL's
    Image.open(f).convert("RGB") (orient=True: with the EXIF Orientation applied, as hdr_io.read_ldr).  Unsupported / CorruptJpeg
    name the offending item.  unstuff="device" prepares the scan on the device too (Decoded): the same pixels."""
    d = Decoded(items, device, True, subseq_bits, unstuff=unstuff)
    d.check()
    res = []
    for i, hd in enumerate(d.plan.headers):
        img = d.image(i)
        res.append(apply_orientation(img, hd.orientation) if orient and hd.orientation != 1 else img)
    return res


def decode_coefficients(item, device=None, subseq_bits=SUBSEQ_BITS, unstuff="host"):
    """one file -> per component the quantised coefficients int16 [bh, bw, 64] on the device (natural order, DC prediction undone,
    the padded block grid): for tests and debugging"""
    d = Decoded([item], device, False, subseq_bits, unstuff=unstuff)
    d.check()
    return d.coefficients(0)


def read_ldr_device(path, device=None, unstuff="host"):
    """hdr_io.read_ldr(path) as a uint8 device tensor: decoded on the device when the file is in scope, by PIL and uploaded when it is
    not (Unsupported: progressive, CMYK, ..., or no JPEG at all).  CorruptJpeg propagates.  unstuff: as decode()."""
    import torch
    check_unstuff_option("jpeg.read_ldr_device", unstuff)
    try:
        return decode([path], device, unstuff=unstuff)[0]
    except Unsupported:
        pass
    try:
        from . import hdr_io
    except ImportError:
        import hdr_io
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(hdr_io.read_ldr(path)).to(dev)


# ---------------------------------------------------------------- the writer (csrc/jpeg_enc.hip, csrc/jpeg_enc.h)
ENCODE_OPTIONS = ("quality", "subsampling", "restart_interval", "encoder")
_ENCODE_BUFFERS = {}           # (thread, device, stream) -> encode()'s output and workspace, kept from call to call: encode() has copied
                               # the files to the host before it returns, and both are sized for the worst case


def _ops():
    try:
        from . import _ops as K
    except ImportError:
        import _ops as K
    return K


def _check_encode_options(what, options):
    """the writer's scope: 8-bit RGB, the standard Huffman tables, sequential; what PIL would take beyond that is refused by name"""
    refused = {"optimize": "optimised Huffman tables", "progressive": "progressive coding", "progression": "progressive coding",
               "arithmetic": "arithmetic coding", "exif": "EXIF segments", "icc_profile": "ICC segments", "comment": "comment segments",
               "qtables": "custom quantisation tables", "dpi": "a density other than 1:1"}
    for key in options:
        if key in refused:
            raise ValueError("%s: %s are outside the writer's scope (option %r)" % (what, refused[key], key))
        if key not in ENCODE_OPTIONS:
            raise ValueError("%s: unknown option %r (known: %s)" % (what, key, ", ".join(ENCODE_OPTIONS)))


def encode(images, quality=75, subsampling="420", restart_interval=0, encoder="device", stage_ms=None):
    """8-bit RGB images -> baseline-JPEG files (a list of bytes), byte for byte what PIL writes with
    Image.save(f, "JPEG", quality=quality, subsampling=subsampling[, restart_marker_blocks=restart_interval]).
    images: a list of uint8 [H, W, 3] device tensors of any sizes, or one [N, H, W, 3] tensor (float32 in [0, 1] is taken too and
    quantised as the camera simulator does); with encoder="host" host arrays, coded by libshdr's host twin.  quality: 1 .. 100, one
    value or one per image; subsampling: "444" | "422" | "420"; restart_interval: MCUs per restart segment, 0 .. 65535.
    encoder="device": ONE batch call (csrc/jpeg_enc.hip) and one copy of the finished files to the host.  Grey and CMYK images,
    optimised Huffman tables, progressive and arithmetic coding, EXIF / ICC / comment segments and 4:4:0 raise ValueError."""
    K = _ops()
    if encoder not in ("device", "host"):
        raise ValueError("jpeg.encode: encoder must be 'device' or 'host', got %r" % (encoder,))
    if encoder == "host":
        arrays = [np.asarray(a) for a in (images if isinstance(images, (list, tuple)) else (images if np.ndim(images) == 4 else [images]))]
        for a in arrays:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("jpeg.encode: expected uint8 RGB images [H, W, 3] (grey and CMYK are outside the writer's scope), got %s %s"
                                 % (a.dtype, a.shape))
        desc = K.jpeg_enc_images([a.shape[:2] for a in arrays], quality, subsampling, restart_interval)
        return [K.jpeg_encode_host(a, desc[i:i + 1]) for i, a in enumerate(arrays)]
    import torch
    tensors = images if isinstance(images, (list, tuple)) else [images]
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.shape[-1:] != (3,) or t.dim() not in (3, 4):
            raise ValueError("jpeg.encode: expected RGB device tensors [H, W, 3] or [N, H, W, 3] (grey and CMYK are outside the writer's "
                             "scope), got %s" % (tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__,))
    if isinstance(images, (list, tuple)):
        shapes = [tuple(t.shape[:2]) for t in images]
    else:
        shapes = [tuple(images.shape[-3:-1])] * (1 if images.dim() == 3 else images.shape[0])
    desc = K.jpeg_enc_images(shapes, quality, subsampling, restart_interval)
    import threading
    first = images[0] if isinstance(images, (list, tuple)) else images
    key = (threading.get_ident(), first.device, torch.cuda.current_stream(first.device).cuda_stream)
    out, offsets, status = K.jpeg_encode(images, desc, stage_ms=stage_ms, buffers=_ENCODE_BUFFERS.setdefault(key, {}))
    # the offsets and status words first (8 (n + 1) + 4 n bytes), then ONE copy of exactly the bytes written
    off = offsets.cpu().numpy()
    bad = np.flatnonzero(status.cpu().numpy())
    if bad.size:
        raise ValueError("jpeg.encode: image %d holds a coefficient outside the baseline range" % int(bad[0]))
    data = out[:int(off[-1])].cpu().numpy()
    return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(shapes))]


def write_jpeg(path, image, **options):
    """one image [H, W, 3] -> a baseline-JPEG file at `path`; options: encode()'s (quality, subsampling, restart_interval, encoder)"""
    _check_encode_options("jpeg.write_jpeg", options)
    if getattr(image, "ndim", 0) != 3:
        raise ValueError("jpeg.write_jpeg: expected one image [H, W, 3], got %s" % (tuple(getattr(image, "shape", ())),))
    data = encode([image], **options)[0]
    with open(path, "wb") as f:
        f.write(data)
