"""Gain-map JPEG files (Google's Ultra HDR v1 container with Adobe's hdrgm metadata): one ordinary SDR JPEG that every viewer shows,
with a second JPEG behind it that holds a per-pixel log2 gain; a viewer that knows the format multiplies the two and shows HDR.

    files = ultrahdr.encode([hdr_a, hdr_b], [sdr_a, sdr_b])          # float32 / uint8 device tensors [H, W, 3] -> a list of bytes
    files = ultrahdr.encode([hdr], [sdr], base=[open("photo.jpg", "rb").read()])     # the photograph itself stays the primary image
    hdrs = ultrahdr.decode(files, display_boost=4.0)                 # float32 [H, W, 3] device tensors
    ultrahdr.write("scene.jpg", hdr, sdr); hdr = ultrahdr.read("scene.jpg")

The arithmetic -- sRGB linearisation, exposure alignment, box average per map cell, log2, range, quantisation, and the way back -- runs
on the device (K.gainmap_encode: three launches for the whole list; K.gainmap_apply: one), by the rules of csrc/gainmap.h, which the
host twins share bit for bit.  Both JPEG streams are coded by jpeg.encode (the gain map as a three-channel 4:4:4 baseline file: grey
output is outside that writer's scope) and decoded by jpeg.decode.  The container is assembled and taken apart here, on bytes only.

PINNING.  There is no libultrahdr, Skia or Android decoder where this was written, and the format rules are restated from memory of
the Ultra HDR v1 / Adobe gain-map specifications.  NO FOREIGN ULTRA HDR READER HAS OPENED THESE FILES.  Pinned are: both JPEG streams
(Pillow decodes them), the MPF index (Pillow's MPO plugin opens every file with two frames and finds the second at the recorded
offset), the XMP packets (xml.etree parses them) and the arithmetic (a float64 NumPy restatement, tests/gainmap_ref.py).

CONTAINER.  Gain-map file: SOI, APP0, then an APP1 with the XMP packet (hdrgm:Version, GainMapMin, GainMapMax, Gamma, OffsetSDR,
OffsetHDR, HDRCapacityMin, HDRCapacityMax, BaseRenditionIsHDR; log2 values, printed so that they read back to the last bit).  Primary
file: SOI, its leading APP0 / Exif APP1 segments, then an XMP APP1 (hdrgm:Version and a Container:Directory of two Container:Item
entries, the second with the gain-map file's length), then an MPF APP2 (big-endian TIFF header, one IFD with the version 0100, the
image count 2 and two 16-byte MP entries: attribute, size, offset relative to the TIFF header, two zero dependents), then the rest of
the file unaltered, then the gain-map file.
"""
import math
import struct
import xml.etree.ElementTree as ET

import numpy as np

XMP_HEADER = b"http://ns.adobe.com/xap/1.0/\0"
MPF_HEADER = b"MPF\0"
NS_HDRGM = "http://ns.adobe.com/hdr-gain-map/1.0/"
NS_CONTAINER = "http://ns.google.com/photos/1.0/container/"
NS_ITEM = "http://ns.google.com/photos/1.0/container/item/"
NS_RDF = "http://www.w3.org/1999/02/22-rdf-syntax-ns#"
MP_PRIMARY = 0x20030000                # representative image, baseline MP primary image, JPEG
METADATA_FIELDS = ("GainMapMin", "GainMapMax", "Gamma", "OffsetSDR", "OffsetHDR", "HDRCapacityMin", "HDRCapacityMax")
METADATA_DEFAULTS = dict(GainMapMin=0.0, Gamma=1.0, OffsetSDR=0.015625, OffsetHDR=0.015625, HDRCapacityMin=0.0)
MIN_CAPACITY = 2.0 ** -10
ENCODE_OPTIONS = ("factor", "hdr_scale", "log2_range", "base", "base_options", "map_quality", "reverse_channels", "encoder")


def _mods():
    try:
        from . import _ops as K
        from . import jpeg
    except ImportError:
        import _ops as K
        import jpeg
    return K, jpeg


# ---------------------------------------------------------------- bytes: segments, XMP, MPF
def _segments(data, what):
    """[(marker, start, end)] of the segments between SOI and SOS: data[start:end] is FF, the marker, the length and the payload.
    ValueError with the reason for anything else than a marker walk that reaches SOS"""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("%s: not a JPEG file (no SOI)" % what)
    pos, segs = 2, []
    while True:
        if pos + 4 > len(data):
            raise ValueError("%s: the file ends inside its header (at byte %d)" % (what, pos))
        if data[pos] != 0xFF:
            raise ValueError("%s: no marker at byte %d" % (what, pos))
        marker = data[pos + 1]
        if marker == 0xFF:                                          # a fill byte
            pos += 1
            continue
        if marker in (0xD8, 0xD9, 0x01) or 0xD0 <= marker <= 0xD7:
            raise ValueError("%s: marker FF%02X in the header (at byte %d)" % (what, marker, pos))
        length = struct.unpack_from(">H", data, pos + 2)[0]
        if length < 2 or pos + 2 + length > len(data):
            raise ValueError("%s: segment FF%02X at byte %d runs past the end of the file" % (what, marker, pos))
        segs.append((marker, pos, pos + 2 + length))
        if marker == 0xDA:
            return segs
        pos += 2 + length


def _payload(data, seg):
    return data[seg[1] + 4:seg[2]]


def _frame_size(data, segs, what):
    for seg in segs:
        if 0xC0 <= seg[0] <= 0xCF and seg[0] not in (0xC4, 0xC8, 0xCC):
            p = _payload(data, seg)
            if len(p) < 6:
                break
            return struct.unpack_from(">HH", p, 1)
    raise ValueError("%s: no frame header" % what)


def _xmp(data, segs):
    """the XMP packets (bytes) of the header's APP1 segments"""
    return [_payload(data, s)[len(XMP_HEADER):] for s in segs if s[0] == 0xE1 and _payload(data, s).startswith(XMP_HEADER)]


def _app(marker, payload):
    if len(payload) + 2 > 65535:
        raise ValueError("ultrahdr: a segment of %d bytes does not fit" % len(payload))
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


# Every attribute of a packet stands on a line of its own, with no blank in front of it.  Pillow (11 and later) hands a file back as a
# plain JPEG, not as a two-frame MPO, when an APP1 of the primary image holds the bytes ' hdrgm:Version="' with the blank; the tests
# pin the MPF index through Pillow's MPO plugin, and an XML reader sees the same attributes either way.
def _num(v):
    """a float so that float(text) gives it back to the last bit"""
    return repr(float(v))


def gainmap_xmp(meta):
    """the XMP packet (bytes) of a gain-map file; meta: a dict with METADATA_FIELDS (log2 values) and BaseRenditionIsHDR"""
    fields = "".join('\nhdrgm:%s="%s"' % (k, _num(meta[k])) for k in METADATA_FIELDS)
    return ('<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="%s"><rdf:Description rdf:about=""\nxmlns:hdrgm="%s"\n'
            'hdrgm:Version="1.0"%s\nhdrgm:BaseRenditionIsHDR="%s"/></rdf:RDF></x:xmpmeta>'
            % (NS_RDF, NS_HDRGM, fields, "True" if meta.get("BaseRenditionIsHDR") else "False")).encode("utf-8")


def primary_xmp(gainmap_length):
    """the XMP packet (bytes) of a primary file whose gain-map file has `gainmap_length` bytes"""
    return ('<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="%s"><rdf:Description rdf:about=""\nxmlns:Container="%s"\n'
            'xmlns:Item="%s"\nxmlns:hdrgm="%s"\nhdrgm:Version="1.0"><Container:Directory><rdf:Seq>'
            '<rdf:li rdf:parseType="Resource"><Container:Item Item:Semantic="Primary" Item:Mime="image/jpeg"/></rdf:li>'
            '<rdf:li rdf:parseType="Resource"><Container:Item Item:Semantic="GainMap" Item:Mime="image/jpeg" Item:Length="%d"/></rdf:li>'
            '</rdf:Seq></Container:Directory></rdf:Description></rdf:RDF></x:xmpmeta>'
            % (NS_RDF, NS_CONTAINER, NS_ITEM, NS_HDRGM, int(gainmap_length))).encode("utf-8")


def mpf_payload(primary_size, gainmap_size, gainmap_offset):
    """the payload of the MPF APP2: sizes in bytes, the offset of the gain-map file relative to the first byte of the TIFF header"""
    ifd = struct.pack(">H", 3)
    ifd += struct.pack(">HHI4s", 0xB000, 7, 4, b"0100")
    ifd += struct.pack(">HHII", 0xB001, 4, 1, 2)
    ifd += struct.pack(">HHII", 0xB002, 7, 32, 8 + 2 + 36 + 4)
    ifd += struct.pack(">I", 0)
    entries = struct.pack(">IIIHH", MP_PRIMARY, primary_size, 0, 0, 0) + struct.pack(">IIIHH", 0, gainmap_size, gainmap_offset, 0, 0)
    return MPF_HEADER + b"MM\0*" + struct.pack(">I", 8) + ifd + entries


def _insert_at(data, segs):
    """the byte behind SOI and the leading APP0 / Exif APP1 segments"""
    pos = 2
    for marker, start, end in segs:
        if start == pos and (marker == 0xE0 or (marker == 0xE1 and data[start + 4:start + 10] == b"Exif\0\0")):
            pos = end
        else:
            break
    return pos


def gainmap_file(jpeg_bytes, meta):
    """a gain-map JPEG with its XMP APP1 directly behind SOI and APP0"""
    segs = _segments(jpeg_bytes, "ultrahdr: the gain-map JPEG")
    pos = 2
    if segs and segs[0][0] == 0xE0:
        pos = segs[0][2]
    return jpeg_bytes[:pos] + _app(0xE1, XMP_HEADER + gainmap_xmp(meta)) + jpeg_bytes[pos:]


def check_base(data, shape, what="ultrahdr.encode: base"):
    """a base JPEG must not be a gain-map file already and must hold shape[0] x shape[1] pixels"""
    segs = _segments(data, what)
    for seg in segs:
        if seg[0] == 0xE2 and _payload(data, seg).startswith(MPF_HEADER):
            raise ValueError("%s already holds an MPF APP2 segment (a multi-picture file)" % what)
    for packet in _xmp(data, segs):
        if b"hdrgm" in packet or NS_HDRGM.encode() in packet:
            raise ValueError("%s already holds an hdrgm XMP packet (a gain-map file)" % what)
    h, w = _frame_size(data, segs, what)
    if (h, w) != (int(shape[0]), int(shape[1])):
        raise ValueError("%s is %d x %d, the HDR image %d x %d" % (what, h, w, shape[0], shape[1]))
    return segs


def assemble(primary_jpeg, gainmap_jpeg, meta):
    """the container: primary_jpeg (its coded data unaltered) with the XMP and MPF segments inserted, then the gain-map file"""
    gm = gainmap_file(gainmap_jpeg, meta)
    segs = _segments(primary_jpeg, "ultrahdr: the primary JPEG")
    pos = _insert_at(primary_jpeg, segs)
    xmp = _app(0xE1, XMP_HEADER + primary_xmp(len(gm)))
    mpf_len = len(_app(0xE2, mpf_payload(0, 0, 0)))
    primary_size = len(primary_jpeg) + len(xmp) + mpf_len
    tiff_at = pos + len(xmp) + 4 + len(MPF_HEADER)
    if primary_size + len(gm) >= 1 << 32:
        raise ValueError("ultrahdr: a file of %d bytes does not fit the MPF index" % (primary_size + len(gm)))
    mpf = _app(0xE2, mpf_payload(primary_size, len(gm), primary_size - tiff_at))
    return primary_jpeg[:pos] + xmp + mpf + primary_jpeg[pos:] + gm


def metadata_of(record):
    """the hdrgm fields of one K.GAINMAP_META_DTYPE record (rule 6 of csrc/gainmap.h): Python floats that hold fp32 values"""
    gmax = float(record["gain_max"])
    return dict(GainMapMin=float(record["gain_min"]), GainMapMax=gmax, Gamma=1.0, OffsetSDR=0.015625, OffsetHDR=0.015625,
                HDRCapacityMin=0.0, HDRCapacityMax=max(gmax, MIN_CAPACITY), BaseRenditionIsHDR=False)


def parse_gainmap_xmp(packet, what="ultrahdr"):
    """the metadata dict of a gain-map file's XMP packet; one scalar per field (per-channel sequences are refused by name)"""
    try:
        root = ET.fromstring(packet)
    except ET.ParseError as exc:
        raise ValueError("%s: the gain-map XMP packet does not parse: %s" % (what, exc)) from None
    for desc in root.iter("{%s}Description" % NS_RDF):
        if desc.get("{%s}Version" % NS_HDRGM) is None:
            continue
        meta = dict(METADATA_DEFAULTS, Version=desc.get("{%s}Version" % NS_HDRGM))
        for key in METADATA_FIELDS:
            text = desc.get("{%s}%s" % (NS_HDRGM, key))
            if text is None:
                if desc.find("{%s}%s" % (NS_HDRGM, key)) is not None:
                    raise ValueError("%s: hdrgm:%s is a per-channel sequence, which this reader does not take" % (what, key))
                if key not in meta:
                    raise ValueError("%s: the gain-map XMP packet has no hdrgm:%s" % (what, key))
                continue
            try:
                meta[key] = float(text)
            except ValueError:
                raise ValueError("%s: hdrgm:%s is %r, not a number" % (what, key, text)) from None
        meta["BaseRenditionIsHDR"] = desc.get("{%s}BaseRenditionIsHDR" % NS_HDRGM, "False").strip().lower() == "true"
        return meta
    raise ValueError("%s: the gain-map XMP packet has no hdrgm:Version" % what)


def _item_lengths(packet, what):
    """[(semantic, length or None)] of the Container:Item entries of a primary XMP packet"""
    try:
        root = ET.fromstring(packet)
    except ET.ParseError as exc:
        raise ValueError("%s: the primary XMP packet does not parse: %s" % (what, exc)) from None
    items = []
    for it in root.iter("{%s}Item" % NS_CONTAINER):
        length = it.get("{%s}Length" % NS_ITEM)
        items.append((it.get("{%s}Semantic" % NS_ITEM), None if length is None else int(length)))
    return items


def split(data):
    """a gain-map JPEG file -> (primary bytes, gain-map file bytes, metadata dict).  Walks markers only (no pixel is decoded), reads
    the MPF index and cross-checks it against Item:Length and the file's size; ValueError with the reason for anything malformed."""
    data = bytes(data)
    what = "ultrahdr.split"
    segs = _segments(data, what)
    mpf = [s for s in segs if s[0] == 0xE2 and _payload(data, s).startswith(MPF_HEADER)]
    if not mpf:
        raise ValueError("%s: no MPF APP2 segment: not a gain-map file" % what)
    tiff_at = mpf[0][1] + 4 + len(MPF_HEADER)
    tiff = data[tiff_at:mpf[0][2]]
    if len(tiff) < 8 or tiff[:2] not in (b"MM", b"II"):
        raise ValueError("%s: the MPF segment has no TIFF header" % what)
    e = ">" if tiff[:2] == b"MM" else "<"
    magic, ifd = struct.unpack_from(e + "HI", tiff, 2)
    if magic != 42 or ifd + 2 > len(tiff):
        raise ValueError("%s: the MPF TIFF header is damaged" % what)
    count, = struct.unpack_from(e + "H", tiff, ifd)
    n_images = entries_at = None
    for i in range(count):
        o = ifd + 2 + 12 * i
        if o + 12 > len(tiff):
            raise ValueError("%s: the MPF index is truncated" % what)
        tag, typ, cnt, value = struct.unpack_from(e + "HHII", tiff, o)
        if tag == 0xB001:
            n_images = value
        elif tag == 0xB002:
            entries_at, entries_len = value, cnt
    if n_images is None or entries_at is None:
        raise ValueError("%s: the MPF index lacks the image count or the MP entries" % what)
    if n_images != 2 or entries_len != 32 or entries_at + 32 > len(tiff):
        raise ValueError("%s: the MPF index lists %d images in %d bytes of entries (a gain-map file has 2 in 32)" % (what, n_images, entries_len))
    _, size0, off0, _, _ = struct.unpack_from(e + "IIIHH", tiff, entries_at)
    _, size1, off1, _, _ = struct.unpack_from(e + "IIIHH", tiff, entries_at + 16)
    start = tiff_at + off1
    if off0 != 0 or off1 == 0 or start + size1 > len(data) or size0 > start:
        raise ValueError("%s: the MPF index points outside the file (primary %d bytes; second picture %d bytes at byte %d of %d)"
                         % (what, size0, size1, start, len(data)))
    gm = data[start:start + size1]
    if gm[:2] != b"\xff\xd8" or gm[-2:] != b"\xff\xd9":
        raise ValueError("%s: the bytes the MPF index points to are no JPEG file" % what)
    packets = [p for p in _xmp(data, segs) if NS_CONTAINER.encode() in p]
    if not packets:
        raise ValueError("%s: the primary image has no Container:Directory XMP packet" % what)
    lengths = [length for semantic, length in _item_lengths(packets[0], what) if semantic == "GainMap"]
    if lengths != [size1]:
        raise ValueError("%s: Item:Length %s and the MPF size %d disagree" % (what, lengths, size1))
    gm_packets = _xmp(gm, _segments(gm, what + ": the gain-map file"))
    if not gm_packets:
        raise ValueError("%s: the gain-map file has no XMP packet" % what)
    return data[:size0], gm, parse_gainmap_xmp(gm_packets[0], what)


# ---------------------------------------------------------------- pixels
def _scales(hdr_scale, n):
    if isinstance(hdr_scale, str):
        if hdr_scale != "auto":
            raise ValueError("ultrahdr.encode: hdr_scale must be 'auto' or a positive number, got %r" % (hdr_scale,))
        return None
    values = np.asarray(hdr_scale, dtype=np.float64).reshape(-1)
    if values.size == 1:
        values = np.repeat(values, n)
    if values.size != n or not (np.isfinite(values).all() and (values > 0).all()):
        raise ValueError("ultrahdr.encode: hdr_scale must be 'auto', one positive number or one per image, got %r" % (hdr_scale,))
    return values.astype(np.float32)


def encode(hdrs, sdrs, factor=4, hdr_scale="auto", log2_range=(-4.0, 8.0), base=None, base_options=None, map_quality=85,
           reverse_channels=False, encoder="device"):
    """HDR images and their SDR renditions -> gain-map JPEG files (a list of bytes).
    hdrs: float32 [H, W, 3] linear images, sdrs: uint8 [H, W, 3] sRGB images of the same sizes -- lists of device tensors, or with
    encoder="host" of host arrays (libshdr's host twins and jpeg.encode(encoder="host"): the same bytes).  reverse_channels: channel 0
    of the HDR images is blue (what HdrReconstructor.reconstruct_device returns).  factor: 1, 2, 4 or 8 image pixels per map cell and
    axis.  hdr_scale: "auto" aligns the exposure of every HDR image to its SDR image (include/shdr.h), a number (or one per image)
    fixes the scale.  log2_range: the clamp of the log2 gain.  base=None codes the SDR images with jpeg.encode(**base_options) (PIL's
    defaults: quality 75, 4:2:0), in ONE call for the whole list, and decodes them again in one call: the gains are taken against the
    pixels that a viewer of the primary image sees, so that SDR times gain is the HDR image whatever the quality; base=[bytes, ...] takes these JPEG files as the primary images with
    their coded data unaltered -- for the photograph an estimate was made from; sdrs are then their decoded pixels (a None in the list:
    that image's primary is coded like the others without a base, all of them in one call).  All gain maps
    go through ONE jpeg.encode(quality=map_quality, subsampling="444") call."""
    K, jpeg = _mods()
    if encoder not in ("device", "host"):
        raise ValueError("ultrahdr.encode: encoder must be 'device' or 'host', got %r" % (encoder,))
    hdrs, sdrs = list(hdrs), list(sdrs)
    n = len(hdrs)
    if n == 0 or len(sdrs) != n:
        raise ValueError("ultrahdr.encode: %d HDR images and %d SDR images" % (n, len(sdrs)))
    shapes = []
    for i, (h, s) in enumerate(zip(hdrs, sdrs)):
        if len(h.shape) != 3 or h.shape[2] != 3 or tuple(s.shape) != tuple(h.shape):
            raise ValueError("ultrahdr.encode: image %d: expected HDR and SDR [H, W, 3] of one size, got %s and %s"
                             % (i, tuple(h.shape), tuple(s.shape)))
        shapes.append((int(h.shape[0]), int(h.shape[1])))
    scales = _scales(hdr_scale, n)
    if base is not None:
        base = [None if b is None else bytes(b) for b in base]
        if len(base) != n:
            raise ValueError("ultrahdr.encode: %d base files for %d images" % (len(base), n))
        for i, b in enumerate(base):
            if b is not None:
                check_base(b, shapes[i], "ultrahdr.encode: base %d" % i)
    images, _, _ = K.gainmap_images(shapes, factor)
    map_shapes = [(-(-h // int(im["factor"])), -(-w // int(im["factor"]))) for (h, w), im in zip(shapes, images)]
    options = dict(base_options or {}, encoder=encoder)
    if encoder == "device":
        import torch
        for t in hdrs + sdrs:
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise TypeError("ultrahdr.encode: encoder='device' takes device tensors (encoder='host' takes host arrays)")
    else:
        sdrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in sdrs]
    # the primaries first: a gain is the ratio to the pixels a viewer will see, which for a primary coded here are the DECODED ones
    primaries = list(base) if base is not None else [None] * n
    todo = [i for i in range(n) if primaries[i] is None]
    if todo:
        coded = jpeg.encode([sdrs[i] for i in todo], **options)
        seen = jpeg.decode(coded, sdrs[todo[0]].device, orient=False) if encoder == "device" else [_pil_rgb(c) for c in coded]
        sdrs = list(sdrs)
        for i, data, pixels in zip(todo, coded, seen):
            primaries[i], sdrs[i] = data, pixels
    if encoder == "host":
        sdr_arena = np.concatenate([s.reshape(-1, 3) for s in sdrs])
        hdr_arena = np.concatenate([np.ascontiguousarray(h, dtype=np.float32).reshape(-1, 3) for h in hdrs])
        maps, meta = K.gainmap_encode_host(sdr_arena, hdr_arena, images, scales, log2_range, reverse_channels)
        pictures = [maps[3 * int(im["cell_off"]):3 * int(im["cell_off"]) + 3 * mh * mw].reshape(mh, mw, 3) for im, (mh, mw) in zip(images, map_shapes)]
    else:
        sdr_arena = sdrs[0].contiguous().reshape(-1) if n == 1 else torch.cat([s.reshape(-1) for s in sdrs])
        hdr_arena = hdrs[0].contiguous().reshape(-1) if n == 1 else torch.cat([h.reshape(-1) for h in hdrs])
        maps, meta_dev = K.gainmap_encode(sdr_arena, hdr_arena, images, scales, log2_range, reverse_channels)
        pictures = [maps[3 * int(im["cell_off"]):3 * int(im["cell_off"]) + 3 * mh * mw].view(mh, mw, 3) for im, (mh, mw) in zip(images, map_shapes)]
    coded_maps = jpeg.encode(pictures, quality=map_quality, subsampling="444", encoder=encoder)
    if encoder == "device":
        meta = meta_dev.cpu().numpy().view(K.GAINMAP_META_DTYPE)    # after the maps' files have come back: no wait of its own
    return [assemble(p, m, metadata_of(meta[i])) for i, (p, m) in enumerate(zip(primaries, coded_maps))]


def _factor_of(shape, map_shape, what):
    for f in range(1, 65):
        if (-(-shape[0] // f), -(-shape[1] // f)) == tuple(map_shape):
            return f
    raise ValueError("%s: a %d x %d map is not ceil(size / f) of a %d x %d image for any f in 1 .. 64"
                     % (what, map_shape[0], map_shape[1], shape[0], shape[1]))


def weight_of(meta, display_boost):
    """rule 8's w: how much of the gain a display with `display_boost` (linear; None: all of it) shows"""
    if display_boost is None:
        return 1.0
    if not (display_boost > 0 and math.isfinite(display_boost)):
        raise ValueError("ultrahdr.decode: display_boost must be a positive number, got %r" % (display_boost,))
    lo, hi = meta["HDRCapacityMin"], meta["HDRCapacityMax"]
    if not hi > lo:
        raise ValueError("ultrahdr.decode: HDRCapacityMax %r is not above HDRCapacityMin %r" % (hi, lo))
    return min(max((math.log2(display_boost) - lo) / (hi - lo), 0.0), 1.0)


def _pil_rgb(data, keep_grey=False):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        if keep_grey and im.mode == "L":
            return np.array(im, dtype=np.uint8)[:, :, None]
        return np.array(im.convert("RGB"), dtype=np.uint8)


def decode(items, display_boost=None, decoder="device", device=None):
    """gain-map JPEG files (paths or bytes) -> one float32 [H, W, 3] RGB image per item: linear light, 1.0 = SDR white, s times the HDR
    image that was encoded (include/shdr.h "gain maps", apply).  display_boost: the display's HDR headroom as a linear factor; None shows
    the whole gain.  decoder="device": both pictures of ALL items go through one jpeg.decode call (PIL where a file is outside that
    decoder's scope), then ONE K.gainmap_apply launch; "pil": PIL decodes, the device applies; "host": PIL and the host twin, and the
    results are host arrays.  The file's own metadata is used: gamma, offsets, a one-channel map."""
    K, jpeg = _mods()
    if decoder not in ("device", "pil", "host"):
        raise ValueError("ultrahdr.decode: decoder must be 'device', 'pil' or 'host', got %r" % (decoder,))
    parts = [split(jpeg._read(item)) for item in items]
    if not parts:
        return []
    files = [p[0] for p in parts] + [p[1] for p in parts]
    n = len(parts)
    if decoder == "device":
        try:
            pixels = jpeg.decode(files, device, orient=False)
        except jpeg.Unsupported:
            pixels = None
    if decoder != "device" or pixels is None:
        pixels = [_pil_rgb(f, keep_grey=i >= n) for i, f in enumerate(files)]
    descs = []
    for i, (_, _, meta) in enumerate(parts):
        what = "ultrahdr.decode: item %d" % i
        if meta["BaseRenditionIsHDR"]:
            raise ValueError("%s: the base rendition is HDR, which this reader does not take" % what)
        sdr, gm = pixels[i], pixels[n + i]
        descs.append(dict(height=sdr.shape[0], width=sdr.shape[1], factor=_factor_of(sdr.shape[:2], gm.shape[:2], what), map_channels=gm.shape[2],
                          gain_min=meta["GainMapMin"], gain_max=meta["GainMapMax"], gamma=meta["Gamma"], offset_sdr=meta["OffsetSDR"],
                          offset_hdr=meta["OffsetHDR"], weight=weight_of(meta, display_boost)))
    images, _ = K.gainmap_apply_images(descs)
    if decoder == "host":
        out = K.gainmap_apply_host(np.concatenate([p.reshape(-1, 3) for p in pixels[:n]]), np.concatenate([p.reshape(-1) for p in pixels[n:]]), images)
    else:
        import torch
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        pixels = [p if isinstance(p, torch.Tensor) else torch.from_numpy(p).to(dev) for p in pixels]
        out = K.gainmap_apply(torch.cat([p.reshape(-1, 3) for p in pixels[:n]]), torch.cat([p.reshape(-1) for p in pixels[n:]]), images)
    return [out[int(im["pix_off"]):int(im["pix_off"]) + int(im["height"]) * int(im["width"])].reshape(int(im["height"]), int(im["width"]), 3)
            for im in images]


def write(path, hdr, sdr, **options):
    """one HDR image and its SDR rendition -> a gain-map JPEG file at `path`; options: encode()'s (base: ONE file's bytes)"""
    for key in options:
        if key not in ENCODE_OPTIONS:
            raise ValueError("ultrahdr.write: unknown option %r (known: %s)" % (key, ", ".join(ENCODE_OPTIONS)))
    if options.get("base") is not None:
        options["base"] = [options["base"]]
    data = encode([hdr], [sdr], **options)[0]
    with open(path, "wb") as f:
        f.write(data)


def read(path, display_boost=None, decoder="device", device=None):
    """a gain-map JPEG file -> its HDR image float32 [H, W, 3] (decode()'s arguments)"""
    return decode([path], display_boost, decoder, device)[0]
