"""PNG output: 8-bit grey, RGB and RGBA images -> finished .png files, coded on the device.

    files = png.encode([u8_a, u8_b, ...])            # uint8 device tensors [H, W] or [H, W, C] of any sizes -> a list of bytes
    png.write_png("preview.png", u8)

The whole batch is ONE stream-ordered launch sequence (csrc/png_enc.hip): the scanlines are filtered (per row the cheapest of PNG's
five predictors, or one fixed type), the filtered stream is cut into segments of 65 520 bytes that the project's deflate encoders
code on their own (deflate="lz", the one with LZ77 matches, or "huffman"), the segments are joined into one zlib stream per image
the way Z_SYNC_FLUSH joins them, and Adler-32, the chunk CRCs, IHDR and IEND are written on the device too; only the finished bytes
come back.  Every PNG reader opens the files.  On smooth content they are larger than PIL's (zlib level 6 with hash chains and lazy
matching, and libpng's filter heuristics, find more): tools/png_write_bench.py reports by how much.  Bit depth 8 only; no palettes,
no interlace, no ancillary chunks.  encoder="host" is libshdr's host twin, which writes the same bytes (csrc/png.h)."""
import numpy as np

ENCODE_OPTIONS = ("filter", "deflate", "encoder")
_ENCODE_BUFFERS = {}           # (thread, device, stream) -> encode()'s output and workspace, kept from call to call: encode() has copied
                               # the files to the host before it returns, and both are sized for the worst case


def _ops():
    try:
        from . import _ops as K
    except ImportError:
        import _ops as K
    return K


def encode(images, filter="adaptive", deflate="lz", encoder="device", stage_ms=None):
    """8-bit images -> PNG files (a list of bytes).  images: a list of uint8 device tensors [H, W] (grey) or [H, W, C] with C = 1, 3
    (RGB) or 4 (RGBA), of any sizes and channel counts, or one [N, H, W, C] tensor; with encoder="host" host arrays, coded by
    libshdr's host twin (the same bytes).  filter: "adaptive" (per row the type with the smallest sum of absolute filtered values)
    or "none" | "sub" | "up" | "average" | "paeth" for every row; deflate: "lz" | "huffman".  encoder="device": ONE batch call
    (K.png_encode) and one copy of the finished files to the host.  stage_ms: a list that receives the device times of
    K.PNG_STAGE_NAMES."""
    K = _ops()
    if encoder not in ("device", "host"):
        raise ValueError("png.encode: encoder must be 'device' or 'host', got %r" % (encoder,))
    batch = not isinstance(images, (list, tuple))
    if batch and getattr(images, "ndim", 0) != 4:
        raise ValueError("png.encode: expected a list of images [H, W] or [H, W, C], or one [N, H, W, C] batch, got %s"
                         % (tuple(getattr(images, "shape", ())),))
    if not len(images):
        raise ValueError("png.encode: no images")
    if encoder == "host":
        if any(hasattr(a, "is_cuda") and a.is_cuda for a in images):
            raise ValueError("png.encode: encoder='host' takes host arrays")
        return [K.png_encode_host(np.asarray(a), filter, deflate) for a in images]
    import torch
    tensors = list(images)
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError("png.encode: encoder='device' takes uint8 device tensors, got %s" % (type(t).__name__,))
        if t.dtype != torch.uint8:
            raise TypeError("png.encode: expected uint8 pixels, got %s" % (t.dtype,))
        if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3, 4)):
            raise ValueError("png.encode: expected [H, W] or [H, W, C] with C = 1 (grey), 3 (RGB) or 4 (RGBA), got %s" % (tuple(t.shape),))
        if t.numel() == 0:
            raise ValueError("png.encode: an image has no pixels: %s" % (tuple(t.shape),))
    shapes = [(t.shape[0], t.shape[1], t.shape[2] if t.dim() == 3 else 1) for t in tensors]
    if batch:
        flat = images.contiguous().reshape(-1)
    else:
        flat = tensors[0].contiguous().reshape(-1) if len(tensors) == 1 else torch.cat([t.reshape(-1) for t in tensors])
    import threading
    key = (threading.get_ident(), flat.device, torch.cuda.current_stream(flat.device).cuda_stream)
    out, offsets = K.png_encode(flat, shapes, filter, deflate, stage_ms=stage_ms, buffers=_ENCODE_BUFFERS.setdefault(key, {}))
    off = offsets.cpu().numpy()                                  # 8 (n + 1) bytes first, then ONE copy of exactly the bytes written
    data = out[:int(off[-1])].cpu().numpy()
    return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(shapes))]


def write_png(path, image, **options):
    """one image [H, W] or [H, W, C] -> a PNG file at `path`; options: encode()'s (filter, deflate, encoder)"""
    for key in options:
        if key not in ENCODE_OPTIONS:
            raise ValueError("png.write_png: unknown option %r (known: %s)" % (key, ", ".join(ENCODE_OPTIONS)))
    if getattr(image, "ndim", 0) not in (2, 3):
        raise ValueError("png.write_png: expected one image [H, W] or [H, W, C], got %s" % (tuple(getattr(image, "shape", ())),))
    data = encode([image], **options)[0]
    with open(path, "wb") as f:
        f.write(data)
