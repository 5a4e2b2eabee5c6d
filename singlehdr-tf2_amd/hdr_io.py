"""Image I/O around the inference path: the file loop of test_real_refinement.py:114-155.

    recon = HdrReconstructor(pipeline.Inference(deq, lin, hal, ref))
    recon.reconstruct_file("scene.jpg", "scene.hdr")          # or recon.reconstruct_dir(in_dir, out_dir)

Per image the reference does: cv2.imread (BGR) -> flip to RGB, /255 -> cubic resize up to a multiple of 64 ->
symmetric pad by 32 -> `bgr2rgb` (a second flip: the networks see BGR-ordered data) -> inference ->
flip, crop the pad, cubic resize back -> cv2.imwrite('.hdr') of the channel-reversed result.  Here only the JPEG
decode (PIL) and the file write are host work; the uint8 image goes to the device once and RGBE bytes (4 B/pixel
instead of 12) come back -- every step in between is a libshdr kernel (csrc/imageio.hip).  With encoder="device" the scanline
RLE runs on the device too (csrc/hdr_rle.hip, the host routine's bytes) and only the coded bytes come back; reconstruct_files
does that for a whole list of files in one batched encode and one copy.  output_format="exr" stores the float estimate as OpenEXR
instead (exr.encode_exr: HALF or FLOAT, ZIP by default) -- RGBE keeps an 8-bit mantissa, about 1 % steps.  output_format="ultrahdr"
stores it as a gain-map JPEG (ultrahdr.encode): the input photograph with a log2 gain map behind it, which browsers and phones show as HDR.
cv2 is not installed in this image, so cv2's behaviour is restated: INTER_CUBIC = a -0.75 bicubic
with replicated borders, '.hdr' = Radiance RGBE with adaptive scanline RLE and the `-Y h +X w` orientation.
"""
import ctypes
import glob
import os
import re
import time

import numpy as np
import torch

try:
    from . import _lib
    from . import _ops as K
    from . import exr
except ImportError:
    import _lib
    import _ops as K
    import exr

PADDING = 32          # test_real_refinement.py:135
MULTIPLE = 64         # :129-133


def read_ldr(path):
    """8-bit image file -> uint8 RGB [H, W, 3] (cv2.imread drops alpha and converts grey to 3 channels as well).  Like
    cv2.imread with its default flags (test_real_refinement.py:124) the EXIF Orientation tag is APPLIED: a camera JPEG stored
    rotated comes back upright."""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        return np.array(ImageOps.exif_transpose(im).convert("RGB"), dtype=np.uint8)          # a writable copy


def rle_encode(rgbe):
    """uint8 [H, W, 4] -> scanline-RLE bytes (libshdr host routine)"""
    rgbe = np.ascontiguousarray(rgbe, dtype=np.uint8)
    h, w, _ = rgbe.shape
    cap = h * (4 + 4 * (w + w // 127 + 2))
    out = np.empty(cap, dtype=np.uint8)
    n = _lib.load().shdr_rgbe_rle_encode(ctypes.c_void_p(rgbe.ctypes.data), w, h, ctypes.c_void_p(out.ctypes.data), cap)
    if n < 0:
        raise RuntimeError("shdr_rgbe_rle_encode: %s" % _lib.load().shdr_last_error().decode())
    return out[:n].tobytes()


def rle_encode_device(rgbe):
    """uint8 RGBE device tensor [H, W, 4] or [N, H, W, 4], or a list of [H, W, 4] tensors of different sizes -> a list of scanline-RLE
    `bytes`, one per image: rle_encode's bytes, coded by the device kernels (K.rgbe_rle_encode) and brought back in ONE copy of the
    coded bytes (after a 8 (N + 1)-byte copy of the offsets that says how many there are) -- the pixels stay on the device"""
    data, offsets = K.rgbe_rle_encode(rgbe)
    off = offsets.cpu().numpy()
    blob = data[:int(off[-1])].cpu().numpy().tobytes()
    return [blob[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def _check_encoder(encoder, what, output_format="hdr"):
    """"device_lz" (the device deflate encoder with LZ77 matches, exr.encode_exr) exists for OpenEXR output only"""
    if encoder not in ("host", "device", "device_lz"):
        raise ValueError("%s: encoder must be 'host', 'device' or 'device_lz', got %r" % (what, encoder))
    if encoder == "device_lz" and output_format == "hdr":
        raise ValueError("%s: encoder 'device_lz' is for OpenEXR output (output_format='exr'); Radiance files take 'host' or 'device'" % what)


def _check_format(output_format, what):
    if output_format not in ("hdr", "exr", "ultrahdr"):
        raise ValueError("%s: output_format must be 'hdr', 'exr' or 'ultrahdr', got %r" % (what, output_format))


def _exr_options(encoder, exr_options):
    """encode_exr's keyword arguments for the file loop: the estimate is in the networks' channel order.  exr_options passes through
    as it is, compression="piz" with piz="host" / "device" included"""
    opts = dict(encoder=encoder)
    opts.update(exr_options or {})
    opts["reverse_channels"] = True
    return opts


def _jpeg_base(data):
    """the bytes of an input file if they can stand as the primary image of a gain-map file: a JPEG whose pixels are stored upright
    (an EXIF Orientation other than 1 is applied by the readers, so the estimate would not lie on the coded pixels); None otherwise"""
    try:
        from . import jpeg, ultrahdr
    except ImportError:
        import jpeg
        import ultrahdr
    if data[:2] != b"\xff\xd8":
        return None
    try:
        segs = ultrahdr._segments(data, "input")
    except ValueError:
        return None
    for seg in segs:
        if seg[0] == 0xE1 and jpeg._exif_orientation(data[seg[1] + 4:seg[2]]) not in (None, 1):
            return None
    return data


def _write_scanlines(path, h, w, data):
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
        f.write(data)


def write_hdr(path, rgbe, encoder="host"):
    """Radiance picture file from RGBE bytes [H, W, 4]: a host array or a uint8 device tensor.  encoder: "host" codes the scanlines
    with the libshdr host routine (a device tensor is copied to the host first), "device" with the device kernels (a host array is
    uploaded first); the files are identical"""
    _check_encoder(encoder, "write_hdr")
    on_device = isinstance(rgbe, torch.Tensor)
    if not on_device:
        rgbe = np.asarray(rgbe)
    if rgbe.dtype != (torch.uint8 if on_device else np.uint8) or rgbe.ndim != 3 or rgbe.shape[2] != 4:
        raise ValueError("write_hdr: expected uint8 [H, W, 4] RGBE (see _ops.rgbe_encode)")
    h, w, _ = rgbe.shape
    if encoder == "device":
        if not on_device:
            rgbe = torch.from_numpy(np.ascontiguousarray(rgbe)).to(torch.device("cuda", torch.cuda.current_device()))
        data = rle_encode_device(rgbe)[0]
    else:
        data = rle_encode(rgbe.cpu().numpy() if on_device else rgbe)
    _write_scanlines(path, h, w, data)


def rle_decode(data, height, width):
    """scanline bytes (flat or RLE) -> uint8 RGBE [height, width, 4] (libshdr host routine); ValueError on truncated or corrupt data"""
    buf = np.frombuffer(data, dtype=np.uint8)
    rgbe = np.empty((height, width, 4), dtype=np.uint8)
    n = _lib.load().shdr_rgbe_rle_decode(ctypes.c_void_p(buf.ctypes.data), buf.size, width, height, ctypes.c_void_p(rgbe.ctypes.data))
    if n < 0:
        raise ValueError(_lib.load().shdr_last_error().decode())
    return rgbe


class Scanlines:
    """The header walk of read_rgbe without the decode: height, width and the scanline bytes of one Radiance file (`path`: where they
    came from, for messages)"""

    def __init__(self, height, width, data, path=None):
        self.height, self.width, self.data, self.path = int(height), int(width), data, path

    @property
    def shape(self):
        return (self.height, self.width, 4)

    def decode(self):
        """the pixels uint8 [H, W, 4], by the host routine"""
        return rle_decode(self.data, self.height, self.width)


def read_scanlines(path):
    """Radiance picture file -> Scanlines: the container is checked, the scanlines are left coded (rle_decode_device's input)"""
    with open(path, "rb") as f:
        data = f.read()
    if data.startswith(b"\x76\x2f\x31\x01"):
        raise ValueError("%s: OpenEXR files are not supported (Radiance .hdr only)" % path)
    if not data.startswith(b"#?"):
        raise ValueError("%s: not a Radiance file" % path)
    end = data.index(b"\n\n")
    if b"32-bit_rle_rgbe" not in data[:end]:
        raise ValueError("%s: only FORMAT=32-bit_rle_rgbe is supported" % path)
    nl = data.index(b"\n", end + 2)
    m = re.match(rb"-Y (\d+) \+X (\d+)", data[end + 2:nl])
    if not m:
        raise ValueError("%s: unsupported resolution line %r" % (path, data[end + 2:nl]))
    return Scanlines(int(m.group(1)), int(m.group(2)), memoryview(data)[nl + 1:], path)


def check_decoder_option(what, decoder):
    """the scanline decoder of a reader: "host" (shdr_rgbe_rle_decode) or "device" (K.rgbe_rle_decode)"""
    if decoder not in ("host", "device"):
        raise ValueError("%s: the Radiance scanline decoder must be 'host' or 'device', got %r" % (what, decoder))
    return decoder


def _item_name(item, i):
    return item.path if item.path is not None else "scanlines[%d]" % i


def rle_decode_device(items, device=None):
    """a list of Scanlines -> a list of uint8 device tensors [H, W, 4], rle_decode's pixels: ONE upload of all coded bytes, ONE decode
    call (K.rgbe_rle_decode) and ONE read-back of the per-file reports.  A file with more line markers than the device decoder takes
    (RGBE_DEC_FALLBACK) is decoded by rle_decode on the host and uploaded.  The first file of the list that the format refuses raises
    ValueError("<path>: rgbe_rle_decode: ...") with the host route's text."""
    items = list(items)
    if not items:
        return []
    device = device or torch.device("cuda", torch.cuda.current_device())
    shapes = np.array([(it.height, it.width) for it in items], dtype=np.int32).reshape(-1, 2)
    if (shapes <= 0).any():
        bad = int(np.argmax((shapes <= 0).any(axis=1)))
        raise ValueError("%s: rgbe_rle_decode: bad arguments" % _item_name(items[bad], bad))
    sizes = [len(it.data) for it in items]
    src_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blob = np.empty(max(int(src_off[-1]), 1), dtype=np.uint8)
    for it, a, b in zip(items, src_off[:-1], src_off[1:]):
        blob[a:b] = np.frombuffer(it.data, dtype=np.uint8)
    src = torch.from_numpy(blob).to(device)[:int(src_off[-1])]
    out, out_off, status, line, _ = K.rgbe_rle_decode(src, src_off, shapes)
    report = torch.stack([status, line]).cpu().numpy()                                        # one read-back, and the wait
    off = np.concatenate([[0], np.cumsum(4 * shapes[:, 0].astype(np.int64) * shapes[:, 1])])
    result = []
    for i, it in enumerate(items):
        st, ln = int(report[0, i]), int(report[1, i])
        if st == K.RGBE_DEC_OK:
            result.append(out[off[i]:off[i + 1]].view(it.height, it.width, 4))
        elif st == K.RGBE_DEC_FALLBACK:
            try:
                result.append(torch.from_numpy(it.decode()).to(device))
            except ValueError as exc:
                raise ValueError("%s: %s" % (_item_name(it, i), exc)) from None
        else:
            raise ValueError("%s: %s" % (_item_name(it, i), K.rgbe_dec_message(st, ln)))
    return result


def read_rgbe(path, decoder="host"):
    """Radiance picture file -> its RGBE bytes uint8 [H, W, 4] (flat and RLE scanlines, -Y +X orientation).  decoder="device": the
    scanlines are decoded on the device (rle_decode_device) and the result is a device tensor with the same bytes"""
    check_decoder_option("read_rgbe", decoder)
    lines = read_scanlines(path)
    if decoder == "device":
        return rle_decode_device([lines])[0]
    try:
        return lines.decode()
    except ValueError as exc:
        raise ValueError("%s: %s" % (path, exc)) from None


def read_rgbe_batch(paths, decoder="host", device=None):
    """read_rgbe for a list of files: host arrays ("host"), or device tensors out of ONE rle_decode_device ("device")"""
    check_decoder_option("read_rgbe_batch", decoder)
    if decoder == "host":
        return [read_rgbe(p) for p in paths]
    return rle_decode_device([read_scanlines(p) for p in paths], device)


def read_hdr(path):
    """Radiance picture file -> float32 RGB [H, W, 3] (flat and RLE scanlines, -Y +X orientation)"""
    return rgbe_decode(read_rgbe(path))


def rgbe_decode(rgbe):
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - (128 + 8))).astype(np.float32)
    return rgbe[..., :3].astype(np.float32) * scale[..., None]


def _check_preview_encoder(encoder, path, what):
    if encoder not in ("pil", "device", "device_png"):
        raise ValueError("%s: the preview encoder must be 'pil', 'device' or 'device_png', got %r" % (what, encoder))
    ext = os.path.splitext(str(path))[1].lower()
    if encoder == "device" and ext not in (".jpg", ".jpeg"):
        raise ValueError("%s: the device encoder writes JPEG files only (.jpg / .jpeg; 'device_png' writes .png), got %r" % (what, path))
    if encoder == "device_png" and ext != ".png":
        raise ValueError("%s: the preview encoder 'device_png' writes PNG files only (.png), got %r" % (what, path))


def _device_coder(encoder):
    """(module, its one-file writer name) behind a device preview encoder"""
    try:
        from . import jpeg, png
    except ImportError:
        import jpeg
        import png
    return (png, "write_png") if encoder == "device_png" else (jpeg, "write_jpeg")


def write_preview(path, hdr_tensor, peak=None, reverse_channels=False, encoder="pil", jpeg_options=None):
    """8-bit preview of an HDR image: float32 [H, W, 3] on the device -> K.tonemap_u8 (mu-law tone curve up to `peak`, default the
    image's maximum, then a 2.2 gamma) -> an image file through PIL (the format follows the extension; PNG is lossless).
    encoder="device" (only for .jpg / .jpeg paths) codes the file on the device instead (jpeg.encode) and copies the finished bytes:
    the bytes PIL writes for the same 8-bit image and the same `jpeg_options` (quality, subsampling, restart_interval; PIL's defaults
    where they are not given: quality 75, 4:2:0).  encoder="device_png" (only for .png paths) writes a lossless PNG on the device
    (png.encode; `jpeg_options` then holds ITS options: filter, deflate): the same pixels as PIL's file, not the same bytes."""
    if hdr_tensor.dim() != 3:
        raise ValueError("write_preview: expected one image [H, W, 3], got %s" % (tuple(hdr_tensor.shape),))
    _check_preview_encoder(encoder, path, "write_preview")
    options = dict(jpeg_options or {})
    u8 = K.tonemap_u8(hdr_tensor.contiguous(), peak, reverse_channels)
    if encoder != "pil":
        module, writer = _device_coder(encoder)
        getattr(module, writer)(path, u8, **options)
        return
    from PIL import Image
    if "restart_interval" in options:
        options["restart_marker_blocks"] = options.pop("restart_interval")
    if "subsampling" in options:
        options["subsampling"] = {"444": 0, "422": 1, "420": 2}.get(options["subsampling"], options["subsampling"])
    Image.fromarray(u8.cpu().numpy(), "RGB").save(path, **options)


class HdrReconstructor:
    """LDR file -> HDR file with the reference tool's geometry (resize to 64x, 32-pixel symmetric pad, crop, resize back).
    `inference` is any `pipeline.Inference` / `GraphedInference`, e.g. `Inference(deq, lin, hal, ref, precision="fp16")` for the
    native-fp16 inference mode."""

    def __init__(self, inference, padding=PADDING, multiple=MULTIPLE):
        self.inference, self.padding, self.multiple = inference, padding, multiple

    def reconstruct(self, rgb_u8):
        """uint8 RGB [H, W, 3] (host) -> RGBE bytes uint8 [H, W, 4] (host) of the HDR estimate, RGB order"""
        return K.rgbe_encode(self.reconstruct_device(rgb_u8), reverse_channels=True).cpu().numpy()

    def reconstruct_device(self, rgb_u8):
        """uint8 RGB [H, W, 3] (host array, or a uint8 device tensor such as jpeg.decode returns: no host round trip) -> the HDR
        estimate float32 [H, W, 3] on the device, in the NETWORK's channel order: the file's blue first (encode or preview it with
        reverse_channels=True)"""
        if isinstance(rgb_u8, torch.Tensor):
            if rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or not rgb_u8.is_cuda:
                raise ValueError("reconstruct_device: a tensor input must be uint8 [H, W, 3] on the device")
            u8 = rgb_u8.contiguous()
        else:
            rgb_u8 = np.array(rgb_u8, dtype=np.uint8)           # contiguous, writable (torch.from_numpy)
            u8 = torch.from_numpy(rgb_u8).to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
        h, w, _ = u8.shape
        x = K.u8_to_unit(u8, False)[None]                                                         # RGB in [0,1]  (:125)
        m = self.multiple
        rh, rw = -(-h // m) * m, -(-w // m) * m
        if (rh, rw) != (h, w):
            x = K.resize_cubic(x, (rh, rw))                                                       # :129-133
        x = K.pad_symmetric(x, self.padding)                                                      # :135-136
        x = K.reverse3(x)                                                                         # tf_utils.bgr2rgb (:141)
        with torch.no_grad():
            y = self.inference(x)                                                                 # :142
        p = self.padding
        y = y[:, p:y.shape[1] - p, p:y.shape[2] - p, :].contiguous()                              # :145 (flip folded below)
        if (rh, rw) != (h, w):
            y = K.resize_cubic(y, (h, w))                                                         # :146-147
        # :144 flips the channels, :150 flips them back and cv2 stores its BGR argument as RGB: the net's channel 0 is the
        # file's blue, i.e. the network output is read as BGR
        return y[0]

    def _read_device(self, ldr_path, decoder, what):
        if decoder not in ("pil", "device", "device_scan"):
            raise ValueError("%s: decoder must be 'pil', 'device' or 'device_scan', got %r" % (what, decoder))
        if decoder != "pil":
            try:
                from . import jpeg
            except ImportError:
                import jpeg
            return self.reconstruct_device(jpeg.read_ldr_device(ldr_path, unstuff="device" if decoder == "device_scan" else "host"))
        return self.reconstruct_device(read_ldr(ldr_path))

    def _read_ultrahdr(self, ldr_path, decoder, what):
        """(estimate, the input's pixels uint8 on the device, the input's bytes if they can be the primary image or None)"""
        if decoder not in ("pil", "device", "device_scan"):
            raise ValueError("%s: decoder must be 'pil', 'device' or 'device_scan', got %r" % (what, decoder))
        with open(ldr_path, "rb") as f:
            base = _jpeg_base(f.read())
        if decoder != "pil":
            try:
                from . import jpeg
            except ImportError:
                import jpeg
            u8 = jpeg.read_ldr_device(ldr_path, unstuff="device" if decoder == "device_scan" else "host")
        else:
            u8 = torch.from_numpy(read_ldr(ldr_path)).to(torch.device("cuda", torch.cuda.current_device()))
        return self.reconstruct_device(u8), u8, base

    def _write_ultrahdr(self, ldr_paths, hdr_paths, decoder, ultrahdr_options, what):
        """the estimates of a list of files as gain-map JPEG files, ONE ultrahdr.encode call; returns the estimates"""
        try:
            from . import ultrahdr
        except ImportError:
            import ultrahdr
        options = dict(ultrahdr_options or {})
        for key in options:
            if key not in ultrahdr.ENCODE_OPTIONS or key in ("base", "reverse_channels", "encoder"):
                raise ValueError("%s: ultrahdr_options takes %s, got %r" % (what, ", ".join(
                    k for k in ultrahdr.ENCODE_OPTIONS if k not in ("base", "reverse_channels", "encoder")), key))
        ys, sdrs, bases = [], [], []
        for src in ldr_paths:
            y, u8, base = self._read_ultrahdr(src, decoder, what)
            ys.append(y.contiguous())
            sdrs.append(u8)
            bases.append(base)
        for dst, data in zip(hdr_paths, ultrahdr.encode(ys, sdrs, base=bases, reverse_channels=True, **options)):
            with open(dst, "wb") as f:
                f.write(data)
        return ys

    def reconstruct_file(self, ldr_path, hdr_path, preview_path=None, decoder="pil", encoder="host", output_format="hdr",
                         exr_options=None, preview_encoder="pil", preview_options=None, ultrahdr_options=None):
        """preview_path: also write an 8-bit tone-mapped PNG of the estimate (write_preview), for viewers without HDR support;
        preview_encoder, preview_options: write_preview's encoder and jpeg_options ("device": a .jpg preview coded on the device,
        "device_png": a .png preview coded on the device).
        decoder: "pil" decodes the file on the host (read_ldr); "device" decodes baseline JPEG files on the device
        (jpeg.read_ldr_device: the same bytes, PIL for files out of its scope); "device_scan" is "device" with the scan prepared on
        the device too (unstuff="device": the end of the scan, the byte stuffing and the restart segments; the same bytes again).
        encoder: "host" copies the RGBE pixels back and codes the scanlines on the host; "device" codes them on the device and copies
        the coded bytes (write_hdr: the same file).
        output_format: "hdr" writes a Radiance file; "exr" writes the float estimate as OpenEXR without the RGBE conversion
        (exr.encode_exr with `exr_options`, a dict of its keyword arguments such as pixel_type or compression; `encoder` then says
        who deflates, and "device_lz", the device encoder with LZ77 matches, is a third choice that only this format has.
        exr_options=dict(compression="piz", piz="device") -- or piz="host" -- writes PIZ-compressed files, for which `encoder` plays
        no part; the PIZ writer is unpinned against the OpenEXR library, see exr.encode_exr);
        "ultrahdr" writes a gain-map JPEG file (ultrahdr.encode with `ultrahdr_options`: factor, hdr_scale, log2_range, base_options,
        map_quality): the input file's own bytes are the primary image when it is a JPEG stored upright, otherwise the input's pixels are
        coded with base_options (and the gains are taken against the coded pixels); `encoder` plays no part)"""
        _check_encoder(encoder, "reconstruct_file", output_format)
        _check_format(output_format, "reconstruct_file")
        if preview_path is not None:
            _check_preview_encoder(preview_encoder, preview_path, "reconstruct_file")
        if output_format == "ultrahdr":
            y = self._write_ultrahdr([ldr_path], [hdr_path], decoder, ultrahdr_options, "reconstruct_file")[0]
            if preview_path is not None:
                write_preview(preview_path, y, reverse_channels=True, encoder=preview_encoder, jpeg_options=preview_options)
            return
        y = self._read_device(ldr_path, decoder, "reconstruct_file")
        if output_format == "exr":
            exr.write_exr(hdr_path, y, **_exr_options(encoder, exr_options))
        else:
            rgbe = K.rgbe_encode(y, reverse_channels=True)
            write_hdr(hdr_path, rgbe if encoder == "device" else rgbe.cpu().numpy(), encoder=encoder)
        if preview_path is not None:
            write_preview(preview_path, y, reverse_channels=True, encoder=preview_encoder, jpeg_options=preview_options)

    def _write_previews(self, ys, preview_paths, preview_encoder, preview_options):
        """the previews of a list of estimates: with a device encoder ALL of them are tone-mapped and coded in one call"""
        if preview_encoder == "pil":
            for dst, y in zip(preview_paths, ys):
                write_preview(dst, y, reverse_channels=True, jpeg_options=preview_options)
            return
        module, _ = _device_coder(preview_encoder)
        u8 = [K.tonemap_u8(y.contiguous(), None, True) for y in ys]
        for dst, data in zip(preview_paths, module.encode(u8, **dict(preview_options or {}))):
            with open(dst, "wb") as f:
                f.write(data)

    def reconstruct_files(self, ldr_paths, hdr_paths, decoder="pil", encoder="host", output_format="hdr", exr_options=None,
                          preview_paths=None, preview_encoder="pil", preview_options=None, ultrahdr_options=None):
        """reconstruct_file for a list of files: geometry and inference per image as there, then ALL results of the call coded in one
        batched scanline-RLE launch sequence and brought back in one copy (encoder="device"), then the files are written.
        encoder="host" (the default, as everywhere) is a loop over reconstruct_file.  The RGBE pixels of the whole list stay on the device until they are coded:
        4 B per pixel.  output_format="exr": the float estimates of the whole list go through ONE exr.encode_exr call, whatever the
        encoder (and whatever the compression: exr_options=dict(compression="piz", piz="device") codes every chunk of every file in
        one K.piz_encode call).  output_format="ultrahdr": the whole list goes through ONE ultrahdr.encode call (`ultrahdr_options`, see
        reconstruct_file).  preview_paths: one 8-bit preview per file as reconstruct_file writes it; with
        preview_encoder="device_png" (.png paths) or "device" (.jpg paths) the previews of the whole list are coded in one call."""
        _check_encoder(encoder, "reconstruct_files", output_format)
        _check_format(output_format, "reconstruct_files")
        ldr_paths, hdr_paths = list(ldr_paths), list(hdr_paths)
        if len(ldr_paths) != len(hdr_paths):
            raise ValueError("reconstruct_files: %d inputs but %d outputs" % (len(ldr_paths), len(hdr_paths)))
        if preview_paths is not None:
            preview_paths = list(preview_paths)
            if len(preview_paths) != len(ldr_paths):
                raise ValueError("reconstruct_files: %d inputs but %d previews" % (len(ldr_paths), len(preview_paths)))
            for dst in preview_paths:
                _check_preview_encoder(preview_encoder, dst, "reconstruct_files")
            previews = dict(preview_encoder=preview_encoder, preview_options=preview_options)
        if decoder not in ("pil", "device", "device_scan"):
            raise ValueError("reconstruct_files: decoder must be 'pil', 'device' or 'device_scan', got %r" % (decoder,))
        if output_format == "ultrahdr":
            if not ldr_paths:
                return
            ys = self._write_ultrahdr(ldr_paths, hdr_paths, decoder, ultrahdr_options, "reconstruct_files")
            if preview_paths is not None:
                self._write_previews(ys, preview_paths, **previews)
            return
        if output_format == "exr":
            if not ldr_paths:
                return
            ys = [self._read_device(src, decoder, "reconstruct_files") for src in ldr_paths]
            for dst, data in zip(hdr_paths, exr.encode_exr(ys, **_exr_options(encoder, exr_options))):
                with open(dst, "wb") as f:
                    f.write(data)
            if preview_paths is not None:
                self._write_previews(ys, preview_paths, **previews)
            return
        if encoder == "host" and preview_paths is None:
            for src, dst in zip(ldr_paths, hdr_paths):
                self.reconstruct_file(src, dst, decoder=decoder)
            return
        if not ldr_paths:
            return
        ys, rgbe = [], []
        for src in ldr_paths:
            y = self._read_device(src, decoder, "reconstruct_files")
            rgbe.append(K.rgbe_encode(y, reverse_channels=True))
            if preview_paths is not None:                        # the float estimates are kept only for the previews: 12 B per pixel
                ys.append(y)
        if encoder == "host":
            for dst, img in zip(hdr_paths, rgbe):
                write_hdr(dst, img.cpu().numpy(), encoder="host")
        else:
            for dst, img, data in zip(hdr_paths, rgbe, rle_encode_device(rgbe)):
                _write_scanlines(dst, img.shape[0], img.shape[1], data)
        if preview_paths is not None:
            self._write_previews(ys, preview_paths, **previews)

    def reconstruct_dir(self, dataset_dir, output_dir, pattern="*.jpg", verbose=True, decoder="pil", encoder="host", group=16,
                        output_format="hdr", exr_options=None, preview_dir=None, preview_encoder="pil", preview_options=None,
                        ultrahdr_options=None):
        """the `for ldr_img_path in ldr_imgs` loop (:119-151); returns the written paths.  decoder, encoder: as reconstruct_file;
        with encoder="device" the files go through reconstruct_files in groups of `group`.  output_format="exr" names the outputs
        *.exr; output_format="ultrahdr" names them *.jpg, sends the files through reconstruct_files in groups of `group` whatever the
        encoder, and refuses an output_dir that is dataset_dir: the outputs would overwrite the inputs.  preview_dir: also write an 8-bit preview per file there (*.png, or *.jpg with preview_encoder="device"), through
        reconstruct_files' preview_paths"""
        _check_encoder(encoder, "reconstruct_dir", output_format)
        _check_format(output_format, "reconstruct_dir")
        fmt = dict(output_format=output_format, exr_options=exr_options)
        grouped = encoder != "host" or output_format == "ultrahdr"
        if output_format == "ultrahdr":
            if os.path.realpath(output_dir) == os.path.realpath(dataset_dir):
                raise ValueError("reconstruct_dir: output_dir %r is dataset_dir: the gain-map files (*.jpg) would overwrite the inputs" % (output_dir,))
            fmt["ultrahdr_options"] = ultrahdr_options
        os.makedirs(output_dir, exist_ok=True)
        if preview_dir is not None:
            os.makedirs(preview_dir, exist_ok=True)
            fmt.update(preview_encoder=preview_encoder, preview_options=preview_options)
        written = []
        paths = sorted(glob.glob(os.path.join(dataset_dir, pattern)))
        step = max(int(group), 1) if grouped else 1
        for i in range(0, len(paths), step):
            start = time.perf_counter()
            part = paths[i:i + step]
            ext = "jpg" if output_format == "ultrahdr" else output_format
            outs = [os.path.join(output_dir, os.path.split(path)[-1].split(".")[0] + "." + ext) for path in part]        # :148-149
            if preview_dir is not None:
                ext = ".jpg" if preview_encoder == "device" else ".png"
                fmt["preview_paths"] = [os.path.join(preview_dir, os.path.splitext(os.path.basename(out))[0] + ext) for out in outs]
            if grouped or preview_dir is not None:
                self.reconstruct_files(part, outs, decoder=decoder, encoder=encoder, **fmt)
            else:
                self.reconstruct_file(part[0], outs[0], decoder=decoder, **fmt)
            written.extend(outs)
            if verbose:
                print("Spends time : %s seconds" % (time.perf_counter() - start))
        return written
