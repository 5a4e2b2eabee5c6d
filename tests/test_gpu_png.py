"""The PNG writer on the device (csrc/png_enc.hip, png.encode) against libshdr's host twin, byte for byte and offset for offset -- the
twin itself is held to the NumPy reference, zlib and PIL by test_png_host.py -- and the preview routes of hdr_io."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as R

pytestmark = pytest.mark.gpu

FILTER_OPTIONS = R.FILTERS + ("adaptive",)


@pytest.fixture(scope="module")
def cpu_list():
    """the images of the CPU tests, in one list of mixed sizes and channel counts: [(image, filter)]"""
    return [(img, "adaptive") for img in R.filter_cases().values()] + list(R.file_cases().values())


def _device_files(K, images, filter, deflate):
    """one K.png_encode call over the images; the files, and the offsets"""
    flat = torch.cat([torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1) for a in images])
    shapes = [R.as_hwc(a).shape for a in images]
    out, offsets = K.png_encode(flat, shapes, filter, deflate)
    off = offsets.cpu().numpy()
    data = out.cpu().numpy()
    files = [data[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])]
    out2, offsets2 = K.png_encode(flat, shapes, filter, deflate)                 # a second run: the same bytes
    assert torch.equal(offsets, offsets2) and torch.equal(out[:int(off[-1])], out2[:int(off[-1])])
    return files, off


def _check(K, images, filter, deflate):
    want = [K.png_encode_host(a, filter, deflate) for a in images]
    got, off = _device_files(K, images, filter, deflate)
    assert off[0] == 0 and list(np.diff(off)) == [len(w) for w in want]        # the offsets are exact
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "image %d %s, filter %s, deflate %s" % (i, images[i].shape, filter, deflate)
    return got


@pytest.mark.parametrize("deflate", ["lz", "huffman"])
def test_cpu_list_in_one_mixed_batch(shdr, cpu_list, deflate):
    K = shdr._ops
    for f in FILTER_OPTIONS:                                                    # the list's own filters: one batch each
        images = [img for img, g in cpu_list if g == f]
        got = _check(K, images, f, deflate)
        if deflate == "lz" and f == "adaptive":
            for data, img in zip(got[-6:], images[-6:]):                        # and the device's own bytes before the judges, for some
                R.check_file(data, img, f)


@pytest.mark.parametrize("deflate", ["lz", "huffman"])
@pytest.mark.parametrize("filter", FILTER_OPTIONS)
def test_batches_of_1_and_17(shdr, filter, deflate):
    K = shdr._ops
    shapes = [(5, 9, 3), (1, 1, 1), (12, 31, 4), (3, 64, 1), (40, 21, 3), (2, 2, 4), (9, 130, 3), (7, 1, 3), (1, 77, 1), (16, 16, 3),
              (33, 5, 4), (4, 300, 1), (6, 6, 3), (25, 25, 1), (2, 511, 3), (11, 11, 4), (60, 90, 3)]
    images = []
    for k, (h, w, c) in enumerate(shapes):
        y, x = np.mgrid[0:h, 0:w]
        smooth = np.stack([(x * (k % 5) + y * 3 + x * y // 9 + 11 * j) for j in range(c)], axis=-1)
        images.append(((smooth + R.noise(h, w, c, seed=k) // (8 if k % 3 else 1)) & 255).astype(np.uint8))
    assert len(images) == 17
    _check(K, images, filter, deflate)
    got = _check(K, images[4:5], filter, deflate)
    R.check_file(got[0], images[4], filter)


@pytest.mark.parametrize("row_bytes", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097])
def test_tile_and_wave_edges(shdr, row_bytes):
    """rows of W C + 1 bytes around the wave, the block and the deflate tile"""
    K = shdr._ops
    n = row_bytes - 1
    c = 3 if n % 3 == 0 else 4 if n % 4 == 0 else 1
    w = n // c
    y, x = np.mgrid[0:5, 0:w]
    img = np.stack([(x * 2 + y * 7 + (x * x) // 50 + 5 * j) for j in range(c)], axis=-1).astype(np.uint8)
    img[3] = R.noise(1, w, c, seed=row_bytes)[0]
    assert img.shape[1] * img.shape[2] + 1 == row_bytes
    for deflate in ("lz", "huffman"):
        got = _check(K, [img], "adaptive", deflate)
    R.check_file(got[0], img)


def test_two_rows_two_cuts_three_segments(shdr):
    K = shdr._ops
    w = 70000
    x = np.arange(w)
    img = np.stack([(x // 3) & 255, (x * x // 1000) & 255]).astype(np.uint8)[:, :, None]    # 2 rows of 70001 bytes: cuts at 65520 and 131040
    img[1, 60000:] = R.noise(1, 10000, 1, seed=2)[0]
    assert 2 * R.SEGMENT < 2 * (w + 1) <= 3 * R.SEGMENT
    for deflate in ("lz", "huffman"):
        got = _check(K, [img], "adaptive", deflate)
        assert len(R.check_file(got[0], img)) == 3


def test_encode_takes_lists_batches_and_grey(shdr):
    K, png = shdr._ops, shdr.png
    imgs = [R.noise(9, 14, 3, seed=1), R.noise(5, 5, 1, seed=2)[:, :, 0], R.noise(3, 8, 4, seed=3)]
    got = png.encode([torch.from_numpy(a).cuda() for a in imgs])
    assert got == png.encode(imgs, encoder="host") == [K.png_encode_host(a) for a in imgs]
    batch = np.stack([R.noise(16, 24, 3, seed=s) // 32 for s in range(4)])
    got = png.encode(torch.from_numpy(batch).cuda(), filter="paeth", deflate="huffman")
    assert got == [K.png_encode_host(a, "paeth", "huffman") for a in batch]
    with pytest.raises(TypeError, match="uint8"):
        png.encode([torch.zeros((4, 4, 3), device="cuda")])
    with pytest.raises(ValueError, match="C = 1"):
        png.encode([torch.zeros((4, 4, 2), device="cuda", dtype=torch.uint8)])
    with pytest.raises(ValueError, match="no pixels"):
        png.encode([torch.zeros((0, 4, 3), device="cuda", dtype=torch.uint8)])
    with pytest.raises(ValueError, match="filter"):
        png.encode([torch.zeros((4, 4, 3), device="cuda", dtype=torch.uint8)], filter="best")


def test_stage_times(shdr):
    K = shdr._ops
    ms = []
    files = shdr.png.encode([torch.from_numpy(R.noise(40, 50, 3)).cuda()], stage_ms=ms)
    assert len(ms) == len(K.PNG_STAGE_NAMES) == 5
    assert all(math.isfinite(v) and v >= 0 for v in ms)
    assert files == [K.png_encode_host(R.noise(40, 50, 3))]


def test_write_preview_device_png(shdr, tmp_path):
    K, io_ = shdr._ops, shdr.hdr_io
    g = torch.Generator().manual_seed(1)
    hdr = (torch.rand((37, 53, 3), generator=g) * 6.0).cuda()
    want = K.tonemap_u8(hdr.contiguous(), None, True).cpu().numpy()
    for k, options in enumerate((None, dict(filter="up", deflate="huffman"))):
        p = str(tmp_path / ("p%d.png" % k))
        io_.write_preview(p, hdr, reverse_channels=True, encoder="device_png", jpeg_options=options)
        im = Image.open(p)
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), want)
        assert open(p, "rb").read() == K.png_encode_host(want, **(options or {}))
    with pytest.raises(ValueError, match="PNG"):
        io_.write_preview(str(tmp_path / "c.jpg"), hdr, encoder="device_png")
    with pytest.raises(ValueError, match="JPEG"):
        io_.write_preview(str(tmp_path / "c.png"), hdr, encoder="device")
    with pytest.raises(ValueError, match="encoder"):
        io_.write_preview(str(tmp_path / "c.png"), hdr, encoder="host")


def test_reconstruct_files_previews(shdr, tmp_path):
    K, io_ = shdr._ops, shdr.hdr_io
    rng = np.random.default_rng(9)
    recon = io_.HdrReconstructor(lambda x: x.clone())                           # a stub inference: the geometry and the writers
    src, outs, previews, singles = [], [], [], []
    for i, (h, w) in enumerate(((64, 128), (50, 75), (128, 64))):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack((xx * 255.0 / w, yy * 255.0 / h, np.full((h, w), 40.0)), axis=-1)
        pix = np.clip(base + rng.normal(0, 2, base.shape), 0, 255).astype(np.uint8)
        src.append(str(tmp_path / ("in%d.png" % i)))
        Image.fromarray(pix).save(src[-1])
        outs.append(str(tmp_path / ("out%d.hdr" % i)))
        previews.append(str(tmp_path / ("prev%d.png" % i)))
        singles.append(str(tmp_path / ("single%d.png" % i)))
    recon.reconstruct_files(src, outs, preview_paths=previews, preview_encoder="device_png")
    for s, o, p, q in zip(src, outs, previews, singles):
        one = str(tmp_path / "one.hdr")
        recon.reconstruct_file(s, one, preview_path=q, preview_encoder="device_png")
        assert open(one, "rb").read() == open(o, "rb").read()
        assert open(p, "rb").read() == open(q, "rb").read()
        want = K.tonemap_u8(recon.reconstruct_device(io_.read_ldr(s)).contiguous(), None, True).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(p)), want)
    # the device HDR encoder beside it, and the directory loop
    outs_dev = [str(tmp_path / ("dev%d.hdr" % i)) for i in range(3)]
    prev_dev = [str(tmp_path / ("devprev%d.png" % i)) for i in range(3)]
    recon.reconstruct_files(src, outs_dev, encoder="device", preview_paths=prev_dev, preview_encoder="device_png",
                            preview_options=dict(deflate="huffman"))
    for a, b, s in zip(prev_dev, previews, src):
        assert np.array_equal(np.asarray(Image.open(a)), np.asarray(Image.open(b)))
    written = recon.reconstruct_dir(str(tmp_path), str(tmp_path / "d"), pattern="in*.png", verbose=False, preview_dir=str(tmp_path / "pv"),
                                    preview_encoder="device_png")
    assert len(written) == 3
    for i in range(3):
        assert open(str(tmp_path / "pv" / ("in%d.png" % i)), "rb").read() == open(previews[i], "rb").read()
    with pytest.raises(ValueError, match="PNG"):
        recon.reconstruct_files(src, outs, preview_paths=[p[:-4] + ".jpg" for p in previews], preview_encoder="device_png")
    with pytest.raises(ValueError, match="previews"):
        recon.reconstruct_files(src, outs, preview_paths=previews[:2], preview_encoder="device_png")
