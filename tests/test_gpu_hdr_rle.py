"""The device scanline encoder (csrc/hdr_rle.hip) against its exact oracle, the host routine shdr_rgbe_rle_encode: byte equality,
never a tolerance.  Widths around every boundary of the format (flat below 8 and above 32767, runs capped at 127, literal chunks of
128), heights 1 / 3 / 17, and every line family of tests/hdr_rle_ref.py in every component."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import hdr_rle_ref as R

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
IO, K, LIB = pkg.hdr_io, pkg._ops, pkg._lib

RLE_WIDTHS = (8, 9, 126, 127, 128, 129, 254, 255, 257, 300, 1000)
HEIGHTS = (1, 3, 17)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _all_families_image(w, seed):
    """every family line of width w once, four to a row (neighbouring components from different families)"""
    lines = list(R.families(w, np.random.default_rng(seed)).values())
    while len(lines) % 4:
        lines.append(lines[len(lines) % 3])
    return np.stack(lines).reshape(-1, 4, w).transpose(0, 2, 1).copy()


def _check(images):
    """device bytes == host bytes for every image of the batch, and they decode back to the pixels"""
    got = IO.rle_encode_device([_dev(a) for a in images] if len(images) > 1 else _dev(images[0]))
    assert len(got) == len(images)
    for a, data in zip(images, got):
        want = IO.rle_encode(a)
        assert len(data) == len(want), (a.shape, len(data), len(want))
        if data != want:
            i = next(k for k in range(len(want)) if data[k] != want[k])
            raise AssertionError("%s: first difference at byte %d of %d: %r != %r" % (a.shape, i, len(want), data[i:i + 8], want[i:i + 8]))
        assert np.array_equal(IO.rle_decode(data, a.shape[0], a.shape[1]), a)
    return got


@pytest.mark.parametrize("w", RLE_WIDTHS)
def test_every_family_and_height_at_width(w):
    _check([_all_families_image(w, seed=w)])
    for h in HEIGHTS:
        _check([R.family_image(h, w, seed=7 * w + h)])


@pytest.mark.parametrize("w", (7, 32768))
def test_flat_widths(w):
    for h in HEIGHTS:
        img = R.family_image(h, w, seed=w + h)
        assert _check([img])[0] == img.tobytes()


def test_longest_coded_line():
    _check([R.family_image(2, 32767, seed=3)])
    _check([_all_families_image(32767, seed=4)])


def test_real_rgbe_of_a_noisy_ramp():
    g = torch.Generator(device="cuda").manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 67, device="cuda"), torch.linspace(0, 1, 301, device="cuda"), indexing="ij")
    smooth = torch.stack((4.0 * xx, 0.5 * yy + 0.1, xx * yy), dim=-1)
    noisy = smooth * (1 + 0.02 * torch.randn(smooth.shape, device="cuda", generator=g))
    dark = torch.zeros_like(smooth)
    dark[:, 100:200] = smooth[:, 100:200]
    batch = K.rgbe_encode(torch.stack((smooth, noisy, dark)).contiguous())          # [3, 67, 301, 4]: coded as it lies, no copy
    got = IO.rle_encode_device(batch)
    host = batch.cpu().numpy()
    assert got == [IO.rle_encode(host[i]) for i in range(3)]
    assert len(got[2]) < len(got[1])                                                # zeros really are compressed
    assert IO.rle_encode_device(batch[1]) == [got[1]]                               # a single [H, W, 4] tensor


def _mixed_batch():
    return [R.family_image(3, 257, seed=11), R.family_image(17, 9, seed=12), R.family_image(3, 7, seed=13),      # flat in the middle
            R.family_image(1, 1000, seed=14), R.family_image(2, 128, seed=15), R.family_image(1, 32768, seed=16),
            R.family_image(5, 127, seed=17)]


def test_batch_of_different_sizes_and_offsets():
    images = _mixed_batch()
    _check(images)
    data, offsets = K.rgbe_rle_encode([_dev(a) for a in images])
    sizes = [len(IO.rle_encode(a)) for a in images]
    assert offsets.dtype == torch.int64 and offsets.is_cuda and data.is_cuda
    assert offsets.cpu().tolist() == [0] + np.cumsum(sizes).tolist()


def test_more_rows_than_the_scan_block_takes_in_one_step():
    """the one-block scan of the row sizes (rle_scan_kernel over scan_array of csrc/batch.h, 1024 rows a step): 4097 + 1025 rows, so
    the first image ends one row past a step and the batch two rows past another; bytes and per-image offsets against the host's"""
    images = [R.family_image(4097, 8, seed=21), R.family_image(1025, 9, seed=22)]
    _check(images)
    data, offsets = K.rgbe_rle_encode([_dev(a) for a in images])
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(IO.rle_encode(a)) for a in images]).tolist()


def test_two_runs_give_identical_bytes_and_offsets():
    tensors = [_dev(a) for a in _mixed_batch()]
    d1, o1 = K.rgbe_rle_encode(tensors)
    d2, o2 = K.rgbe_rle_encode(tensors)
    total = int(o1[-1])
    assert torch.equal(o1, o2) and torch.equal(d1[:total], d2[:total])


def test_argument_errors_come_from_the_host_checks():
    lib = LIB.load()
    img = _dev(R.family_image(3, 300, seed=1))
    with pytest.raises(RuntimeError, match="too small"):
        K.rgbe_rle_encode(img, capacity=3 * (4 + 4 * (300 + 300 // 127 + 2)) - 1)
    base = torch.zeros(3 * 300 * 4 + 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        K.rgbe_rle_encode(base[1:1 + 3 * 300 * 4].view(3, 300, 4))
    with pytest.raises(ValueError):
        K.rgbe_rle_encode(torch.zeros((3, 0, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        K.rgbe_rle_encode(torch.zeros((3, 8, 4), dtype=torch.uint8))               # a host tensor
    # the ABI itself: a shape table with W <= 0 (or H <= 0, or no images) is refused before anything is launched, the canaries stay
    out = torch.full((8192,), 0xAB, dtype=torch.uint8, device="cuda")
    offsets = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for table, n in (([[3, 0], [3, 300]], 2), ([[3, 300], [3, -5]], 2), ([[0, 300], [3, 300]], 2), ([[3, 300]], 0)):
        shapes = np.array(table, dtype=np.int32)
        shapes_dev = _dev(shapes)
        rc = lib.shdr_rgbe_rle_encode_batch(ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(shapes.ctypes.data),
                                            ctypes.c_void_p(shapes_dev.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                            ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(ws.data_ptr()), None)
        assert rc != 0 and b"rgbe_rle_encode_batch" in lib.shdr_last_error()
        need, wsb = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.shdr_rgbe_rle_encode_batch_sizes(ctypes.c_void_p(shapes.ctypes.data), n, ctypes.byref(need), ctypes.byref(wsb)) != 0
    assert lib.shdr_rgbe_rle_encode_batch(None, None, None, 1, None, 0, None, None, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and offsets.cpu().tolist() == [-7, -7, -7]
    need, wsb = ctypes.c_int64(0), ctypes.c_int64(0)
    shapes = np.array([[3, 300], [2, 7]], dtype=np.int32)
    assert lib.shdr_rgbe_rle_encode_batch_sizes(ctypes.c_void_p(shapes.ctypes.data), 2, ctypes.byref(need), ctypes.byref(wsb)) == 0
    assert need.value == 3 * (4 + 4 * (300 + 2 + 2)) + 2 * 28 and wsb.value > 0 and wsb.value % 16 == 0


def test_write_hdr_device_and_host_encoders_write_the_same_file(tmp_path):
    img = R.family_image(17, 300, seed=5)
    t = _dev(img)
    paths = [str(tmp_path / n) for n in ("dd.hdr", "dh.hdr", "hd.hdr", "hh.hdr")]
    IO.write_hdr(paths[0], t, encoder="device")
    IO.write_hdr(paths[1], t, encoder="host")
    IO.write_hdr(paths[2], img, encoder="device")
    IO.write_hdr(paths[3], img)
    files = [open(p, "rb").read() for p in paths]
    assert files[0] == files[1] == files[2] == files[3]
    assert np.array_equal(IO.read_rgbe(paths[0]), img)
    with pytest.raises(ValueError, match="encoder"):
        IO.write_hdr(paths[0], t, encoder="gpu")
    with pytest.raises(ValueError):
        IO.write_hdr(paths[0], t.float(), encoder="device")


def test_reconstruct_files_writes_what_reconstruct_file_writes(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(9)
    recon = IO.HdrReconstructor(lambda x: x.clone())                                # a stub inference: the geometry and the writers
    src, outs_dev, outs_host = [], [], []
    for i, (h, w) in enumerate(((64, 128), (50, 75), (128, 64))):                   # one with sides that are no multiple of 64
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack((xx * 255.0 / w, yy * 255.0 / h, np.full((h, w), 40.0)), axis=-1)
        base[: h // 3] = 0                                                          # a black band: long runs in the file
        pix = np.clip(base + rng.normal(0, 2, base.shape) * (base > 0), 0, 255).astype(np.uint8)
        src.append(str(tmp_path / ("in%d.jpg" % i)))
        Image.fromarray(pix).save(src[-1], quality=95)
        outs_dev.append(str(tmp_path / ("dev%d.hdr" % i)))
        outs_host.append(str(tmp_path / ("host%d.hdr" % i)))
    recon.reconstruct_files(src, outs_dev, encoder="device")
    for s, o in zip(src, outs_host):
        recon.reconstruct_file(s, o)
    for a, b in zip(outs_dev, outs_host):
        assert open(a, "rb").read() == open(b, "rb").read()
    one = str(tmp_path / "one.hdr")
    recon.reconstruct_file(src[1], one, encoder="device")
    assert open(one, "rb").read() == open(outs_host[1], "rb").read()
    (tmp_path / "d").mkdir()
    written = recon.reconstruct_dir(str(tmp_path), str(tmp_path / "d"), verbose=False, encoder="device", group=2)
    assert [open(p, "rb").read() for p in written] == [open(p, "rb").read() for p in outs_host]
    with pytest.raises(ValueError, match="encoder"):
        recon.reconstruct_files(src, outs_dev, encoder="gpu")
    with pytest.raises(ValueError, match="encoder"):
        recon.reconstruct_dir(str(tmp_path), str(tmp_path / "d"), encoder="gpu")
