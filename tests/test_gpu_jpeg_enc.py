"""The baseline-JPEG writer on the device (csrc/jpeg_enc.hip, jpeg.encode) against libshdr's host twin, byte for byte and offset for
offset -- the twin itself is held to PIL's files by test_jpeg_enc_host.py -- and the closed loops through the decoder, the camera
simulator, the preview and the fine-tuning folder."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_enc_ref as R

pytestmark = pytest.mark.gpu


def _grid():
    """the host grid thinned: per layout every edge class of sizes (one pixel, whole MCUs, partial MCUs to the right / below / both,
    narrower or lower than a block, dummy blocks), the restart classes, contents and qualities cycling so that every layout meets all"""
    sizes = [(1, 1), (8, 8), (16, 16), (7, 9), (12, 3), (3, 12), (17, 33), (33, 8), (9, 40), (24, 40), (48, 64)]
    cases = []
    for li, layout in enumerate(R.LAYOUTS):
        for i, (h, w) in enumerate(sizes):
            k = i + li
            cases.append((h, w, layout, R.QUALITIES[k % 7], R.CONTENTS[k % 4], R.restart_intervals(h, w, layout)[k % 5]))
    return cases


GRID = _grid()


def _files(out, offsets):
    off = offsets.cpu().numpy()
    data = out.cpu().numpy()
    return [data[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])], off


def _guards_intact(K, info):
    g = info["guard"]
    assert g >= 64
    for raw, size in ((info["out_raw"], info["out_bytes"]), (info["workspace_raw"], info["workspace_bytes"])):
        raw = raw.cpu().numpy()
        assert raw.size == size + 2 * g
        assert (raw[:g] == K.JPEG_ENC_GUARD).all() and (raw[g + size:] == K.JPEG_ENC_GUARD).all()


def _encode_checked(K, pixels, desc, want):
    """one device call; the files, offsets and status against the host twin's files `want`; the guards; a second run"""
    info = {}
    out, offsets, status = K.jpeg_encode(pixels, desc, guard=64, info=info)
    got, off = _files(out, offsets)
    assert (status.cpu().numpy() == 0).all()
    assert off[0] == 0 and list(np.diff(off)) == [len(w) for w in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "image %d: %s" % (i, tuple(desc[i]))
    _guards_intact(K, info)
    out2, offsets2, _ = K.jpeg_encode(pixels, desc)
    assert torch.equal(offsets, offsets2) and torch.equal(out[:int(off[-1])], out2[:int(off[-1])])
    return got


def test_device_equals_host_twin_on_the_grid(shdr):
    """33 images of mixed sizes, layouts, qualities and restart intervals in ONE call"""
    K = shdr._ops
    imgs = [R.content(kind, h, w, seed=q) for h, w, layout, q, kind, rst in GRID]
    desc = K.jpeg_enc_images([(h, w) for h, w, *_ in GRID], [c[3] for c in GRID], [c[2] for c in GRID], [c[5] for c in GRID])
    want = [K.jpeg_encode_host(img, desc[i:i + 1]) for i, img in enumerate(imgs)]
    assert len(imgs) >= 8 and len({(c[0], c[1]) for c in GRID}) > 8 and {c[2] for c in GRID} == set(R.LAYOUTS)
    got = _encode_checked(K, [torch.from_numpy(a).cuda() for a in imgs], desc, want)
    # three of them against PIL directly
    for i in (3, 17, 32):
        h, w, layout, q, kind, rst = GRID[i]
        assert got[i] == R.pil_encode(imgs[i], layout, q, rst)


def test_long_segments_and_flat_content(shdr):
    """a 40 x 1000 noise image at quality 100: one segment over many tiles of the bit-stream writer and of the FF count; the same with
    restart intervals that cut it inside tiles; flat images: many blocks per output byte"""
    K = shdr._ops
    noise = R.content("noise", 40, 1000, seed=9)
    imgs = [noise, noise, noise, R.content("white", 64, 512), R.content("black", 200, 24), noise[:, :333]]
    layouts = ["444", "420", "422", "420", "444", "420"]
    desc = K.jpeg_enc_images([a.shape[:2] for a in imgs], [100, 100, 95, 75, 1, 100], layouts, [0, 7, 200, 0, 3, 1])
    want = [K.jpeg_encode_host(np.ascontiguousarray(img), desc[i:i + 1]) for i, img in enumerate(imgs)]
    assert len(want[0]) > 20 * 4096 and want[0].count(b"\xff\x00") > 100           # many tiles, many stuffed bytes
    assert len(want[3]) - 623 < (64 // 16) * (512 // 16) * 6                        # flat: less than a byte per block
    _encode_checked(K, [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in imgs], desc, want)


@pytest.mark.parametrize("restart", [0, 1])
def test_more_blocks_than_the_scan_block_takes_in_one_step(shdr, restart):
    """the one-block scans (enc_scan_kernel over scan_array of csrc/batch.h, 1024 lanes x 4 items = 4096 a step): a 4:2:0 image of
    16 x 10928 pixels is 683 MCUs = 4098 blocks, two past a step, with an 8 x 8 image behind it in the same batch"""
    K = shdr._ops
    imgs = [R.content("noise", 16, 10928, seed=5), R.content("noise", 8, 8, seed=6)]
    desc = K.jpeg_enc_images([a.shape[:2] for a in imgs], 75, "420", restart)
    assert K.jpeg_encode_blocks(desc[0:1])[0] == 4098
    want = [K.jpeg_encode_host(np.ascontiguousarray(img), desc[i:i + 1]) for i, img in enumerate(imgs)]
    _encode_checked(K, [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in imgs], desc, want)


def test_float_pixels_equal_the_uint8_they_round_to(shdr):
    K = shdr._ops
    g = torch.Generator().manual_seed(4)
    x = (torch.rand((3, 40, 56, 3), generator=g) * 1.2 - 0.1).cuda()
    x[0, :4, :4] = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255], device="cuda")                     # ties: half to even
    u8 = torch.clamp(torch.round(x * 255.0), 0, 255).to(torch.uint8)
    desc = K.jpeg_enc_images([(40, 56)] * 3, [90, 100, 30], ["420", "444", "422"], [0, 2, 0])
    a, off_a, _ = K.jpeg_encode(x, desc)
    b, off_b, _ = K.jpeg_encode(u8, desc)
    n = int(off_b[-1])
    assert torch.equal(off_a, off_b) and torch.equal(a[:n], b[:n])
    want = [K.jpeg_encode_host(u8[i].cpu().numpy(), desc[i:i + 1]) for i in range(3)]
    assert _files(b, off_b)[0] == want
    # an exact 8-bit image as floats
    exact = u8.float() / 255.0
    c, off_c, _ = K.jpeg_encode(exact, desc)
    assert torch.equal(off_c, off_b) and torch.equal(c[:n], b[:n])


COEF_CASES = R.coefficient_cases()


def test_entropy_stages_on_coefficients(shdr):
    """the coefficient cases of the host test in one call, with an out-of-range arena among them: only its status word is set, its
    range is empty, and the neighbours' bytes are right"""
    K = shdr._ops
    items = [(R.arena(w, h, layout, coef), (h, w), layout, rst) for _, w, h, layout, rst, coef in COEF_CASES]
    bad = items[2][0].copy()
    bad[len(bad) // 2, 17] = 1024                                                         # an AC of category 11
    bad2 = items[8][0].copy()
    bad2[1, 0], bad2[2, 0] = 2047, -2047                                                  # a DC difference of category 12
    bad_at = 5
    bad_items = [(bad,) + items[2][1:], (bad2,) + items[8][1:]]
    items.insert(bad_at, bad_items[0])
    items.insert(bad_at + 3, bad_items[1])
    arenas, shapes, layouts, restarts = [list(v) for v in zip(*items)]
    desc = K.jpeg_enc_images(shapes, 75, layouts, restarts)
    want = []
    for i, arena in enumerate(arenas):
        try:
            want.append(K.jpeg_encode_entropy_host(arena, desc[i:i + 1]))
        except ValueError:
            want.append(None)
    assert [i for i, w in enumerate(want) if w is None] == [bad_at, bad_at + 3]
    info = {}
    coef = torch.from_numpy(np.concatenate(arenas)).cuda()
    out, offsets, status = K.jpeg_encode_entropy(coef, desc, guard=64, info=info)
    got, off = _files(out, offsets)
    st = status.cpu().numpy()
    assert list(st) == [K.JPEG_ENC_OUT_OF_RANGE if w is None else 0 for w in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == (b if b is not None else b""), i
    _guards_intact(K, info)
    # the reference's scans, for the cases themselves
    for (name, w, h, layout, rst, c), i in zip(COEF_CASES, [i for i, x in enumerate(want) if x is not None]):
        if name in ("every-symbol-444", "constant-1023-444", "alternating-dc-420-restart-1"):
            assert got[i] == R.scan(w, h, layout, c, rst), name


def test_jpeg_encode_interface(shdr):
    """jpeg.encode: a list of images of different sizes, one [N, H, W, 3] tensor, per-image qualities; write_jpeg"""
    jpeg = shdr.jpeg
    imgs = [R.content("ramp", 23, 17), R.content("noise", 16, 48, seed=2), R.content("noise", 9, 40, seed=3)]
    got = jpeg.encode([torch.from_numpy(a).cuda() for a in imgs], quality=[50, 90, 100], subsampling="422", restart_interval=2)
    assert got == [R.pil_encode(a, "422", q, 2) for a, q in zip(imgs, (50, 90, 100))]
    assert got == jpeg.encode(imgs, quality=[50, 90, 100], subsampling="422", restart_interval=2, encoder="host")
    batch = np.stack([R.content("noise", 32, 32, seed=s) for s in range(4)])
    got = jpeg.encode(torch.from_numpy(batch).cuda())
    assert got == [R.pil_encode(a, "420", 75) for a in batch]
    with pytest.raises(ValueError, match="grey"):
        jpeg.encode(torch.zeros((8, 8), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        jpeg.encode(torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"), subsampling="440")


def test_device_decoder_reads_the_written_files(shdr):
    jpeg = shdr.jpeg
    cases = [(48, 64, "420", 90, 0), (17, 33, "422", 75, 2), (40, 24, "444", 100, 0), (33, 8, "420", 30, 1)]
    imgs = [R.content("noise" if i % 2 else "ramp", h, w, seed=i) for i, (h, w, *_) in enumerate(cases)]
    files = [jpeg.encode([torch.from_numpy(a).cuda()], quality=q, subsampling=lay, restart_interval=rst)[0]
             for a, (h, w, lay, q, rst) in zip(imgs, cases)]
    for data, rgb in zip(files, jpeg.decode(files)):
        assert np.array_equal(rgb.cpu().numpy(), np.array(Image.open(io.BytesIO(data)).convert("RGB")))


def test_camera_files_decode_to_the_round_trip(shdr, tmp_path):
    """PIL's decode of the files camera.write_ldr_jpegs writes from the float batch is K.jpeg_round_trip's image times 255, exactly"""
    K = shdr._ops
    g = torch.Generator().manual_seed(7)
    qualities = [30, 90, 93, 97, 100]
    yy, xx = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), indexing="ij")
    smooth = torch.stack([xx / 255.0, yy / 255.0, (xx + yy) / 510.0], dim=2)
    ldr = torch.stack([torch.clamp(smooth * (0.5 + 0.2 * i) + 0.1 * torch.rand((256, 256, 3), generator=g), 0, 1) for i in range(5)]).cuda()
    paths = [str(tmp_path / ("%d.jpg" % i)) for i in range(5)]
    shdr.camera.write_ldr_jpegs(ldr, paths, qualities)
    rt, _ = K.jpeg_round_trip(ldr, qualities)
    rt = (rt * 255.0).cpu().numpy()
    assert np.abs(rt - np.rint(rt)).max() < 1e-3
    for i, path in enumerate(paths):
        assert np.array_equal(np.array(Image.open(path).convert("RGB")), np.rint(rt[i]).astype(np.uint8)), qualities[i]
    # the default qualities are the simulator's
    files = shdr.camera.write_ldr_jpegs(ldr[:3], paths[:3])
    u8 = torch.clamp(torch.round(ldr[:3] * 255.0), 0, 255).to(torch.uint8).cpu().numpy()
    assert files == [R.pil_encode(u8[i], "420", q) for i, q in enumerate(shdr.camera.jpeg_qualities(3))]


def test_write_preview_device_writes_pils_bytes(shdr, tmp_path):
    io_ = shdr.hdr_io
    g = torch.Generator().manual_seed(1)
    hdr = (torch.rand((37, 53, 3), generator=g) * 6.0).cuda()
    for k, options in enumerate((None, dict(quality=90, subsampling="444"), dict(quality=60, subsampling="422", restart_interval=3))):
        a, b = str(tmp_path / ("a%d.jpg" % k)), str(tmp_path / ("b%d.jpeg" % k))
        io_.write_preview(a, hdr, reverse_channels=True, jpeg_options=options)
        io_.write_preview(b, hdr, reverse_channels=True, encoder="device", jpeg_options=options)
        assert open(a, "rb").read() == open(b, "rb").read(), options
    with pytest.raises(ValueError, match="JPEG"):
        io_.write_preview(str(tmp_path / "c.png"), hdr, encoder="device")
    with pytest.raises(ValueError, match="encoder"):
        io_.write_preview(str(tmp_path / "c.jpg"), hdr, encoder="host")


def test_hdr_real_folder_from_written_files(shdr, tmp_path):
    """a fine-tuning folder whose LDR_in files the device wrote loads the same arena as one PIL wrote"""
    rng = np.random.default_rng(5)
    specs = [((96, 80), "420", 92), ((64, 64), "444", 100), ((80, 96), "422", 85)]
    roots = [tmp_path / "device", tmp_path / "pil"]
    for root in roots:
        os.makedirs(root / "HDR_gt")
        os.makedirs(root / "LDR_in")
    for i, ((h, w), layout, q) in enumerate(specs):
        ldr = R.content("ramp", h, w) // 2 + R.content("noise", h, w, seed=i) // 4
        shdr.jpeg.write_jpeg(str(roots[0] / "LDR_in" / ("%02d.jpg" % i)), torch.from_numpy(ldr).cuda(), quality=q, subsampling=layout)
        with open(roots[1] / "LDR_in" / ("%02d.jpg" % i), "wb") as f:
            f.write(R.pil_encode(ldr, layout, q))
        rgbe = shdr._ops.rgbe_encode(torch.from_numpy((rng.random((h, w, 3)) * 4).astype(np.float32)).cuda()).cpu().numpy()
        for root in roots:
            shdr.hdr_io.write_hdr(str(root / "HDR_gt" / ("%02d.hdr" % i)), rgbe)
    kw = dict(size=32, stride=16, seed=3, batch_size=4)
    a = shdr.hdr_real.HdrRealFolder(str(roots[0]), jpeg_decoder="device", **kw)
    b = shdr.hdr_real.HdrRealFolder(str(roots[1]), jpeg_decoder="pil", **kw)
    assert torch.equal(a.ldr_arena, b.ldr_arena) and a.shapes == b.shapes and len(a.candidates) > 0
