"""The JPEG file decoder on the device (csrc/jpeg.hip, singlehdr-tf2_amd/jpeg.py) against PIL, byte for byte, and its
coefficients against the sequential reference (tests/jpeg_ref.py).  Files are written with PIL at test time."""
import io
import os
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref

pytestmark = pytest.mark.gpu

CASES = jpeg_ref.grid_cases()
GROUPS = sorted({c[0].rsplit("-", 1)[0] for c in CASES})               # size-layout: its qualities / variants decode as one batch


@pytest.fixture(scope="module")
def jpeg(shdr):
    return shdr.jpeg


def _noise_file(**kw):
    return jpeg_ref.encode(jpeg_ref.content(11, 256, 384, noise=True), "420", 95, **kw)


@pytest.fixture(scope="module")
def big():
    """256 x 384 pure noise at quality 95, 4:2:0, no restarts: one entropy segment of hundreds of subsequences"""
    data = _noise_file()
    return data, jpeg_ref.pil_rgb(data)


@pytest.mark.parametrize("group", GROUPS)
def test_grid_coefficients_and_pixels(jpeg, group):
    files = [(n, d) for n, d in CASES if n.rsplit("-", 1)[0] == group]
    got = jpeg.decode([d for _, d in files])
    for (name, data), rgb in zip(files, got):
        _, want = jpeg_ref.coefficients(data)
        coef = jpeg.decode_coefficients(data)
        assert len(coef) == len(want), name
        for c, (a, b) in enumerate(zip(coef, want)):
            assert a.dtype == torch.int16 and tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b), (name, c)
        pil = jpeg_ref.pil_rgb(data)
        assert rgb.dtype == torch.uint8 and rgb.is_cuda and tuple(rgb.shape) == pil.shape, name
        assert np.array_equal(rgb.cpu().numpy(), pil), name


@pytest.mark.parametrize("bits", [256, 512, 1024, 2048])
def test_every_compiled_subsequence_length(jpeg, bits):
    name, data = next(c for c in CASES if c[0] == "40x64-444-q100")
    assert np.array_equal(jpeg.decode([data], subseq_bits=bits)[0].cpu().numpy(), jpeg_ref.pil_rgb(data)), name


def test_many_subsequences_many_workgroups(jpeg, big):
    data, pil = big
    d = jpeg.Decoded([data])
    d.check()
    assert d.plan.images["n_wg"][0] > 1 and (d.plan.sub_seg >= 0).sum() >= 300 and d.plan.segs.shape[0] == 1
    assert d.passes >= 2
    assert np.array_equal(d.image(0).cpu().numpy(), pil)
    rounds = d.sync_rounds()
    assert rounds.shape == d.plan.sub_seg.shape and np.all(rounds[d.plan.sub_seg >= 0] >= 0)
    timed = jpeg.Decoded([data], stages=True)
    assert set(timed.stage_ms) == set(jpeg.STAGE_NAMES) and all(0.0 < v < 1000.0 for v in timed.stage_ms.values())
    assert torch.equal(timed.out, d.out)
    small = jpeg.Decoded([data], subseq_bits=256)                       # four times as many subsequences and workgroups
    small.check()
    assert small.plan.images["n_wg"][0] >= 4 and np.array_equal(small.image(0).cpu().numpy(), pil)


def test_more_scan_partials_than_one_step_of_their_block(jpeg):
    """scan_partials_kernel (csrc/jpeg.hip, over scan_array of csrc/batch.h) takes WG = 256 partials a step, one partial per
    SCAN_CHUNK = 1024 scanned elements: the DC sums of more than 256 * 1024 = 262144 blocks need a second step.  The smallest such
    image has 262145 = 65 * 4033 blocks of one component: 520 x 32264 grey pixels.  Every block row has a value of its own, so the DC
    differences are not zero where a row of 65 blocks begins, and the DC of the last block holds the sum over all partials."""
    bw, bh = 65, 4033
    assert bw * bh == 256 * 1024 + 1
    rows = ((np.arange(8 * bh) // 8 * 7) % 200 + 20).astype(np.uint8)
    data = jpeg_ref.encode(np.repeat(rows[:, None, None], 8 * bw, axis=1).repeat(3, axis=2), "grey", 75)
    _, want = jpeg_ref.coefficients(data)
    coef = jpeg.decode_coefficients(data)
    assert len(coef) == len(want) == 1 and tuple(coef[0].shape) == want[0].shape == (bh, bw, 64)
    assert len(set(want[0][:, 0, 0].tolist())) > 20 and want[0][-1, -1, 0] != 0
    assert np.array_equal(coef[0].cpu().numpy(), want[0])


def test_many_restart_segments(jpeg, big):
    data = _noise_file(restart_marker_blocks=5)
    hd = jpeg.parse(data)
    assert hd.restart_interval == 5 and len(hd.rst_offsets) == -(-16 * 24 // 5) - 1
    pil = jpeg_ref.pil_rgb(data)
    assert np.array_equal(pil, big[1])                                   # restart markers do not change the image
    assert np.array_equal(jpeg.decode([data])[0].cpu().numpy(), pil)


def test_batch_of_mixed_files_is_deterministic(jpeg, big):
    by_name = dict(CASES)
    items = [by_name["1x1-420-q75"], big[0], by_name["47x33-422-q100"], by_name["23x17-grey-q30"], by_name["47x33-444-rst3"],
             by_name["40x64-420-optimize"]]
    first = jpeg.decode(items)
    for item, got in zip(items, first):
        assert np.array_equal(got.cpu().numpy(), jpeg_ref.pil_rgb(item))
        assert torch.equal(got, jpeg.decode([item])[0])
    again = jpeg.Decoded(items)
    once = jpeg.Decoded(items)
    assert torch.equal(again.out, once.out) and torch.equal(again.coef, once.coef)
    assert all(torch.equal(a, again.image(i)) for i, a in enumerate(first))


@pytest.mark.parametrize("orientation", range(1, 9))
def test_exif_orientation(jpeg, shdr, tmp_path, orientation):
    exif = Image.Exif()
    exif[0x0112] = orientation
    path = str(tmp_path / "o.jpg")
    with open(path, "wb") as f:
        f.write(jpeg_ref.encode(jpeg_ref.content(3, 23, 17), "420", 90, exif=exif))
    want = torch.from_numpy(shdr.hdr_io.read_ldr(path))
    got = jpeg.decode([path])[0]
    assert got.is_contiguous() and torch.equal(got.cpu(), want)
    assert torch.equal(jpeg.read_ldr_device(path).cpu(), want)


def test_stream_shorter_than_the_header_claims(jpeg, tmp_path):
    good = jpeg_ref.encode(jpeg_ref.content(4, 47, 33), "420", 75)
    i = good.index(b"\xff\xc0")
    assert struct.unpack_from(">HH", good, i + 5) == (47, 33)
    bad = good[:i + 5] + struct.pack(">H", 95) + good[i + 7:]
    path = str(tmp_path / "short.jpg")
    with open(path, "wb") as f:
        f.write(bad)
    assert jpeg.parse(bad).height == 95                                  # the container is intact: only the device can tell
    with pytest.raises(jpeg.CorruptJpeg, match="short.jpg"):
        jpeg.decode([path])
    with pytest.raises(jpeg.CorruptJpeg, match="short.jpg"):             # in a batch, naming the damaged file; its neighbours are fine
        jpeg.decode([good, path])
    with pytest.raises(jpeg.CorruptJpeg):
        jpeg.read_ldr_device(path)
    d = jpeg.Decoded([good, path, good])
    assert d.errors.cpu().tolist()[0] == 0 and d.errors.cpu().tolist()[1] != 0 and d.errors.cpu().tolist()[2] == 0
    assert np.array_equal(d.image(0).cpu().numpy(), jpeg_ref.pil_rgb(good)) and torch.equal(d.image(0), d.image(2))
    assert np.array_equal(jpeg.decode([good])[0].cpu().numpy(), jpeg_ref.pil_rgb(good))


def test_library_refuses_bad_tables(jpeg, shdr):
    """the launchers validate the host tables: a segment that points past the byte arena never launches"""
    data = dict(CASES)["16x16-420-q75"]
    real_plan = jpeg.plan

    def broken(items, subseq_bits=jpeg.SUBSEQ_BITS):
        p = real_plan(items, subseq_bits)
        p.segs[0, 1] = 8 * p.data.size + 64
        return p
    jpeg.plan = broken
    try:
        with pytest.raises(RuntimeError, match="segment 0"):
            jpeg.Decoded([data])
    finally:
        jpeg.plan = real_plan


def _folder(tmp_path, shdr):
    specs = [((96, 80), "420"), ((64, 64), "444"), ((96, 80), "444")]
    os.makedirs(tmp_path / "HDR_gt")
    os.makedirs(tmp_path / "LDR_in")
    rng = np.random.default_rng(5)
    for i, ((h, w), layout) in enumerate(specs):
        ldr = jpeg_ref.content(20 + i, h, w)
        ldr[: h // 2] = np.clip(ldr[: h // 2].astype(np.int32) * (3 if i == 1 else 1), 0, 255)     # file 1: a half that saturates
        with open(tmp_path / "LDR_in" / ("%02d.jpg" % i), "wb") as f:
            f.write(jpeg_ref.encode(ldr, layout, 92))
        hdr = (rng.random((h, w, 3)) * 4).astype(np.float32)
        rgbe = shdr._ops.rgbe_encode(torch.from_numpy(hdr).cuda()).cpu().numpy()
        shdr.hdr_io.write_hdr(str(tmp_path / "HDR_gt" / ("%02d.hdr" % i)), rgbe)
    return str(tmp_path)


def test_hdr_real_folder_device_decoder(shdr, tmp_path):
    root = _folder(tmp_path, shdr)
    kw = dict(size=32, stride=16, seed=3, batch_size=4)
    a = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="pil", **kw)
    b = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="device", **kw)
    assert torch.equal(a.ldr_arena, b.ldr_arena) and a.shapes == b.shapes and a.candidates == b.candidates
    assert np.array_equal(a.extreme_counts, b.extreme_counts) and np.array_equal(a.means, b.means) and np.array_equal(a.keep, b.keep)
    assert len(a.candidates) > 0
    (la, ha), (lb, hb) = next(iter(a)), next(iter(b))
    assert torch.equal(la, lb) and torch.equal(ha, hb)
    with pytest.raises(ValueError, match="jpeg_decoder"):
        shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="cpu", **kw)
    # a file outside the decoder's scope and one stored rotated: the others still decode in ONE batch, the arena is the same
    calls = []
    real = shdr.jpeg.Decoded
    ldr0 = shdr.hdr_io.read_ldr(os.path.join(root, "LDR_in", "00.jpg"))
    exif = Image.Exif()
    exif[0x0112] = 3
    with open(os.path.join(root, "LDR_in", "00.jpg"), "wb") as f:
        f.write(jpeg_ref.encode(ldr0, "420", 92, progressive=True))
    ldr2 = shdr.hdr_io.read_ldr(os.path.join(root, "LDR_in", "02.jpg"))
    with open(os.path.join(root, "LDR_in", "02.jpg"), "wb") as f:
        f.write(jpeg_ref.encode(ldr2, "444", 92, exif=exif))

    class Counted(real):
        def __init__(self, items, *a, **k):
            calls.append(len(items))
            real.__init__(self, items, *a, **k)
    shdr.jpeg.Decoded = Counted
    try:
        c = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="device", **kw)
    finally:
        shdr.jpeg.Decoded = real
    assert calls == [2]
    assert torch.equal(c.ldr_arena, shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="pil", **kw).ldr_arena)


def test_reconstruct_file_device_decoder(shdr, tmp_path):
    from oracle import nets
    models = []
    for i, (k, mod) in enumerate(dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net",
                                      ref="refinement_net").items()):
        models.append(getattr(shdr, mod).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 100 + i)))
    recon = shdr.hdr_io.HdrReconstructor(shdr.pipeline.Inference(*models))
    path = str(tmp_path / "in.jpg")
    with open(path, "wb") as f:
        f.write(jpeg_ref.encode(jpeg_ref.content(6, 40, 56), "420", 90))
    recon.reconstruct_file(path, str(tmp_path / "pil.hdr"), decoder="pil")
    recon.reconstruct_file(path, str(tmp_path / "dev.hdr"), decoder="device")
    with open(tmp_path / "pil.hdr", "rb") as f, open(tmp_path / "dev.hdr", "rb") as g:
        want, got = f.read(), g.read()
    assert len(want) > 40 * 56 and want == got
    with pytest.raises(ValueError, match="decoder"):
        recon.reconstruct_file(path, str(tmp_path / "x.hdr"), decoder="gpu")


def test_read_ldr_device_falls_back_for_files_out_of_scope(jpeg, shdr, tmp_path):
    img = jpeg_ref.content(8, 33, 47)
    prog = str(tmp_path / "p.jpg")
    with open(prog, "wb") as f:
        f.write(jpeg_ref.encode(img, "420", 80, progressive=True))
    png = str(tmp_path / "p.png")
    Image.fromarray(img).save(png)
    for path in (prog, png):
        got = jpeg.read_ldr_device(path)
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), shdr.hdr_io.read_ldr(path))
    with pytest.raises(jpeg.Unsupported, match="p.jpg"):
        jpeg.decode([prog])
