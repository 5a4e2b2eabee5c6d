"""Host half of the JPEG file decoder (singlehdr-tf2_amd/jpeg.py) and the reference it is tested against (tests/jpeg_ref.py).

The reference's pixels must equal PIL's byte for byte over the whole grid: that pins the reference on this machine and settles
the edge rules (partial MCUs, the downsampled size the upsamplers run on, replication for planes of one or two columns).  Then
jpeg.parse must agree with the reference's own marker walk and with PIL, and refuse what it has to refuse."""
import io
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref

CASES = jpeg_ref.grid_cases()


@pytest.fixture(scope="module")
def jpeg(shdr):
    return shdr.jpeg


@pytest.mark.parametrize("name,data", CASES, ids=[c[0] for c in CASES])
def test_reference_equals_pil(name, data):
    assert np.array_equal(jpeg_ref.decode(data), jpeg_ref.pil_rgb(data))


@pytest.mark.parametrize("name,data", CASES, ids=[c[0] for c in CASES])
def test_parse_matches_reference_and_pil(jpeg, name, data):
    hd = jpeg.parse(data)
    ref = jpeg_ref.markers(data)
    im = Image.open(io.BytesIO(data))
    assert (hd.width, hd.height) == (ref["width"], ref["height"]) == im.size
    assert [tuple(c) for c in hd.components] == ref["comps"]
    want_layout = "grey" if im.mode == "L" else {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[ref["comps"][0][1:3]]
    assert hd.layout == want_layout == name.split("-")[1]
    assert set(hd.qtables) == set(ref["q"]) == set(im.quantization)
    for t in hd.qtables:
        assert hd.qtables[t].dtype == np.uint16 and hd.qtables[t].tolist() == ref["q"][t]
        assert sorted(hd.qtables[t].tolist()) == sorted(im.quantization[t])
    assert set(hd.htables) == set(ref["huff"])
    for k, (counts, symbols) in hd.htables.items():
        assert (counts.tolist(), symbols.tolist()) == ref["huff"][k]
    assert hd.restart_interval == ref["ri"]
    assert (hd.scan_start, hd.scan_end) == ref["scan"] and hd.rst_offsets.tolist() == ref["rst"]
    assert data[hd.scan_end:hd.scan_end + 2] == b"\xff\xd9" and hd.orientation == 1
    # the unstuffed segments, and the geometry the device is given
    stream, offs = jpeg.unstuff(data, hd)
    segs = jpeg_ref.unstuff(data, ref)
    assert [stream[a:b].tobytes() for a, b in zip(offs[:-1], offs[1:])] == segs
    mx, my, bpm, comps = jpeg.geometry(hd)
    rmx, rmy, rcomps = jpeg_ref.grid(ref)
    assert (mx, my, comps) == (rmx, rmy, rcomps) and bpm == sum(c[0] * c[1] for c in rcomps)


def test_quantisation_tables_are_pil_natural_order(jpeg):
    """PIL reports the tables in natural order too: a de-zigzag mistake cannot hide behind the sorted comparison above"""
    data = jpeg_ref.encode(jpeg_ref.content(0, 16, 16), "420", 75)
    hd, im = jpeg.parse(data), Image.open(io.BytesIO(data))
    zz = [hd.qtables[0][jpeg.ZIGZAG[k]] for k in range(64)]
    assert list(im.quantization[0]) in (hd.qtables[0].tolist(), zz)
    # Annex K luma row 0 is 16 11 10 ..., column 0 is 16 12 14 ...; at quality 75 (scale 50, half up, integer division): 8 6 5 / 8 6 7
    assert [int(hd.qtables[0][i]) for i in (0, 1, 2, 8, 16)] == [8, 6, 5, 6, 7]


def test_16_bit_quantisation_table(jpeg):
    data = bytearray(jpeg_ref.encode(jpeg_ref.content(0, 8, 8), "grey", 75))
    i = data.index(b"\xff\xdb")
    assert struct.unpack_from(">H", data, i + 2)[0] == 67 and data[i + 4] == 0
    wide = bytes([0xFF, 0xDB]) + struct.pack(">HB", 131, 0x10) + b"".join(struct.pack(">H", v * 3) for v in data[i + 5:i + 69])
    out = bytes(data[:i]) + wide + bytes(data[i + 69:])
    assert jpeg.parse(out).qtables[0].tolist() == [3 * v for v in jpeg.parse(bytes(data)).qtables[0].tolist()]
    assert jpeg.parse(out).qtables[0].tolist() == jpeg_ref.markers(out)["q"][0]


@pytest.mark.parametrize("orientation", range(1, 9))
def test_exif_orientation(jpeg, orientation, tmp_path, shdr):
    exif = Image.Exif()
    exif[0x0112] = orientation
    data = jpeg_ref.encode(jpeg_ref.content(3, 23, 17), "420", 90, exif=exif)
    assert jpeg.parse(data).orientation == orientation == jpeg_ref.markers(data)["orientation"]
    path = tmp_path / "o.jpg"
    path.write_bytes(data)
    upright = shdr.hdr_io.read_ldr(str(path))
    got = jpeg.apply_orientation(torch.from_numpy(jpeg_ref.pil_rgb(data)), orientation)
    assert got.is_contiguous() and np.array_equal(got.numpy(), upright)


def test_unsupported_files(jpeg):
    img = jpeg_ref.content(1, 33, 47)
    with pytest.raises(jpeg.Unsupported, match="progressive"):
        jpeg.parse(jpeg_ref.encode(img, "420", 80, progressive=True))
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    with pytest.raises(jpeg.Unsupported, match="4 components"):
        jpeg.parse(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG")
    with pytest.raises(jpeg.Unsupported, match="not a JPEG"):
        jpeg.parse(buf.getvalue())
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", keep_rgb=True)
    with pytest.raises(jpeg.Unsupported, match="transform=0"):
        jpeg.parse(buf.getvalue())
    with pytest.raises(jpeg.Unsupported) as exc:                         # plan() names the item
        jpeg.plan([jpeg_ref.encode(img, "444", 80), jpeg_ref.encode(img, "420", 80, progressive=True)])
    assert "bytes>" in str(exc.value) and "progressive" in str(exc.value)


def test_corrupt_files(jpeg):
    data = jpeg_ref.encode(jpeg_ref.content(2, 33, 47), "420", 80)
    with pytest.raises(jpeg.CorruptJpeg, match="EOI"):
        jpeg.parse(data[:-2])
    with pytest.raises(jpeg.CorruptJpeg, match="EOI"):
        jpeg.parse(data[:len(data) * 3 // 4])
    with pytest.raises(jpeg.CorruptJpeg, match="SOI"):
        jpeg.parse(b"\xff\xd9" + data[2:])
    i = data.index(b"\xff\xc4")
    over = bytearray(data)
    over[i + 5] = 3                                                      # three codes of length 1
    with pytest.raises(jpeg.CorruptJpeg, match="over-subscribes"):
        jpeg.parse(bytes(over))
    many = bytearray(data)
    many[i + 5 + 15] = 255                                               # 255 more codes of length 16: > 256 symbols
    many[i + 5 + 14] = 255
    with pytest.raises(jpeg.CorruptJpeg, match="symbols"):
        jpeg.parse(bytes(many))
    long = bytearray(data)
    j = data.index(b"\xff\xdb")
    long[j + 2:j + 4] = struct.pack(">H", 65000)
    with pytest.raises(jpeg.CorruptJpeg, match="runs past the end"):
        jpeg.parse(bytes(long))
    k = data.index(b"\xff\xda")
    missing = bytearray(data)
    missing[k + 6] = 0x33                                                # the first scan component selects tables DC3 / AC3
    with pytest.raises(jpeg.CorruptJpeg, match="does not define"):
        jpeg.parse(bytes(missing))
    rst = jpeg_ref.encode(jpeg_ref.content(2, 33, 47), "420", 80, restart_marker_blocks=1)
    with pytest.raises(jpeg.CorruptJpeg, match="restart segments"):     # a restart marker went missing
        jpeg.plan([rst.replace(b"\xff\xd3", b"\x12\x34", 1)])


def test_device_huffman_tables_decode_every_code(jpeg):
    """the look-ahead / maxcode / valoff tables the kernel reads give back every (code, symbol) of an optimised table"""
    data = jpeg_ref.encode(jpeg_ref.content(5, 40, 64, noise=True), "444", 100, optimize=True)
    hd = jpeg.parse(data)
    for key, (counts, symbols) in hd.htables.items():
        blob = jpeg.device_huffman(counts, symbols)
        look = blob[:1024].view(np.uint16)
        maxcode, valoff, val = blob[1024:1092].view(np.int32), blob[1092:1160].view(np.int32), blob[1160:]
        for (l, code), sym in jpeg_ref.code_book(counts.tolist(), symbols.tolist()).items():
            for tail in (0, (1 << (16 - l)) - 1):                        # the code followed by zeros / by ones
                v = (code << (16 - l)) | tail
                e = int(look[v >> 7])
                if l <= 9:
                    assert (e >> 8, e & 255) == (l, sym)
                    continue
                assert e == 0
                n = 10
                while (v >> (16 - n)) > maxcode[n]:
                    n += 1
                assert n == l and val[(v >> (16 - n)) + valoff[n]] == sym


def test_plan_lays_the_batch_out(jpeg):
    """segments on dword boundaries holding the unstuffed bytes, every workgroup inside one image, block counts per segment"""
    items = [jpeg_ref.encode(jpeg_ref.content(1, 47, 33), "420", 75, restart_marker_blocks=3),
             jpeg_ref.encode(jpeg_ref.content(2, 1, 1), "grey", 75),
             jpeg_ref.encode(jpeg_ref.content(3, 96, 128, noise=True), "444", 100)]
    p = jpeg.plan(items, 256)
    assert p.sub_seg.size % jpeg.WG == 0 and p.images["first_wg"].tolist() == np.cumsum([0] + p.images["n_wg"].tolist())[:-1].tolist()
    assert p.images["n_wg"][2] > 1                                       # the noise file spans several workgroups
    for s, row in enumerate(p.segs):
        img = row[5]
        ref = jpeg_ref.markers(items[img])
        segs = jpeg_ref.unstuff(items[img], ref)
        k = s - int(np.flatnonzero(p.segs[:, 5] == img)[0])
        assert p.data[4 * row[0]:4 * row[0] + row[1] // 8].tobytes() == segs[k] and row[1] == 8 * len(segs[k])
        slots = np.flatnonzero(p.sub_seg == s)
        assert slots.tolist() == list(range(row[2], row[2] + max(1, -(-row[1] // 256))))
        assert np.all(slots // jpeg.WG >= p.images["first_wg"][img]) and np.all(slots // jpeg.WG < p.images["first_wg"][img] + p.images["n_wg"][img])
    first = p.segs[p.segs[:, 5] == 0]
    assert first[:, 4].sum() == 3 * 3 * 6 and first[:, 4].tolist() == [18, 18, 18] and p.images["restart_interval"][0] == 3     # PIL counts MCUs: 3 x 6 blocks
    assert p.n_blocks == 3 * 3 * 6 + 1 + 3 * 12 * 16 and p.out_bytes == 3 * (47 * 33 + 1 + 96 * 128)


def _batch(jpeg, p):
    """shdr_jpeg_batch over a plan, with made-up device addresses: the launchers validate the host tables before anything else"""
    fake = 0x1000
    return jpeg.Batch(fake, fake, p.images.ctypes.data, fake, p.segs.ctypes.data, fake, p.sub_seg.ctypes.data, fake, None, None,
                      p.data.size, p.tables.size, p.sub_seg.size, p.n_blocks, p.plane_bytes, p.out_bytes, len(p.images), p.segs.shape[0],
                      p.subseq_bits, 0)


def test_library_refuses_descriptors_its_kernels_cannot_index(jpeg, shdr):
    """host-side validation of the public ABI: shapes jpeg.py never builds are refused before a launch (no device is touched)"""
    import ctypes
    lib = shdr._lib.load()
    items = [jpeg_ref.encode(jpeg_ref.content(1, 40, 64), "420", 75), jpeg_ref.encode(jpeg_ref.content(2, 16, 16), "444", 75)]

    def refused(change, message):
        p = jpeg.plan(items)
        change(p)
        rc = lib.shdr_jpeg_entropy_decode(ctypes.byref(_batch(jpeg, p)), 0x1000, 0x1000, 0x1000, None)
        assert rc < 0 and message in lib.shdr_last_error().decode(), (rc, lib.shdr_last_error())

    def tall_luma(p):                                                    # 4:4:0: h = 1, v = 2 with consistent geometry
        im = p.images[1]
        im["comp"][0]["v"], im["mcus_y"], im["blocks_per_mcu"] = 2, 1, 4
        im["comp"][1]["bh"] = im["comp"][2]["bh"] = 1
    refused(tall_luma, "image 1 component 0")

    def overlap(p):
        p.images["first_wg"][1] = 0
    refused(overlap, "workgroups must follow")

    def sampled_grey(p):
        p.images["ncomp"][1] = 1
        p.images["comp"][1][0]["h"] = 2
    refused(sampled_grey, "image 1 component 0")

    def short_arena(p):
        p.segs[0, 1] = 8 * p.data.size + 64
    refused(short_arena, "segment 0")
    # (an intact batch passes the tables; it is not launched here: there is no device)
