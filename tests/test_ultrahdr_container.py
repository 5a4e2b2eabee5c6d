"""CPU tests of the gain-map JPEG container (ultrahdr.py) on the host routes: encoder="host" / decoder="host" use libshdr's host twins
and jpeg.encode(encoder="host"), so no kernel is launched here.  Pinned: both JPEG streams and the MPF index by Pillow (its MPO
plugin), both XMP packets by xml.etree, every recorded size and offset by the true byte positions, and the round trip by a bound
stated from the rules.  No foreign Ultra HDR reader has opened these files (ultrahdr.py, "PINNING")."""
import io
import struct
import xml.etree.ElementTree as ET

import numpy as np
import pytest
from PIL import Image

import gainmap_ref as R

LN2 = float(np.log(2.0))


@pytest.fixture(scope="module")
def U(shdr):
    return shdr.ultrahdr


def _pair(shape, seed):
    sdr, hdr = R.content("noise", shape, seed)
    return sdr, hdr


def _save_jpeg(sdr, **kw):
    buf = io.BytesIO()
    Image.fromarray(sdr, "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def _pixels(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


def _scan(data):
    """from the SOS marker to the end of the file"""
    return data[data.index(b"\xff\xda"):]


@pytest.fixture(scope="module")
def files(shdr, U):
    """[(file bytes, the base decoded alone, (H, W), factor, meta record of the host twin, base bytes given or None)]"""
    K = shdr._ops
    out = []

    def twin_meta(sdrs, hdrs, factor, scale):
        images, _, _ = K.gainmap_images([s.shape[:2] for s in sdrs], factor)
        _, meta = K.gainmap_encode_host(np.concatenate([s.reshape(-1, 3) for s in sdrs]), np.concatenate([h.reshape(-1, 3) for h in hdrs]),
                                        images, scale)
        return meta

    # one image, the base coded here
    sdr, hdr = _pair((31, 64), 1)
    data = U.encode([hdr], [sdr], encoder="host")[0]
    alone = _pixels(shdr.jpeg.encode([sdr], encoder="host")[0])          # the gains are taken against the primary as a viewer decodes it
    out.append((data, alone, (31, 64), 4, twin_meta([alone], [hdr], 4, None)[0], None))
    # the base given: a Pillow file with an Exif segment and 4:2:0 chroma; the SDR pixels are its decoded pixels
    exif = Image.Exif()
    exif[0x010E] = "a base with an Exif segment"
    base = _save_jpeg(_pair((40, 56), 2)[0], quality=90, exif=exif)
    sdr, hdr = _pixels(base), _pair((40, 56), 2)[1]
    data = U.encode([hdr], [sdr], factor=2, base=[base], hdr_scale=0.75, encoder="host")[0]
    out.append((data, sdr, (40, 56), 2, twin_meta([sdr], [hdr], 2, [0.75])[0], base))
    # a mixed batch in one call, one of them with a base
    shapes = [(1, 1), (9, 17), (65, 130)]
    pairs = [_pair(s, 10 + i) for i, s in enumerate(shapes)]
    base1 = _save_jpeg(pairs[1][0], quality=80)
    sdrs = [pairs[0][0], _pixels(base1), pairs[2][0]]
    hdrs = [p[1] for p in pairs]
    batch = U.encode(hdrs, sdrs, factor=[1, 8, 4], base=[None, base1, None], base_options=dict(quality=95, subsampling="444"), encoder="host")
    seen = [sdrs[i] if i == 1 else _pixels(shdr.jpeg.encode([sdrs[i]], quality=95, subsampling="444", encoder="host")[0]) for i in range(3)]
    metas = twin_meta(seen, hdrs, [1, 8, 4], None)
    for i, f in enumerate((1, 8, 4)):
        out.append((batch[i], seen[i], shapes[i], f, metas[i], base1 if i == 1 else None))
    return out


def test_pillow_opens_every_file_as_a_two_frame_mpo(U, files):
    for data, alone, shape, f, meta, base in files:
        with Image.open(io.BytesIO(data)) as im:
            assert im.format == "MPO" and im.n_frames == 2, shape
            assert im.size == (shape[1], shape[0])
            assert np.array_equal(np.array(im.convert("RGB")), alone), shape                 # frame 0: the base decoded alone
            im.seek(1)
            assert im.size == (-(-shape[1] // f), -(-shape[0] // f)), shape                  # frame 1 has the map size
            frame1 = np.array(im.convert("RGB"))
        assert np.array_equal(frame1, _pixels(U.split(data)[1])), shape                      # ... and the gain-map JPEG's pixels
        if base is not None:
            assert _scan(base)[:-2] in data and data.count(_scan(base)[:-2]) == 1, shape    # the base's coded data, verbatim


def test_recorded_sizes_and_offsets_are_the_true_byte_positions(U, files):
    for data, alone, shape, f, meta, base in files:
        primary, gm, fields = U.split(data)
        assert primary + gm == data, shape                                                    # split(encode(...)) round-trips
        start = len(data) - len(gm)
        assert data[start:start + 2] == b"\xff\xd8" and data[start - 2:start] == b"\xff\xd9"
        at = data.index(b"\xff\xe2") + 4
        assert data[at:at + 4] == b"MPF\0" and data[at + 4:at + 12] == b"MM\0*\0\0\0\x08"
        tiff = at + 4
        assert struct.unpack_from(">H", data, tiff + 8)[0] == 3
        assert struct.unpack_from(">HHI4s", data, tiff + 10) == (0xB000, 7, 4, b"0100")
        assert struct.unpack_from(">HHII", data, tiff + 22) == (0xB001, 4, 1, 2)
        assert struct.unpack_from(">HHII", data, tiff + 34) == (0xB002, 7, 32, 50)
        assert struct.unpack_from(">I", data, tiff + 46)[0] == 0
        assert struct.unpack_from(">IIIHH", data, tiff + 50) == (0x20030000, start, 0, 0, 0)
        assert struct.unpack_from(">IIIHH", data, tiff + 66) == (0, len(gm), start - tiff, 0, 0)
        assert struct.unpack_from(">H", data, at - 2)[0] == 2 + 4 + 50 + 32
        if base is not None and b"Exif\0\0" in base:
            assert data.index(b"Exif\0\0") < data.index(b"http://ns.adobe.com/xap/1.0/\0") < at


def test_both_xmp_packets_parse_and_hold_the_metadata_to_the_last_bit(U, files):
    ns = dict(hdrgm="http://ns.adobe.com/hdr-gain-map/1.0/", c="http://ns.google.com/photos/1.0/container/",
              i="http://ns.google.com/photos/1.0/container/item/", rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#")
    head = b"http://ns.adobe.com/xap/1.0/\0"
    for data, alone, shape, f, meta, base in files:
        primary, gm, fields = U.split(data)
        packets = []
        for blob in (primary, gm):
            at = blob.index(head)
            length = struct.unpack_from(">H", blob, at - 2)[0]
            assert blob[at - 4:at - 2] == b"\xff\xe1"
            packets.append(ET.fromstring(blob[at + len(head):at - 2 + length]))
        desc = packets[0].find(".//rdf:Description", ns)
        assert desc.get("{%s}Version" % ns["hdrgm"]) == "1.0"
        items = packets[0].findall(".//rdf:Seq/rdf:li/c:Item", ns)
        assert [(it.get("{%s}Semantic" % ns["i"]), it.get("{%s}Mime" % ns["i"])) for it in items] == [("Primary", "image/jpeg"), ("GainMap", "image/jpeg")]
        assert items[0].get("{%s}Length" % ns["i"]) is None and int(items[1].get("{%s}Length" % ns["i"])) == len(gm)
        g = packets[1].find(".//rdf:Description", ns)
        read = {k: g.get("{%s}%s" % (ns["hdrgm"], k)) for k in ("Version", "GainMapMin", "GainMapMax", "Gamma", "OffsetSDR", "OffsetHDR",
                                                                "HDRCapacityMin", "HDRCapacityMax", "BaseRenditionIsHDR")}
        assert read["Version"] == "1.0" and read["BaseRenditionIsHDR"] == "False"
        assert np.float32(float(read["GainMapMin"])) == meta["gain_min"] and float(read["GainMapMin"]) == float(meta["gain_min"])
        assert np.float32(float(read["GainMapMax"])) == meta["gain_max"] and float(read["GainMapMax"]) == float(meta["gain_max"])
        assert float(read["Gamma"]) == 1.0 and float(read["OffsetSDR"]) == 0.015625 and float(read["OffsetHDR"]) == 0.015625
        assert float(read["HDRCapacityMin"]) == 0.0 and float(read["HDRCapacityMax"]) == max(float(meta["gain_max"]), 2.0 ** -10)
        assert fields["GainMapMin"] == float(meta["gain_min"]) and fields["GainMapMax"] == float(meta["gain_max"])
        assert fields["HDRCapacityMax"] == float(read["HDRCapacityMax"]) and fields["BaseRenditionIsHDR"] is False
        assert gm.index(head) < gm.index(b"\xff\xdb") and gm[2:4] == b"\xff\xe0" and gm.index(head) == 2 + 2 + struct.unpack_from(">H", gm, 4)[0] + 4


def test_refusals_name_their_reason(U, files):
    sdr, hdr = _pair((40, 56), 2)
    with pytest.raises(ValueError, match="MPF APP2"):
        U.encode([hdr], [sdr], base=[files[1][0]], encoder="host")
    gm_only = U.split(files[1][0])[1]                                   # 20 x 28, with an hdrgm packet and no MPF
    small = R.content("noise", (20, 28), 3)
    with pytest.raises(ValueError, match="hdrgm XMP packet"):
        U.encode([small[1]], [small[0]], base=[gm_only], encoder="host")
    with pytest.raises(ValueError, match="is 40 x 56, the HDR image 20 x 28"):
        U.encode([small[1]], [small[0]], base=[files[1][5]], encoder="host")
    with pytest.raises(ValueError, match="not a JPEG"):
        U.encode([hdr], [sdr], base=[b"PNG"], encoder="host")
    data = files[0][0]
    with pytest.raises(ValueError, match="no MPF APP2"):
        U.split(files[1][5])
    with pytest.raises(ValueError, match="not a JPEG"):
        U.split(data[1:])
    with pytest.raises(ValueError, match="ends inside its header|runs past the end"):
        U.split(data[:40])
    with pytest.raises(ValueError, match="points outside the file"):
        U.split(data[:-1])
    at = data.index(b'Item:Length="') + len(b'Item:Length="')
    digit = b"1" if data[at:at + 1] != b"1" else b"2"
    with pytest.raises(ValueError, match="Item:Length .* disagree"):
        U.split(data[:at] + digit + data[at + 1:])
    start = len(data) - len(U.split(data)[1])
    with pytest.raises(ValueError, match="no JPEG file"):
        U.split(data[:start] + b"\x00" + data[start + 1:])
    with pytest.raises(ValueError, match="hdr_scale"):
        U.encode([hdr], [sdr], hdr_scale=-1.0, encoder="host")
    with pytest.raises(ValueError, match="factor 3"):
        U.encode([hdr], [sdr], factor=3, encoder="host")


@pytest.mark.parametrize("given", [True, False], ids=["base_given", "base_coded_444_q100"])
@pytest.mark.parametrize("scale", [None, 1.5])
def test_round_trip_recovers_the_scaled_hdr_image_within_the_stated_bound(shdr, U, scale, given):
    """decode(encode(hdr, sdr)) at f = 1, w = 1, with the map coded at 4:4:4 and quality 100, against s * hdr after rule 2 and the rule 5
    clamp: T = (lin + 1/64) 2^g - 1/64 with g the clamped gain of the pixel.  The primary is a given base and sdr its decoded pixels, or
    it is coded here at 4:4:4 and quality 100 and encode() takes the gains against its decoded pixels: the SDR side is exact either way.  Per element the decoded code differs from the real-valued code of g by at most 1/2 (quantisation) + delta
    (test_gainmap_host.py) + J, J = |decoded map - coded map| in codes, measured here; L moves by that times (max - min) / 255, the
    output by the factor 2^dL, plus the twin's own error (test_gainmap_host.py, apply)."""
    K = shdr._ops
    shape = (31, 64)
    base = _save_jpeg(R.content("ramp", shape, 5)[0], quality=92, subsampling=0)
    sdr = _pixels(base)
    hdr = R.content("noise", shape, 6)[1]
    if given:
        data = U.encode([hdr], [sdr], factor=1, hdr_scale="auto" if scale is None else scale, base=[base], map_quality=100, encoder="host")[0]
    else:
        data = U.encode([hdr], [sdr], factor=1, hdr_scale="auto" if scale is None else scale, base_options=dict(quality=100, subsampling="444"),
                        map_quality=100, encoder="host")[0]
        sdr = _pixels(U.split(data)[0])
    got = U.decode([data], decoder="host")[0]
    images, _, _ = K.gainmap_images([shape], 1)
    codes, meta = K.gainmap_encode_host(sdr.reshape(-1, 3), hdr.reshape(-1, 3), images, None if scale is None else [scale])
    s, mn, mx = float(meta[0]["scale"]), float(meta[0]["gain_min"]), float(meta[0]["gain_max"])
    decoded = _pixels(U.split(data)[1]).astype(np.float64)
    J = np.abs(decoded - codes.reshape(shape + (3,)))
    print("JPEG error of the map in codes: max %.0f, mean %.3f; max - min = %.4f" % (J.max(), J.mean(), mx - mn))
    T, bound = R.round_trip_bound(sdr, hdr, s, mn, mx, J)
    err = np.abs(got.astype(np.float64) - T)
    assert (err <= bound).all(), float((err / bound).max())
    print("largest error / bound = %.3f" % float((err / bound).max()))


def test_display_boost_weights_the_gain(U, files):
    data, alone, shape, f, meta, base = files[1]
    full = U.decode([data], decoder="host")[0]
    cap = max(float(meta["gain_max"]), 2.0 ** -10)
    assert np.array_equal(U.decode([data], display_boost=2.0 ** (cap + 1), decoder="host")[0], full)          # above the capacity: w = 1
    none = U.decode([data], display_boost=0.5, decoder="host")[0]                                             # below: w = 0, the SDR image
    lin = R.srgb_table()[alone]
    assert np.abs(none - lin).max() <= 4 * R.U * (1 + 1.0 / 64)
    half = U.decode([data], display_boost=2.0 ** (cap / 2), decoder="host")[0]
    assert U.weight_of(U.split(data)[2], 2.0 ** (cap / 2)) == pytest.approx(0.5, abs=1e-12)
    assert not np.array_equal(half, full) and not np.array_equal(half, none)


def test_write_and_read(U, tmp_path):
    sdr, hdr = _pair((16, 33), 4)
    path = str(tmp_path / "one.jpg")
    U.write(path, hdr, sdr, factor=2, encoder="host")
    with open(path, "rb") as f:
        assert f.read() == U.encode([hdr], [sdr], factor=2, encoder="host")[0]
    assert np.array_equal(U.read(path, decoder="host"), U.decode([path], decoder="host")[0])
    with pytest.raises(ValueError, match="unknown option"):
        U.write(path, hdr, sdr, quality=3)
