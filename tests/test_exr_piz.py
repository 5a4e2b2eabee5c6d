"""PIZ-compressed OpenEXR files through exr.py on the host: refused by default, read with piz="host".  The files are written by
piz_ref (the tests' own PIZ codec); decoding is lossless, so pixels are compared for equality.  No GPU."""
import importlib

import numpy as np
import pytest

import exr_ref
import piz_ref

exr = importlib.import_module("singlehdr-tf2_amd.exr")
HALF, FLOAT, UINT = exr_ref.HALF, exr_ref.FLOAT, exr_ref.UINT


def channels_of(rng, h, w, extra=()):
    """R, G, B HALF (smooth: the chunks shrink) plus extra channels [(name, type)]"""
    y, x = np.mgrid[0:h, 0:w]
    ch = {n: (exr_ref.half_values(np.exp(((x * (k + 1) + y * 3) % 64) / 16.0 - 2.0) * (k + 1)), HALF) for k, n in enumerate("RGB")}
    for name, t in extra:
        if t == UINT:
            ch[name] = (((x // 4 + y // 4) % 50).astype(np.uint32), UINT)
        else:
            v = ((x // 3 + 2 * (y // 5)) % 17 / 16.0).astype(np.float32)
            ch[name] = (exr_ref.half_values(v) if t == HALF else v, t)
    return ch


def planes_of(payload):
    """{name: array [h, w]} decoded in numpy from a Payload's planar scanlines"""
    hdr = payload.header
    assert not payload.coded.any()
    dtype = {UINT: "<u4", HALF: "<f2", FLOAT: "<f4"}
    rows = payload.data.reshape(hdr.height, hdr.row_bytes)
    out = {}
    for ch in hdr.channels:
        n = exr.SAMPLE_BYTES[ch.type] * hdr.width
        out[ch.name] = np.ascontiguousarray(rows[:, ch.offset:ch.offset + n]).view(dtype[ch.type])
    return out


def test_default_still_refuses(tmp_path):
    path = str(tmp_path / "a.exr")
    piz_ref.write_exr(path, channels_of(np.random.default_rng(0), 40, 24))
    message = "PIZ compression is not supported \\(NO_COMPRESSION, RLE, ZIPS and ZIP are\\)"
    for read in (exr.read_header, exr.read_payload, exr.read_stored, exr.read_item):
        with pytest.raises(ValueError, match=message):
            read(path)
    with pytest.raises(ValueError, match="piz must be"):
        exr.read_payload(path, piz="device")
    with pytest.raises(ValueError, match="piz must be"):
        exr.read_item(path, piz="gpu")


@pytest.mark.parametrize("comp,name", [(5, "PXR24"), (6, "B44"), (7, "B44A"), (8, "DWAA"), (9, "DWAB")])
def test_other_compressions_stay_refused_in_every_mode(tmp_path, comp, name):
    path = str(tmp_path / "a.exr")
    piz_ref.write_exr(path, channels_of(np.random.default_rng(0), 8, 8), compression=comp)
    for piz in ("refuse", "host", "device"):
        with pytest.raises(ValueError, match="%s compression is not supported" % name):
            exr.read_item(path, piz=piz)


@pytest.mark.parametrize("line_order", [exr_ref.INC, exr_ref.DEC])
@pytest.mark.parametrize("origin", [(0, 0), (-7, -45)])
@pytest.mark.parametrize("extra", [(), (("A", HALF),), (("A", HALF), ("Z", FLOAT)), (("Z", UINT),)])
def test_host_reads_every_layout(tmp_path, line_order, origin, extra):
    h, w = 70, 37                                                      # three chunks, the last of 6 rows
    ch = channels_of(np.random.default_rng(1), h, w, extra)
    path = str(tmp_path / "a.exr")
    info = piz_ref.write_exr(path, ch, line_order=line_order, origin=origin)
    assert any(info["coded"])
    hdr = exr.read_header(path, piz=True)
    assert (hdr.compression, hdr.lines, hdr.n_chunks, hdr.width, hdr.height) == (exr.PIZ_COMPRESSION, 32, 3, w, h)
    assert hdr.data_window == (origin[0], origin[1], origin[0] + w - 1, origin[1] + h - 1)
    payload = exr.read_payload(path, piz="host")
    assert payload.data.tobytes() == b"".join(info["chunks"])
    got = planes_of(payload)
    assert sorted(got) == sorted(ch)
    for name, (arr, t) in ch.items():
        assert np.array_equal(got[name].view(np.uint8), np.ascontiguousarray(arr).astype(exr_ref._DTYPE[t]).view(np.uint8)), name
    same = exr.read_stored(path, piz="host")                           # the host route of the batched readers: the same Payload
    assert isinstance(same, exr.Payload) and same.data.tobytes() == payload.data.tobytes()


def test_raw_chunks_and_stored_items(tmp_path):
    rng = np.random.default_rng(2)
    ch = {n: (rng.integers(0, 1 << 16, (40, 5)).astype(np.uint16).view(np.float16), HALF) for n in "RGB"}     # noise: nothing shrinks
    path = str(tmp_path / "a.exr")
    info = piz_ref.write_exr(path, ch)
    assert not any(info["coded"])
    assert exr.read_payload(path, piz="host").data.tobytes() == b"".join(info["chunks"])
    stored = exr.read_stored(path, piz="device")
    assert isinstance(stored, exr.Stored) and stored.mode.tolist() == [0, 0]
    path2 = str(tmp_path / "b.exr")
    info2 = piz_ref.write_exr(path2, channels_of(rng, 64, 24))
    stored = exr.read_stored(path2, piz="device")
    assert stored.mode.tolist() == [1, 1] and stored.data.tobytes() == b"".join(info2["stored"])
    assert stored.offsets.tolist() == [0, 32 * info2["row_bytes"], 64 * info2["row_bytes"]]


def test_damaged_chunk_names_file_chunk_and_reason(tmp_path):
    path = str(tmp_path / "a.exr")
    piz_ref.write_exr(path, channels_of(np.random.default_rng(3), 64, 24), chunk_hook=lambda c, s: s[:len(s) // 2] if c == 1 else s)
    with pytest.raises(ValueError, match="a.exr: chunk 1: PIZ error: "):
        exr.read_payload(path, piz="host")
